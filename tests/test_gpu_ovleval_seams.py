"""The ovleval unit (simmr_ovleval_*; ovleval.hip, ovleval_kernels.hip) at the sizes where each of its pieces takes another path, every
table and column against the plain model (tests/_ovleval.py) through tests/test_gpu_ovleval.py:against_model.  The constants are read
from the sources.

  test_a_line_start_at_a_tile_and_a_chunk_edge   a line that starts on the last byte of a line-index tile, on the first and on the
      second byte of the next (k_ove_index), at the first tile's end and at the end of the scan's first chunk of 256 tiles
      (k_ove_scan's second round), with one line fewer, that many and one more behind it;
  test_the_batch_of_a_workgroup                  15, 16 and 17 lines on either side (OVE_WG_RECS lines a workgroup and batch);
  test_truth_sizes_at_the_search_rounds          1, 15, 16, 17, 255, 256, 257 and 4097 entries: mev_lower_bound's rounds over the entry
      keys, every entry looked up from both sides, pairs that are no entry between them, reads that are none between the reads;
  test_distinct_keys_at_the_tiles                distinct keys at 255 .. 258 (k_ove_heads' tile of 256 sorted keys and the workgroup of
      k_ove_keys / k_ove_gather), at the sort's tile of keys and of entries, as a chain (every key twice) and as a star (one key in
      every entry: tiles of k_ove_heads without a head);
  test_mates_and_wide_ids                        keys that differ in the mate bit alone next to each other in both searches, ids of 1
      and of 18 digits in one truth (the first sort over 61 bits)."""
import re
from pathlib import Path

import pytest

from tests import _ovleval
from tests._ovleval import rec
from tests.test_gpu_ovleval import against_model, eng  # noqa: F401  (the module's engine)

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def _define(name, macro):
    return int(re.search(rf"^#define\s+{macro}\s+(\d+)u?\b", (CSRC / name).read_text(), re.M).group(1))


FSAM_TILE = _define("fit_sam_kernels.hip", "FSAM_TILE")
OVE_WG_RECS = _define("ovleval_kernels.hip", "OVE_WG_RECS")
OVE_HEAD_TILE = _define("ovleval_kernels.hip", "OVE_HEAD_TILE")
SAMSORT_TILE = _define("sam_sort_kernels.hip", "SAMSORT_TILE")
SCAN_CHUNK = 256   # tile counts a round of sam_scan_chunks takes
assert (FSAM_TILE, OVE_WG_RECS, OVE_HEAD_TILE, SAMSORT_TILE) == (4096, 16, 256, 2048)


def chain(n, first=100_000, step=2, strand=lambda i: "+-"[i % 3 == 0]):
    """n entries over n + 1 reads: read i overlaps read i + 1; lines of one width while the ids keep their digits"""
    return b"".join(rec(first + step * i, 5000, 1000 + i % 1000, 3000 + i % 1000, strand(i), first + step * (i + 1), 5000, 1000, 3000 + i % 1000) for i in range(n))


def lookups(n, first=100_000, step=2):
    """candidates for chain(n): every entry from the other side, the pair (i, i + 2) that is no entry, a read between two reads"""
    out = []
    for i in range(n):
        a, b = first + step * i, first + step * (i + 1)
        out.append(rec(b, 5000, 1000, 3000 + i % 1000, "+-"[i % 3 == 0], a, 5000, 1000 + i % 1000, 3000 + i % 1000))
        out.append(rec(a, 5000, 0, 10, "+", b + step, 5000, 0, 10))          # no entry; at the chain's end no read either
        out.append(rec(a + 1, 5000, 0, 10, "+", b, 5000, 0, 10))             # a + 1 is no read
        if i % 5 == 0:
            out.append(rec(a, 5000, 2990 + i % 1000, 3000 + i % 1000, "+-"[i % 3 == 0], b, 5000, 1000, 3000 + i % 1000))   # ten bases of 2000
    return b"".join(out)


@pytest.mark.parametrize("edge", [FSAM_TILE, SCAN_CHUNK * FSAM_TILE], ids=["tile", "chunk"])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_a_line_start_at_a_tile_and_a_chunk_edge(eng, edge, d):
    body = chain(edge // 40 + 4)
    lines = _ovleval.lines(body)
    w = len(lines[0]) + 1
    assert all(len(ln) + 1 == w for ln in lines)
    k = edge // w                      # line k would start at k * w <= edge
    pad = edge + d - k * w             # ... and a tag of `pad` bytes on the first line moves it to edge + d
    if pad < 4:
        k, pad = k - 1, pad + w
    first = lines[0] + b"\t" + b"x" * (pad - 1)
    for extra in (0, 1, 2):            # the line at the edge is missing, the last one, followed by one more
        text = b"\n".join([first] + lines[1:k + extra]) + b"\n"
        assert (len(text) == edge + d) if extra == 0 else (text[edge + d - 1:edge + d] == b"\n" and len(text) == edge + d + extra * w)
        cand = _ovleval.derive(text, outside_id=7)
        m = against_model(eng, [text], [text + cand], f"edge {edge} {d:+d}, {extra} lines behind")
        assert m.read()[0]["truth_entries"] == k + extra
    assert len(text) > edge


@pytest.mark.parametrize("n", [OVE_WG_RECS - 1, OVE_WG_RECS, OVE_WG_RECS + 1])
def test_the_batch_of_a_workgroup(eng, n):
    truth = chain(n)
    cand = b"".join(ln + b"\n" for ln in _ovleval.lines(lookups(n))[:n])
    m = against_model(eng, [truth], [cand], f"{n} lines")
    assert m.read()[0]["lines"] == n and m.read()[0]["truth_lines"] == n


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 4097])
def test_truth_sizes_at_the_search_rounds(eng, n):
    m = against_model(eng, [chain(n)], [lookups(n)], f"{n} entries")
    c = m.read()[0]
    assert (c["truth_entries"], c["truth_reads"], c["pairs_found"]) == (n, n + 1, n)
    assert c["no_pair"] == n - 1 and c["unknown_read"] == n + 1 and c["wrong_interval"] == (n + 4) // 5 and c["pairs_multiple"] == (n + 4) // 5


@pytest.mark.parametrize("reads", [OVE_HEAD_TILE - 1, OVE_HEAD_TILE, OVE_HEAD_TILE + 1, OVE_HEAD_TILE + 2, SAMSORT_TILE // 2, SAMSORT_TILE // 2 + 1,
                                   SAMSORT_TILE - 1, SAMSORT_TILE, SAMSORT_TILE + 1, SAMSORT_TILE + 2])
def test_distinct_keys_at_the_tiles(eng, reads):
    n = reads - 1
    m = against_model(eng, [chain(n)], [lookups(n)], f"a chain of {reads} reads")
    assert m.read()[0]["truth_reads"] == reads
    # a star: read 500 000 with every other read, so its key stands in every entry and whole tiles of sorted keys hold no head;
    # half the partners below it, half above, and the entries in an order that is not the sorted one
    hub = 500_000
    others = [hub - 1 - i for i in range(n // 2)] + [hub + 1 + i for i in range(n - n // 2)]
    star = b"".join(rec(o, 9000, i, 4000 + i, "+-"[i % 2], hub, 90_000, 2 * i, 2 * i + 4000) if i % 3 else rec(hub, 90_000, 2 * i, 2 * i + 4000, "+-"[i % 2], o, 9000, i, 4000 + i)
                    for i, o in enumerate(others[::-1]))
    cand = _ovleval.derive(star, outside_id=hub + 10 ** 6) + rec(others[0], 9000, 0, 10, "+", others[-1], 9000, 0, 10)
    m = against_model(eng, [star], [cand], f"a star of {reads} reads")
    assert m.read()[0]["truth_reads"] == reads and m.read()[0]["no_pair"] == (1 if n > 1 else 0)


def test_mates_and_wide_ids(eng):
    big = 10 ** 18 - 1
    ids = [0, 1, 2, 9, 10, 99, 10 ** 9, 2 ** 32, 2 ** 32 + 1, big - 1, big]
    truth = []
    for a, b in zip(ids, ids[1:]):
        truth += [rec(f"{a}/1", 700, 0, 600, "+", f"{a}/2", 700, 100, 700), rec(f"{a}/2", 700, 0, 500, "-", f"{b}/1", 700, 200, 700), rec(a, 700, 5, 600, "-", f"{b}/2", 700, 0, 0)]
    truth = b"".join(truth)
    swapped = truth.replace(b"/1\t", b"/9\t").replace(b"/2\t", b"/1\t").replace(b"/9\t", b"/2\t")   # every mate for the other
    m = against_model(eng, [truth], [truth + swapped + _ovleval.derive(truth, outside_id=big - 2)], "mates and wide ids")
    c = m.read()[0]
    assert c["truth_reads"] == 2 * len(ids) and c["no_pair"] > 0 and c["correct"] > len(ids) and m.pairs()[1].max() == big << 1 | 1
