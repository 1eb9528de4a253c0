"""The taxeval unit (simmr_taxeval_*; taxeval.hip, taxeval_kernels.hip) at the sizes where each of its pieces takes another path,
every table and column against the plain model (tests/_taxeval.py) through tests/test_gpu_taxeval.py:against_model.  The constants
are read from the sources.

  test_a_line_start_at_a_tile_and_a_chunk_edge   a line that starts on the last byte of a line-index tile, on the first and on the
      second byte of the next (k_txe_index), at the first tile's end and at the end of the scan's first chunk of 256 tiles
      (k_txe_scan's second round), on either side;
  test_the_batch_of_a_workgroup                  15, 16 and 17 lines on either side (TXE_WG_RECS lines a workgroup and batch);
  test_truth_sizes_at_the_search_rounds          1, 15, 16, 17, 255, 256, 257 and 4097 entries: mev_lower_bound's rounds, every id
      looked up and the ids between them too;
  test_lines_at_the_sort_tile_and_the_collapse   SAMSORT_TILE - 1 .. + 2 lines given unsorted: all ids single, all paired, and pairs
      that straddle a head tile's edge (TXE_HEAD_TILE sorted ids a workgroup and round);
  test_pairs_over_the_scan_chunk_edge            ... and the edge of the scan's first chunk of 256 head tiles;
  test_the_depth_of_a_chain                      chains of depth 1, 2, 254 and 255 with calls and truths at both ends; 256 refused;
  test_the_size_of_a_tree                        255, 256, 257 nodes and one more than a grid trip of k_txe_lineage takes;
  test_the_roll_up                               a star of 4097 leaves and a chain of 255;
  test_one_hot_taxon                             10 000 records that all call one taxon, against the model's single count."""
import re
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import SimmrError, _abi
from tests import _taxeval
from tests._taxeval import call, chain, tree_of, truth_line
from tests.test_gpu_taxeval import against_model, eng  # noqa: F401  (the module's engine)
from tests.test_taxeval_host import GENOMES, TAXONOMY

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def _define(name, macro):
    return int(re.search(rf"^#define\s+{macro}\s+(\d+)u?\b", (CSRC / name).read_text(), re.M).group(1))


FSAM_TILE = _define("fit_sam_kernels.hip", "FSAM_TILE")
TXE_WG_RECS = _define("taxeval_kernels.hip", "TXE_WG_RECS")
TXE_HEAD_TILE = _define("taxeval_kernels.hip", "TXE_HEAD_TILE")
TXE_BUILD_WG = _define("taxeval_kernels.hip", "TXE_BUILD_WG")
TXE_BUILD_TRIP_WGS = _define("taxeval_kernels.hip", "TXE_BUILD_TRIP_WGS")
SAMSORT_TILE = _define("sam_sort_kernels.hip", "SAMSORT_TILE")
SCAN_CHUNK = 256   # tile counts a round of sam_scan_chunks takes
assert (FSAM_TILE, TXE_WG_RECS, TXE_HEAD_TILE, TXE_BUILD_WG, SAMSORT_TILE) == (4096, 16, 256, 256, 2048)

NAMES = [g for g, _ in GENOMES]
POOL = [61, 60, 50, 55, 45, 70, 71, 81, 90, 1, 999, 0]


def truths(ids, pair=0):
    return b"".join(truth_line(i, pair, NAMES[i % 5]) for i in ids)


def calls_for(ids):
    return b"".join(call(i, POOL[i % len(POOL)]) for i in ids)


@pytest.mark.parametrize("edge", [FSAM_TILE, SCAN_CHUNK * FSAM_TILE], ids=["tile", "chunk"])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_a_line_start_at_a_tile_and_a_chunk_edge(eng, edge, d):
    def text_with_a_start_at(lines, at):
        """the lines, the one that crosses `at` made longer so that the next starts at `at`"""
        out = b""
        for k, ln in enumerate(lines):
            if at - 64 <= len(out) + len(ln) <= at:
                ln = ln[:-1] + b"x" * (at - len(out) - len(ln)) + b"\n"
                out += ln
                assert len(out) == at
                return out + b"".join(lines[k + 1:k + 4])
            out += ln
        raise AssertionError("too few lines")
    n = edge // 30 + 8
    t_lines = [truth_line(i, 0, NAMES[i % 5]) for i in range(n)]
    c_lines = [call(i, POOL[i % len(POOL)], rest="\t150\t0:116 1:3 61:20 |:| 0:5") for i in range(n)]
    truth, cand = text_with_a_start_at(t_lines, edge + d), text_with_a_start_at(c_lines, edge + d)
    assert truth[edge + d - 1:edge + d] == b"\n" and cand[edge + d - 1:edge + d] == b"\n" and len(truth) > edge + d + 30
    m = against_model(eng, [truth], [cand], f"a line start at {edge} + {d}")
    assert m.read()[0]["truth_entries"] == m.read()[0]["truth_lines"] > edge // 64 and m.read()[0]["records"] > edge // 64


@pytest.mark.parametrize("n", [TXE_WG_RECS - 1, TXE_WG_RECS, TXE_WG_RECS + 1])
def test_the_batch_of_a_workgroup(eng, n):
    m = against_model(eng, [truths(range(n))], [calls_for(range(n))], f"{n} lines a side")
    assert m.read()[0]["records"] == n and m.read()[0]["missing"] == 0


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 4097])
def test_truth_sizes_at_the_search_rounds(eng, n):
    ids = [10 + 2 * i for i in range(n)]
    m = against_model(eng, [truths(ids)], [calls_for(range(8, 10 + 2 * n + 3))], f"{n} entries, every id and the ids between")
    c = m.read()[0]
    assert c["truth_entries"] == n and c["missing"] == 0 and c["unknown_read"] == n + 5


@pytest.mark.parametrize("n", [SAMSORT_TILE - 1, SAMSORT_TILE, SAMSORT_TILE + 1, SAMSORT_TILE + 2])
def test_lines_at_the_sort_tile_and_the_collapse(eng, n):
    order = [(i * 769) % n for i in range(n)]   # (769 is prime and no divisor of these sizes: a permutation)
    assert sorted(order) == list(range(n))
    m = against_model(eng, [truths(order)], [calls_for(range(0, n, 3))], f"{n} single ids, unsorted")
    assert m.read()[0]["truth_entries"] == n and m.read()[0]["truth_paired"] == 0
    ids = [k // 2 for k in order]               # ids k // 2: all paired (one single where n is odd), the mates far apart in the text
    m = against_model(eng, [truths(ids, pair=1)], [calls_for(range(0, n // 2, 3))], f"{n} lines, all paired")
    assert m.read()[0]["truth_entries"] == (n + 1) // 2 and m.read()[0]["truth_paired"] == n // 2
    # singles first, so that a pair's two sorted lines lie on either side of place `edge`; then pairs
    for edge in (TXE_HEAD_TILE, SAMSORT_TILE - TXE_HEAD_TILE):
        single = edge - 1                       # the ids 0 .. edge - 2 single, then pairs: the first pair has the places edge - 1, edge
        ids = list(range(single)) + [single + k // 2 for k in range(n - single)]
        m = against_model(eng, [truths(ids[::-1], pair=2)], [calls_for(range(single - 2, single + 3))], f"{n} lines, a pair over place {edge}")
        assert m.reads()[2][single - 1:single + 2].tolist() == [1, 2, 2]


def test_pairs_over_the_scan_chunk_edge(eng):
    """the head counts of more than 256 head tiles: the scan's second round; a pair whose lines are the last place of head tile 255 and the first of 256"""
    edge = SCAN_CHUNK * TXE_HEAD_TILE
    single = edge - 1
    ids = list(range(single)) + [single + k // 2 for k in range(2 * TXE_HEAD_TILE + 1)]
    m = against_model(eng, [truths(ids, pair=1)], [calls_for(range(single - 2, single + 3)) + calls_for(range(0, len(ids), 97))], "a pair over the chunk edge")
    assert m.reads()[2][single - 1:single + 2].tolist() == [1, 2, 2] and m.read()[0]["truth_paired"] == TXE_HEAD_TILE


@pytest.mark.parametrize("depth", [1, 2, 254, 255])
def test_the_depth_of_a_chain(eng, depth):
    tax = chain(depth, first=5)   # the taxids 5 .. 5 + depth, the deepest a species
    genomes = [("top", 5), ("bottom", 5 + depth), ("second", 6)]
    truth = truth_line(1, 0, "top") + truth_line(2, 0, "bottom") + truth_line(3, 0, "second")
    cand = b"".join(call(r, t) for r in (1, 2, 3) for t in (5, 6, 5 + depth, 5 + depth - 1, 4))
    m = against_model(eng, [truth], [cand], f"a chain of depth {depth}", taxonomy=tax, genomes=genomes)
    assert m.tree.depth[-1] == depth and m.taxa()[1][0] == 15 and m.read()[0]["scored"] == 12
    ev = eng.classify_eval_open(tax, genomes)
    try:
        assert ev.lineage(5 + depth) == ([0, 0, 0, 0, 0, 0, 5 + depth, 0], depth) and ev.lineage(5) == ([0] * 8 if depth else None, 0)
    finally:
        ev.close()


def test_a_chain_too_deep(eng):
    with pytest.raises(_taxeval.Refused):
        _taxeval.Tree(chain(256), [])
    with pytest.raises(SimmrError) as err:
        eng.classify_eval_open(chain(256), [])
    assert err.value.code == _abi.EINVAL and "255 steps" in str(err.value)


def wide_tree(n):
    """n nodes, given in descending taxid order: a root, 8 domains .. and under them species and strains, three steps deep at the most"""
    rows = [(1, 1, 0)] + [(2 + k, 1, 1) for k in range(8)]
    for i in range(10, n + 1):
        rows.append((i, 2 + i % 8, 7) if i % 3 else (i, i - 1 if (i - 1) % 3 else 2 + i % 8, 8 if (i - 1) % 3 else 7))
    return tree_of(rows[:n][::-1])


def grid_trip(eng):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * TXE_BUILD_TRIP_WGS * TXE_BUILD_WG


@pytest.mark.parametrize("n", [255, 256, 257, "a grid trip and one"])
def test_the_size_of_a_tree(eng, n):
    n = grid_trip(eng) + 1 if isinstance(n, str) else n
    tax = wide_tree(n)
    last = int(tax[0].max())
    genomes = [("a", last), ("b", 11), ("c", last - 1)]
    truth = truth_line(1, 0, "a") + truth_line(2, 0, "b") + truth_line(3, 0, "c")
    cand = b"".join(call(r, t) for r in (1, 2, 3) for t in (last, last - 1, last - 2, 11, 12, 2, 1, last + 1))
    m = against_model(eng, [truth], [cand], f"{n} nodes", taxonomy=tax, genomes=genomes)
    assert m.tree.n == n and m.read()[0]["unknown_taxon"] == 3
    ev = eng.classify_eval_open(tax, genomes)
    try:
        for t in (1, 2, 11, 12, last - 2, last - 1, last):
            assert ev.lineage(t) == m.lineage(t), t
    finally:
        ev.close()


def test_the_roll_up(eng):
    star = tree_of([(1, 1, 1)] + [(2 + k, 1, 7) for k in range(4097)])
    genomes = [(f"g{k}", 2 + k) for k in range(0, 4097, 64)]
    truth = b"".join(truth_line(k, 0, f"g{64 * (k % len(genomes))}") for k in range(4097))
    cand = b"".join(call(k, 2 + (k * 5) % 4097) for k in range(4097))
    m = against_model(eng, [truth], [cand], "a star of 4097 leaves", taxonomy=star, genomes=genomes)
    taxid, true, called, both = m.taxa()
    assert true[0] == called[0] == both[0] == 4097 and (called[1:] == 1).all() and true[1:].sum() == 4097
    tax = chain(254, first=1)   # 255 nodes
    genomes = [("deep", 255), ("mid", 128)]
    truth = b"".join(truth_line(k, 0, "deep" if k % 2 else "mid") for k in range(300))
    cand = b"".join(call(k, 1 + (k * 7) % 255) for k in range(300))
    m = against_model(eng, [truth], [cand], "a chain of 255", taxonomy=tax, genomes=genomes)
    taxid, true, called, both = m.taxa()
    assert true[0] == called[0] == both[0] == 300 and (np.diff(true.astype(np.int64)) <= 0).all() and true[254] == 150


def test_one_hot_taxon(eng):
    n = 10_000
    truth = b"".join(truth_line(k, 0, "gStrain") for k in range(n))
    cand = b"".join(call(k, 60) for k in range(n))
    m = against_model(eng, [truth], [cand], "10 000 records on one taxon", taxonomy=TAXONOMY, genomes=GENOMES)
    taxid, true, called, both = m.taxa()
    at = {int(t): i for i, t in enumerate(taxid)}
    assert called[at[60]] == true[at[61]] == both[at[60]] == n and called[at[61]] == 0 and m.direct[1].max() == n and np.count_nonzero(m.direct) == 3
