"""The vcfeval unit (simmr_vcfeval_*; vcfeval.hip, vcfeval_kernels.hip) at the sizes where each of its pieces takes another path,
every table and column against the plain model (tests/_vcfeval.py) through tests/test_gpu_vcfeval.py:against_model.  The constants
are read from the sources.

  test_a_line_start_at_a_tile_and_a_chunk_edge   a line that starts on the last byte of a line-index tile, on the first and on the
      second byte of the next (k_vce_index), at the first tile's end and at the end of the scan's first chunk of 256 tiles
      (k_vce_scan's second round), with no line, one line and two lines behind it;
  test_the_batch_of_a_workgroup                  15, 16 and 17 lines on either side (VCE_WG_RECS lines a workgroup and batch);
  test_truth_sizes_at_the_search_rounds          1, 15, 16, 17, 255, 256, 257 and 4097 entries: mev_lower_bound's rounds, every entry
      looked up and the positions between the entries too;
  test_entries_at_the_sort_tile                  SAMSORT_TILE - 1 .. + 2 entries given in an order that is not the sorted one;
  test_neighbouring_keys_and_the_last_position   keys that differ in the name row alone and in the lowest position bit alone; POS 2^40
      in the last of three names; an MNP that runs over it;
  test_long_alleles_and_lists                    MNPs of 64 and 65 bases, four ALT alleles all called at four neighbouring truth states,
      an ALT list longer than one 16-byte group step, an INFO that pushes FORMAT past a tile edge."""
import re
from pathlib import Path

import pytest

from tests import _vcfeval
from tests._vcfeval import rec
from tests.test_gpu_vcfeval import against_model, eng  # noqa: F401  (the module's engine)

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def _define(name, macro):
    return int(re.search(rf"^#define\s+{macro}\s+(\d+)u?\b", (CSRC / name).read_text(), re.M).group(1))


FSAM_TILE = _define("fit_sam_kernels.hip", "FSAM_TILE")
VCE_WG_RECS = _define("vcfeval_kernels.hip", "VCE_WG_RECS")
VCE_MAX_MNP = _define("vcfeval_kernels.hip", "VCE_MAX_MNP")
SAMSORT_TILE = _define("sam_sort_kernels.hip", "SAMSORT_TILE")
SCAN_CHUNK = 256   # tile counts a round of sam_scan_chunks takes
assert (FSAM_TILE, VCE_WG_RECS, VCE_MAX_MNP, SAMSORT_TILE) == (4096, 16, 64, 2048)

NAMES = ["ctg_b", "ctg_a", "ctg_c"]
BASES = "ACGT"


def sites(n, first=1_000_000, step=2, chrom="ctg_a", order=None):
    """n truth records of one width, `step` positions apart: site i is BASES[i % 4] > BASES[(i + 1 + i // 4 % 3) % 4], seen by i reads"""
    idx = range(n) if order is None else order
    return b"".join(rec(chrom, first + step * i, BASES[i % 4], BASES[(i + 1 + i // 4 % 3) % 4], info=f"AD=1,{i % 1000:03d}") for i in idx)


def lookups(n, first=1_000_000, step=2, chrom="ctg_a"):
    """candidates for sites(n): every site as it is, the position behind every site (no site), every fifth with another allele,
    every seventh with another reference base"""
    out = []
    for i in range(n):
        ref, alt = BASES[i % 4], BASES[(i + 1 + i // 4 % 3) % 4]
        other = next(b for b in BASES if b not in (ref, alt))
        out.append(rec(chrom, first + step * i, ref, alt, qual=i % 300))
        out.append(rec(chrom, first + step * i + 1, ref, alt, qual=3))
        if i % 5 == 0:
            out.append(rec(chrom, first + step * i, ref, other, qual="12.5"))
        if i % 7 == 0:
            out.append(rec(chrom, first + step * i, other, alt))
    return b"".join(out)


@pytest.mark.parametrize("edge", [FSAM_TILE, SCAN_CHUNK * FSAM_TILE], ids=["tile", "chunk"])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_a_line_start_at_a_tile_and_a_chunk_edge(eng, edge, d):
    lines = _vcfeval.lines(sites(edge // 30 + 4))
    w = len(lines[0]) + 1
    assert all(len(ln) + 1 == w for ln in lines)
    k = edge // w                      # line k would start at k * w <= edge
    pad = edge + d - k * w             # ... and `pad` more bytes of INFO on the first line move it to edge + d
    if pad < 4:
        k, pad = k - 1, pad + w
    first = lines[0] + b";" + b"x" * (pad - 1)
    for extra in (0, 1, 2):            # the line at the edge is missing, the last one, followed by one more
        text = b"\n".join([first] + lines[1:k + extra]) + b"\n"
        assert (len(text) == edge + d) if extra == 0 else (text[edge + d - 1:edge + d] == b"\n" and len(text) == edge + d + extra * w)
        cand = text.replace(b"\t.\t.\tAD=", b"\t50\tPASS\tAD=")
        m = against_model(eng, [text], [cand], f"edge {edge} {d:+d}, {extra} lines behind", names=NAMES)
        c = m.read()[0]
        assert c["truth_entries"] == c["correct"] == c["sites_found"] == k + extra and c["wrong"] == 0
    assert len(text) > edge


@pytest.mark.parametrize("n", [VCE_WG_RECS - 1, VCE_WG_RECS, VCE_WG_RECS + 1])
def test_the_batch_of_a_workgroup(eng, n):
    cand = b"".join(ln + b"\n" for ln in _vcfeval.lines(lookups(n))[:n])
    m = against_model(eng, [sites(n)], [cand], f"{n} lines", names=NAMES)
    assert m.read()[0]["lines"] == n and m.read()[0]["truth_lines"] == n


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 4097])
def test_truth_sizes_at_the_search_rounds(eng, n):
    m = against_model(eng, [sites(n)], [lookups(n)], f"{n} entries", names=NAMES)
    c = m.read()[0]
    assert (c["truth_entries"], c["sites_found"], c["no_site"]) == (n, n, n)
    assert c["wrong_allele"] == (n + 4) // 5 and c["ref_mismatch"] == (n + 6) // 7 and c["sites_multiple"] == len({i for i in range(n) if i % 5 == 0 or i % 7 == 0})


@pytest.mark.parametrize("n", [SAMSORT_TILE - 1, SAMSORT_TILE, SAMSORT_TILE + 1, SAMSORT_TILE + 2])
def test_entries_at_the_sort_tile(eng, n):
    order = [(i * 1021) % n for i in range(n)] if n % 1021 else list(range(n))[::-1]   # a permutation: 1021 is prime
    assert sorted(order) == list(range(n)) and order != sorted(order)
    text = sites(n, order=order)
    m = against_model(eng, [text], [text.replace(b"\t.\t.\tAD=", b"\t7.5e1\t.\tAD=")], f"{n} entries out of order", names=NAMES)
    assert m.read()[0]["sites_found"] == n and m.read()[1][75, 0] == n and m.sites()[0].tolist() == sorted(m.sites()[0].tolist())


def test_neighbouring_keys_and_the_last_position(eng):
    last = 2 ** 40
    truth = (rec("ctg_a", 7, "A", "C", info="AD=0,1") + rec("ctg_b", 7, "A", "G", info="AD=0,2") + rec("ctg_c", 7, "A", "T", info="AD=0,3")   # the name row alone
             + rec("ctg_b", 8, "C", "A") + rec("ctg_b", 9, "G", "A")                                                                              # the lowest bit alone
             + rec("ctg_c", last, "T", "C", info="AD=9,4294967295") + rec("ctg_a", last, "T", "G") + rec("ctg_c", last - 1, "G", "C"))
    cand = (truth + rec("ctg_b", 6, "A", "G") + rec("ctg_b", 10, "A", "G") + rec("ctg_c", 8, "C", "A") + rec("ctg_a", 7, "A", "G")
            + rec("ctg_c", last - 1, "GT", "CC", qual=9)          # an MNP whose second base is the last position
            + rec("ctg_c", last, "TA", "CC", qual=8)              # ... and one whose second base lies behind it: no site
            + rec("ctg_b", last, "T", "C") + rec("ctg_d", last, "T", "C"))
    m = against_model(eng, [truth], [cand], "neighbouring keys", names=NAMES)
    c = m.read()[0]
    assert (c["truth_entries"], c["correct"], c["wrong_allele"], c["no_site"], c["unknown_contig"]) == (8, 11, 1, 5, 1)
    key = m.sites()[0].tolist()
    assert key[-1] == 2 << 40 | (last - 1) and key[-2] == 2 << 40 | (last - 2) and (1 << 40 | 6, 1 << 40 | 7, 1 << 40 | 8) == tuple(key[2:5])
    assert m.read()[2][32].tolist() == [1, 0]


def test_long_alleles_and_lists(eng):
    n = VCE_MAX_MNP
    ref = "".join(BASES[i % 4] for i in range(n + 1))
    alt = "".join(BASES[(i + 1) % 4] if i % 3 == 0 else BASES[i % 4] for i in range(n + 1))    # every third base changed
    truth = b"".join(rec("ctg_a", 500 + i, ref[i], alt[i], info=f"AD=2,{i}") for i in range(0, n + 1, 3))
    # four neighbouring truth states for one record with four alleles: the site with the first, the third, another reference, none
    truth += rec("ctg_b", 20, "A", "C") + rec("ctg_b", 21, "A", "T") + rec("ctg_b", 22, "G", "C")
    cand = rec("ctg_a", 500, ref[:n], alt[:n], qual=64) + rec("ctg_a", 500, ref, alt, qual=65) + rec("ctg_a", 500, ref[:n], alt[:n].lower(), qual=1)
    for pos in (20, 21, 22, 23):
        cand += rec("ctg_b", pos, "A", "C,G,T,a", qual=pos, fmt="GT", sample="1/2/3/4")
    cand += rec("ctg_b", 20, "A", "C,G,T,a", qual=99, fmt="GT:AD", sample="4|3:1,2,3")
    # an ALT list of 30 alleles (59 bytes), the last one called; symbolic and indel alleles between
    many = ",".join(["AA", "<DEL>", "*", "G"] * 7 + ["N", "C"])
    cand += rec("ctg_b", 20, "A", many, qual=30) + rec("ctg_b", 20, "A", many, qual=31, fmt="GT", sample="30/29/0")
    m = against_model(eng, [truth], [cand], "long alleles and lists", names=NAMES)
    c = m.read()[0]
    assert c["long_allele"] == 1 and c["ref_call_allele"] == 5 and m.sites()[4][0] == 2 and m.sites()[3][0] == 3 << 8 | 64
    assert c["symbolic"] == 14 and c["indel"] == 7 and c["correct"] == 2 * 22 + 2 + 2 and c["ref_mismatch"] == 3
    # an INFO that pushes FORMAT and the sample past a tile edge, the GT right behind it
    for d in (-3, 0, 2):
        head = rec("ctg_b", 20, "A", "C,G", qual=5, info="X", fmt="GT", sample="2")
        pad = FSAM_TILE + d - (len(head) - len(b"X\tGT\t2\n")) - 1
        line = rec("ctg_b", 20, "A", "C,G", qual=5, info="X" * pad, fmt="GT", sample="2|1")
        assert line.index(b"\tGT\t") == FSAM_TILE + d - 1
        m = against_model(eng, [truth], [line + line], f"FORMAT at the tile edge {d:+d}", names=NAMES)
        assert (m.read()[0]["correct"], m.read()[0]["wrong_allele"]) == (2, 2)
