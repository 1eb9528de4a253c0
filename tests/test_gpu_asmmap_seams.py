"""simmr_asmmap_* where its kernels change trips: a lane's 32 k-mer ends, a wave's 2048, a workgroup's 8192 and a grid's second trip
(reached with a small text through SIMMR_ASMMAP_MAX_WGS); hit counts around the scans' and the sort's tiles; runs, kept runs and
blocks past 256 and past one workgroup of the engine's scan, also with one workgroup a launch; contigs without a hit; dropped runs at either end; p above 16 bits; a contig that starts where the one before it ended.
Every case is checked against the plain model for exact equality of everything (tests/test_gpu_asmmap.py: against_model).  The
constants are read from the sources."""
import os
import re
from pathlib import Path

import pytest

from tests import _asmmap
from tests._asmmap import fasta, revcomp_bytes
from tests._synth import synthetic_contigs
from tests.test_gpu_asmmap import against_model, eng  # noqa: F401  (the engine fixture)

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def constant(file, name):
    return int(re.search(rf"#define {name} (\d+)u", (CSRC / file).read_text()).group(1))


SAMSORT_TILE = constant("sam_sort_kernels.hip", "SAMSORT_TILE")
ASM_WORD = constant("asmeval_kernels.hip", "ASM_WORD")
AMAP_WG = constant("asmmap_kernels.hip", "AMAP_WG")
SCAN_THREADS, SCAN_ITEMS = (int(re.search(rf"#define {n} (\d+)\b", (CSRC / "kernels.hip").read_text()).group(1)) for n in ("SCAN_THREADS", "SCAN_ITEMS"))
SCAN_ROUND = SCAN_THREADS * SCAN_ITEMS   # the entries one workgroup of eng_scan_u32 takes
K = 15
G = ["gA", "gB"]
A, B = (x.tobytes() for x in synthetic_contigs([72000, 30000], 4343))
P = dict(k=K, band=8, relocation=100, min_anchors=4)


def test_the_constants_are_what_the_cases_assume():
    assert (SAMSORT_TILE, ASM_WORD, AMAP_WG, SCAN_THREADS, SCAN_ITEMS) == (2048, 32, 256, 256, 8)
    assert "SCAN_THREADS * SCAN_ITEMS" in (CSRC / "engine.hip").read_text()   # the scan's tile, as eng_scan_u32 launches it
    assert "SIMMR_ASMMAP_MAX_WGS" in (CSRC / "asmmap.hip").read_text()


@pytest.mark.parametrize("edge", [ASM_WORD, 64 * ASM_WORD, AMAP_WG * ASM_WORD])
def test_a_run_and_a_block_across_a_lanes_a_waves_and_a_workgroups_k_mer_ends(eng, edge):
    truth = [fasta([(b"gA|a", A[:3 * edge + 400]), (b"gB|b", B[:3 * edge + 400])])]
    for d in (-1, 0, 1):
        at = edge + d   # the position in the add at which the second run's first k-mer ends
        lead = A[:at - (K - 1) - 20] if at > K + 20 else b""
        contigs = fasta([(b"c1", lead + B[100:100 + 2 * edge]), (b"c2", A[50:50 + edge + d] + A[300 + edge:300 + 3 * edge])], width=100000)
        against_model(eng, truth, [contigs], f"edge {edge} + {d}", G, **P)


def test_a_grid_s_second_trip(eng):
    """four workgroups at most: the rolls take a second trip behind 4 x 8192 bases, the hit kernels behind 4 x 256 hits"""
    truth = [fasta([(b"gA|a", A), (b"gB|b", B)])]
    contigs = [(b"c1", A[:40000]), (b"c2", B[:9000] + A[50000:60000]), (b"c3", revcomp_bytes(A[60000:70000]))] + [
        (b"s%d" % i, (A if i % 2 else B)[20000 + 40 * i:20000 + 40 * i + 30]) for i in range(300)]
    want = _asmmap.evaluate(truth, [fasta(contigs)], G, **P)
    os.environ["SIMMR_ASMMAP_MAX_WGS"] = "4"
    try:
        against_model(eng, truth, [fasta(contigs)], "four workgroups", G, model=want, **P)
        os.environ["SIMMR_ASMMAP_MAX_WGS"] = "1"
        against_model(eng, truth, [fasta(contigs[:3])], "one workgroup", G, **P)
    finally:
        del os.environ["SIMMR_ASMMAP_MAX_WGS"]
    against_model(eng, truth, [fasta(contigs)], "the default grid", G, model=want, **P)


@pytest.mark.parametrize("hits", [255, 256, 257, 4097, SAMSORT_TILE - 1, SAMSORT_TILE, SAMSORT_TILE + 1])
def test_hit_counts_around_the_tiles(eng, hits):
    n = hits + K - 1   # a contig of n bases equal to the truth has `hits` k-mers, all anchors
    truth = [fasta([(b"gA|a", A[:n])])]
    against_model(eng, truth, [fasta([(b"c1", A[:n])])], f"{hits} hits and occurrences", G, **P)
    against_model(eng, [fasta([(b"gA|a", A[:6000])])], [fasta([(b"c1", A[:n][:6000]), (b"c2", B[:50])])], f"{hits} hits of 5986 anchors", G, **P)


def alternating(n):
    """n pieces of 30 bases (16 15-mers each), taken in turn from B and A: piece i lies 27 bases behind piece i - 2"""
    return [(A if i % 2 else B)[27 * (i // 2):27 * (i // 2) + 30] for i in range(n)]


def test_runs_kept_runs_and_blocks_past_256_and_past_one_scan_round(eng):
    """More runs, kept runs and blocks than one workgroup of the engine's scan takes (SCAN_THREADS x SCAN_ITEMS entries), so that
    the scans over the run heads, the kept marks and the block heads all cross a scan workgroup: as many short contigs alternating
    between two genomes, and one contig that alternates inside; kept and all stray.  Then the same under one workgroup a launch,
    where the kernels indexed by run, kept run and block loop."""
    n = SCAN_ROUND + 100
    assert n > SCAN_ROUND > 256 and 27 * (n // 2) + 30 <= 30000
    truth = [fasta([(b"gA|a", A[:30000]), (b"gB|b", B[:30000])])]
    pieces = alternating(n)
    short, zigzag = fasta([(b"s%d" % i, x) for i, x in enumerate(pieces)]), fasta([(b"zig", b"".join(pieces))])
    stray = P | dict(min_anchors=17)
    models = {}
    for what, text, params in (("contigs of one run", short, P), ("contigs of one stray run", short, stray), ("one contig of many runs", zigzag, P),
                               ("one contig, the runs of 16 hits stray", zigzag, stray)):
        models[what] = m = against_model(eng, truth, [text], what, G, **params)
    # (a handful of 15-mers occur twice in the 60 kbase of truth and anchor nothing, and a junction's 15-mers may happen to lengthen or
    # to add a run: the counts are near n, and what matters is that each passes the scan's workgroup)
    c = models["contigs of one run"].read()[0]
    assert c["runs"] == c["blocks"] == c["contigs_clean"] > SCAN_ROUND and c["runs_dropped"] == 0
    c = models["contigs of one stray run"].read()[0]
    assert c["runs"] == c["runs_dropped"] > SCAN_ROUND and c["blocks"] == 0 and c["stray_hits"] == c["hits"] and c["contigs_unplaced"] == n
    c = models["one contig of many runs"].read()[0]
    assert c["runs"] - c["runs_dropped"] > SCAN_ROUND and c["blocks"] > SCAN_ROUND and c["breaks_inter_genome"] > SCAN_ROUND
    c = models["one contig, the runs of 16 hits stray"].read()[0]
    assert c["runs"] > SCAN_ROUND and c["runs_dropped"] > 256 and c["blocks"] > 256
    os.environ["SIMMR_ASMMAP_MAX_WGS"] = "1"
    try:
        for what, text, params in (("contigs of one run", short, P), ("contigs of one stray run", short, stray), ("one contig of many runs", zigzag, P),
                                   ("one contig, the runs of 16 hits stray", zigzag, stray)):
            against_model(eng, truth, [text], what + ", one workgroup a launch", G, model=models[what], **params)
    finally:
        del os.environ["SIMMR_ASMMAP_MAX_WGS"]


def test_a_contig_with_no_hit_between_two_with_hits_and_dropped_runs_at_either_end(eng):
    truth = [fasta([(b"gA|a", A[:5000]), (b"gB|b", B[:5000])])]
    foreign = B[20000:20300]
    stray = B[1000:1000 + K + 2]   # three hits: below min_anchors
    contigs = [(b"c1", A[:300]), (b"none", foreign), (b"c2", A[400:700]), (b"first", stray + A[1000:1300]), (b"last", A[2000:2300] + stray),
               (b"only", stray), (b"both", stray + A[3000:3300] + stray), (b"empty", b""), (b"c3", A[4000:4300])]
    Q = P | dict(min_anchors=8)   # (a stray piece has three hits, and one or two more where the junction's 15-mers happen to continue it)
    m = against_model(eng, truth, [fasta(contigs)], "dropped runs", G, **Q)
    c = m.read()[0]
    assert (c["runs_dropped"], c["contigs_unplaced"], c["contigs_clean"]) == (5, 3, 6)
    against_model(eng, truth, [fasta([r]) for r in contigs], "dropped runs, an add a contig", G, model=m, **Q)


def test_p_above_16_bits(eng):
    truth = [fasta([(b"gB|b", B[:500]), (b"gA|a", A)])]
    assert len(A) > 65536 + 3000
    m = against_model(eng, truth, [fasta([(b"c1", A[70000:71500]), (b"c2", revcomp_bytes(A[66000:67000]) + A[68000:69000])])], "a block near the record's end", G, **P)
    assert int(m.blocks()[5].min()) > 65536 and int(m.blocks()[6].max()) == 71500


def test_the_first_hit_of_a_contig_on_the_same_diagonal_as_the_last_hit_of_the_one_before(eng):
    """c2 = the bases of the truth that follow c1's, so that with q counted on from c1 the diagonal would be the same: a contig
    boundary starts a run all the same"""
    truth = [fasta([(b"gA|a", A[:2000])])]
    m = against_model(eng, truth, [fasta([(b"c1", A[:100]), (b"c2", A[:100]), (b"c3", A[100:200])], width=100000)], "same (t, s, d)", G, **P)
    assert m.read()[0]["blocks"] == 3 and m.blocks()[8].tolist() == [0, 0, 0]
