"""Placing an assembler's contigs on the gold-standard assembly, without a GPU: the plain restatement of the rules
(tests/_asmmap.py) on cases whose numbers are written out here by hand; the symbols of simmr_asmmap_*; the command line's usage
errors and help rows; and the report, block-row, contig-row and NGA50 routines of host.cpp in a stand-alone program under the
sanitizers.  CASES is shared with tests/test_gpu_asmmap.py, which runs every one of them on the device."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _asmmap
from tests._asmmap import NONE, fasta, revcomp_bytes
from tests._synth import synthetic_contigs

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"

K = 15
S, W = (x.tobytes() for x in synthetic_contigs([200, 200], 77))   # two unrelated sequences of 200 bases: 186 15-mers each, all distinct
G2 = ["gB", "gA"]   # (sorted by the library: gA is row 0)
P = dict(k=K, band=4, relocation=20, min_anchors=3)   # small thresholds, so that 200 bases show every class


def deletion(n):
    return S[:60] + S[60 + n:140 + n]   # 140 bases: d is 0 in front of the cut and n behind it


# name -> (truth records, contig records): the GPU test runs the same
CASES = {
    "equal": ([(b"gA|s:0-100 depth_sum=3", S[:100])], [(b"c1", S[:100])]),
    "equal_rc": ([(b"gA|s", S[:100])], [(b"c1", revcomp_bytes(S[:100]))]),
    "inter_genome": ([(b"gA|a", S[:100]), (b"gB|b", W[:100])], [(b"c1", S[:50] + W[50:100])]),
    "inter_record": ([(b"gA|a", S[:100]), (b"gA|b", W[:100])], [(b"c1", S[:50] + W[50:100])]),
    "inversion": ([(b"gA|s", S[:120])], [(b"c1", S[:40] + revcomp_bytes(S[40:80]) + S[80:120])]),
    "deletion_band": ([(b"gA|s", S)], [(b"c1", deletion(4))]),
    "deletion_band_1": ([(b"gA|s", S)], [(b"c1", deletion(5))]),
    "deletion_relocation": ([(b"gA|s", S)], [(b"c1", deletion(20))]),
    "deletion_relocation_1": ([(b"gA|s", S)], [(b"c1", deletion(21))]),
    "min_anchors": ([(b"gA|s", S)], [(b"c1", S[:K + 1]), (b"c2", S[:K + 2])]),
    "stray_merges": ([(b"gA|s", S), (b"gB|w", W)], [(b"c1", S[:40] + W[104:120] + S[56:100])]),
    "stray_differs": ([(b"gA|s", S), (b"gB|w", W)], [(b"c1", S[:40] + W[104:120] + S[70:114])]),
    "repeat": ([(b"gA|a", S[:60]), (b"gA|b", S[30:60] + W[:30])], [(b"c1", S[:60])]),
    "n_inside": ([(b"gA|s", S[:100])], [(b"c1", S[:40] + b"N" + S[41:100])]),
    "twice": ([(b"gA|s", S[:100])], [(b"c1", S[:100]), (b"c2", S[:100])]),
    "nga50_na": ([(b"gA|s", S), (b"gB|w", W)], [(b"c1", S[:60])]),
}


def run(name, **over):
    truth, contigs = CASES[name]
    m = _asmmap.evaluate([fasta(truth)], [fasta(contigs)], G2, **(P | over))
    c, by = m.read()
    assert c["contigs_unplaced"] + c["contigs_clean"] + c["contigs_local_only"] + c["contigs_misassembled"] == c["records"]
    assert c["hits"] == c["stray_hits"] + sum(int(x) for x in m.blocks()[7]) and c["runs"] >= c["runs_dropped"] + c["blocks"]
    return m, c, by, [list(r) for r in m.block_rows]


def test_the_sequences_have_no_repeat():
    keys = [key for s in (S, W) for key, _, _ in _asmmap.placed_kmers(s, K)]
    assert len(keys) == len(set(keys)) == 372


def test_a_contig_equal_to_a_truth_record_and_its_reverse_complement():
    for name, strand in (("equal", 0), ("equal_rc", 1)):
        m, c, by, blocks = run(name)
        assert (c["truth_records"], c["truth_bases"], c["truth_kmers"], c["truth_anchors"], c["truth_repeats"]) == (1, 100, 86, 86, 0)
        assert (c["records"], c["bases"], c["kmers"], c["hits"], c["stray_hits"], c["repeat_hits"], c["runs"], c["runs_dropped"]) == (1, 100, 86, 86, 0, 0, 1, 0)
        assert blocks == [[0, 0, strand, 0, 100, 0, 100, 86, 0]]
        assert (c["blocks"], c["block_bases"], c["contigs_clean"], c["misassembled_bases"]) == (1, 100, 1, 0)
        assert by.tolist() == [[100, 86, 1, 100, 100], [0, 0, 0, 0, 0]]
        assert [int(x[0]) for x in m.contigs()] == [100, 86, 1, 0, 100, 0]
    key, t, p, o = m.anchors()
    assert np.all(key[1:] > key[:-1]) and int(key.max()) < 4 ** K and set(t.tolist()) == {0} and sorted(p.tolist()) == list(range(86)) and set(o.tolist()) <= {0, 1}


def test_two_halves_of_two_genomes_and_of_two_records():
    for name, join, cls in (("inter_genome", 1, "breaks_inter_genome"), ("inter_record", 2, "breaks_inter_record")):
        m, c, by, blocks = run(name)
        # 36 15-mers inside either half, 14 across the junction
        assert (c["kmers"], c["hits"], c["runs"], c["blocks"], c["block_bases"], c[cls]) == (86, 72, 2, 2, 100, 1)
        assert blocks == [[0, 0, 0, 0, 50, 0, 50, 36, 0], [0, 1, 0, 50, 100, 50, 100, 36, join]]
        assert (c["contigs_misassembled"], c["misassembled_bases"]) == (1, 100)
        assert [int(x[0]) for x in m.contigs()] == [100, 72, 2, 0, 100, join]
    assert run("inter_genome")[2].tolist() == [[100, 86, 1, 50, 50], [100, 86, 1, 50, 50]]
    assert run("inter_record")[2].tolist() == [[200, 172, 2, 100, 50], [0, 0, 0, 0, 0]]


def test_a_middle_third_reverse_complemented():
    m, c, by, blocks = run("inversion")
    assert blocks == [[0, 0, 0, 0, 40, 0, 40, 26, 0], [0, 0, 1, 40, 80, 40, 80, 26, 3], [0, 0, 0, 80, 120, 80, 120, 26, 3]]
    assert (c["breaks_inversion"], c["contigs_misassembled"], c["hits"], c["kmers"]) == (2, 1, 78, 106)


def test_deletions_at_the_band_and_at_the_relocation_threshold():
    m, c, by, blocks = run("deletion_band")   # |dd| = band: no break; 46 + 66 hits and one more, as S[59] == S[63] makes the 15-mer at q = 59 S[63:78]
    assert S[59] == S[63] and blocks == [[0, 0, 0, 0, 140, 0, 144, 113, 0]] and (c["runs"], c["contigs_clean"]) == (1, 1)
    for name, n, join in (("deletion_band_1", 5, 5), ("deletion_relocation", 20, 5), ("deletion_relocation_1", 21, 4)):
        m, c, by, blocks = run(name)
        assert blocks == [[0, 0, 0, 0, 60, 0, 60, 46, 0], [0, 0, 0, 60, 140, 60 + n, 140 + n, 66, join]]
        assert (c["breaks_local"], c["breaks_relocation"]) == ((1, 0) if join == 5 else (0, 1))
        assert (c["contigs_local_only"], c["contigs_misassembled"], c["misassembled_bases"]) == ((1, 0, 0) if join == 5 else (0, 1, 140))
        assert by[0].tolist() == [200, 186, 2, 140, 80]


def test_a_run_of_min_anchors_minus_one_and_of_min_anchors_hits():
    m, c, by, blocks = run("min_anchors")
    assert blocks == [[1, 0, 0, 0, 17, 0, 17, 3, 0]]
    assert (c["hits"], c["stray_hits"], c["runs"], c["runs_dropped"], c["contigs_unplaced"], c["contigs_clean"]) == (5, 2, 2, 1, 1, 1)
    assert m.contigs()[3].tolist() == [NONE, 0] and m.contigs()[1].tolist() == [2, 3]


def test_a_stray_run_between_two_runs():
    m, c, by, blocks = run("stray_merges")   # the two hits on W are dropped and the runs around them lie on one diagonal
    assert blocks == [[0, 0, 0, 0, 100, 0, 100, 56, 0]]
    assert (c["hits"], c["stray_hits"], c["runs"], c["runs_dropped"], c["blocks"], c["contigs_clean"]) == (58, 2, 3, 1, 1, 1)
    m, c, by, blocks = run("stray_differs")  # d steps from 0 to 14
    assert blocks == [[0, 0, 0, 0, 40, 0, 40, 26, 0], [0, 0, 0, 56, 100, 70, 114, 30, 5]]
    assert (c["stray_hits"], c["runs_dropped"], c["breaks_local"], c["contigs_local_only"]) == (2, 1, 1, 1)


def test_a_kmer_that_occurs_twice_in_the_truth_anchors_nothing():
    m, c, by, blocks = run("repeat")
    assert (c["truth_kmers"], c["truth_anchors"], c["truth_repeats"]) == (92, 60, 16)
    assert (c["kmers"], c["hits"], c["repeat_hits"]) == (46, 30, 16)
    assert blocks == [[0, 0, 0, 0, 44, 0, 44, 30, 0]]


def test_an_n_inside_a_contig_keeps_q_counting():
    m, c, by, blocks = run("n_inside")
    assert (c["bases"], c["invalid"], c["kmers"], c["hits"], c["runs"]) == (100, 1, 71, 71, 1)
    assert blocks == [[0, 0, 0, 0, 100, 0, 100, 71, 0]]


def test_the_same_contig_twice_gives_a_block_each():
    m, c, by, blocks = run("twice")
    assert blocks == [[0, 0, 0, 0, 100, 0, 100, 86, 0], [1, 0, 0, 0, 100, 0, 100, 86, 0]]
    assert (c["runs"], c["contigs_clean"]) == (2, 2) and m.contigs()[3].tolist() == [0, 1]


def test_nga50_na_and_the_report():
    m, c, by, blocks = run("nga50_na")
    lengths, genomes = [b[4] - b[3] for b in blocks], [m.truth_genome[b[1]] for b in blocks]
    assert lengths == [60] and _asmmap.nga50(lengths, c["bases"]) == 60 and _asmmap.nga50(lengths, c["truth_bases"]) is None
    text = _asmmap.report_text(c, by, ["gA", "gB"], K, 4, 20, 3, lengths, genomes)
    assert "#NA50\t60\n#NGA50\tNA\n" in text and "#misassemblies\t0\n" in text
    assert "G\tgA\t200\t186\t1\t60\t60\tNA\t0.300000\n" in text and "G\tgB\t200\t186\t0\t0\t0\tNA\t0.000000\n" in text
    assert _asmmap.nga50([10, 30, 20, 40], 100) == 30 and _asmmap.nga50([], 0) is None


def test_the_invariances_of_the_model():
    for name, (truth, contigs) in CASES.items():
        want = _asmmap.invariants(_asmmap.evaluate([fasta(truth)], [fasta(contigs)], G2, **P))
        rc = _asmmap.evaluate([fasta([r]) for r in truth], [fasta([(n, revcomp_bytes(s))]) for n, s in contigs], G2, **P)
        assert _asmmap.invariants(rc) == want, name


# ---- the library's surface ---------------------------------------------------------------------------------------------------------
SYMBOLS = ["simmr_asmmap_create", "simmr_asmmap_destroy", "simmr_asmmap_reset", "simmr_asmmap_truth_add", "simmr_asmmap_truth_plan", "simmr_asmmap_add",
           "simmr_asmmap_read", "simmr_asmmap_anchors", "simmr_asmmap_blocks", "simmr_asmmap_contigs", "simmr_last_asmmap_ms"]


def test_symbols_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in SYMBOLS:
        assert re.search(rf"^(?:int|void) {name}\(", header, re.M), name
        assert name in _abi.SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(_abi.AsmmapCounts) == 8 * len(_abi.ASMMAP_COUNTS) == 8 * 27 and _abi.ASMMAP_COUNTS == _asmmap.COUNTS
    fields = re.search(r"typedef struct simmr_asmmap_counts \{(.*?)\} simmr_asmmap_counts;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert tuple(re.findall(r"\b([a-z_]+)\s*[,;]", fields)) == _abi.ASMMAP_COUNTS
    assert int(re.search(r"#define SIMMR_ASMMAP_GENOME_COLS (\d+)u", header).group(1)) == len(_abi.ASMMAP_GENOME_COLS) == len(_asmmap.GENOME_COLS) == 5
    assert int(re.search(r"#define SIMMR_ASMMAP_BLOCK_COLS (\d+)u", header).group(1)) == len(_abi.ASMMAP_BLOCK_COLS) == len(_asmmap.BLOCK_COLS) == 9
    for i, name in enumerate(_asmmap.JOINS[1:], 1):
        assert f"#define SIMMR_ASMMAP_{name.upper()} {i}u" in header and _abi.ASMMAP_JOINS[i] == name
    assert C.sizeof(_abi.AsmmapConfig) == 32 and "#define SIMMR_ABI_VERSION 1\n" in header


def test_calls_need_an_object():
    lib = _abi.load()
    h, n, ms = C.c_void_p(), C.c_uint64(), C.c_float()
    assert lib.simmr_asmmap_create(None, C.byref(h)) == _abi.EINVAL
    assert lib.simmr_asmmap_reset(None, C.byref(_abi.AsmmapConfig())) == _abi.EINVAL
    assert lib.simmr_asmmap_truth_add(None, None, 0) == _abi.EINVAL and lib.simmr_asmmap_add(None, None, 0) == _abi.EINVAL
    assert lib.simmr_asmmap_truth_plan(None, C.byref(n)) == _abi.EINVAL
    assert lib.simmr_asmmap_read(None, C.byref(_abi.AsmmapCounts()), None) == _abi.EINVAL
    assert lib.simmr_asmmap_anchors(None, None, None, None, None, 0) == _abi.EINVAL
    assert lib.simmr_asmmap_blocks(None, None, 0, C.byref(n)) == _abi.EINVAL
    assert lib.simmr_asmmap_contigs(None, None, None, None, None, None, None, 0, C.byref(n)) == _abi.EINVAL
    assert lib.simmr_last_asmmap_ms(None, C.byref(ms)) == _abi.EINVAL
    lib.simmr_asmmap_destroy(None)


def test_the_unit_is_built_into_the_library():
    make = (ROOT / "simmr_amd" / "csrc" / "Makefile").read_text()
    assert {"asmmap.hip", "asmmap_kernels.hip", "asmeval_front.hpp"} <= set(re.search(r"^SRCS = (.*)$", make, re.M).group(1).split())
    for line in make.split("\n"):   # wherever the library's units are compiled together, this one is among them
        if " asmeval.hip " in line and "-shared" in line:
            assert " asmmap.hip " in line, line


# ---- the command line --------------------------------------------------------------------------------------------------------------
EVAL = ["--eval-placement", "c.fa", "--eval-placement-truth", "t.fa", "--eval-placement-report", "r.tsv"]
ONLY = ("it takes only --eval-placement-truth, --eval-placement-report, --eval-placement-blocks, --eval-placement-contigs, --eval-placement-k, "
        "--eval-placement-band, --eval-placement-relocation, --eval-placement-min-anchors and --device")
USAGE_ERRORS = [
    (EVAL + ["--num-reads", "5"], f"error: --eval-placement runs no simulation: {ONLY} ('--num-reads' given)"),
    (["--genome", "g.fna"] + EVAL, f"error: --eval-placement runs no simulation: {ONLY} ('--genome' given)"),
    (EVAL + ["--devices", "0,1"], f"error: --eval-placement runs no simulation: {ONLY} ('--devices' given)"),
    (EVAL + ["--eval-assembly-k", "21"], "error: --eval-assembly-k needs --eval-assembly"),
    (EVAL[:4], "error: --eval-placement needs --eval-placement-report"),
    (EVAL[:2] + EVAL[4:], "error: --eval-placement needs --eval-placement-truth"),
    (EVAL[2:], "error: --eval-placement-truth needs --eval-placement"),
    (["--eval-placement-blocks", "x.tsv"], "error: --eval-placement-blocks needs --eval-placement"),
    (EVAL + ["--eval-placement-k", "16"], "error: invalid value '16' for '--eval-placement-k': k is odd"),
    (EVAL + ["--eval-placement-k", "33"], "error: invalid value for --eval-placement-k"),
    (EVAL + ["--eval-placement-min-anchors", "0"], "error: invalid value for --eval-placement-min-anchors"),
    (EVAL + ["--eval-placement-relocation", "2147483648"], "error: invalid value for --eval-placement-relocation"),
    (EVAL + ["--eval-placement-band", "2000"], "error: --eval-placement-band 2000 is above --eval-placement-relocation 1000"),
    (["--eval-placement"], "error: a value is required for '--eval-placement'"),
    (["--eval-placement-report="], "error: a file name is required for '--eval-placement-report'"),
]


@pytest.mark.parametrize("argv,first", USAGE_ERRORS, ids=[" ".join(a)[-60:] for a, _ in USAGE_ERRORS])
def test_cli_usage_errors(argv, first, tmp_path):
    subprocess.check_call(["make", "-s", "-C", str(HOST), "simmr-hip"])
    r = subprocess.run([str(HOST / "simmr-hip")] + argv, capture_output=True, text=True, cwd=tmp_path)
    assert (r.returncode, r.stderr.split("\n")[0]) == (2, first)
    assert not list(tmp_path.iterdir())  # nothing was written


def test_help_rows():
    subprocess.check_call(["make", "-s", "-C", str(HOST), "simmr-hip"])
    text = subprocess.run([str(HOST / "simmr-hip"), "--help"], capture_output=True, text=True, check=True).stdout
    flags = ["--eval-assembly-k <K>", "--eval-placement <FILE>", "--eval-placement-truth <FILE>", "--eval-placement-report <FILE>", "--eval-placement-blocks <FILE>",
             "--eval-placement-contigs <FILE>", "--eval-placement-k <K>", "--eval-placement-band <N>", "--eval-placement-relocation <N>",
             "--eval-placement-min-anchors <N>", "--eval-bins <FILE>"]
    at = [text.index("            " + f) for f in flags]
    assert at == sorted(at) and "no simulation" in text[at[1]:at[2]] and "--gold-assembly" in text[at[2]:at[3]] and "NGA50" in text[at[3]:at[4]]


# ---- host.cpp's routines under the sanitizers --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("asmmap") / "asmmap_report_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "asmmap_report_main.cpp"), str(HOST / "host.cpp")])
    return exe


def ask(exe, block: bytes) -> bytes:
    r = subprocess.run([str(exe)], input=block, capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    assert r.stdout.endswith(b"--\n")
    return r.stdout[:-3]


def test_report_formatter(report_main):
    rng = np.random.default_rng(13)
    names = ["gA", "gB", "z|9"]
    for case in range(5):
        counts = {n: int(v) for n, v in zip(_asmmap.COUNTS, rng.integers(0, 2 ** 40, 27))}
        by = rng.integers(0, 2 ** 40, (3, 5)).astype(np.uint64)
        nb = 0 if case == 4 else 9
        lengths = [int(x) for x in rng.integers(1, 90000, nb)]
        genomes = [int(x) for x in rng.integers(0, 3, nb)]
        if case == 1:   # reachable targets
            counts["bases"], counts["truth_bases"] = sum(lengths), sum(lengths) + 10
            by[:, 0] = [sum(l for l, g in zip(lengths, genomes) if g == r) for r in range(3)]
        if case == 2:
            counts["bases"] = counts["truth_bases"] = 0
            by[1, 0] = 0
        block = "report 21 64 1000 16 3 %d\n%s\n%s\n%s\n%s\n%s\n" % (nb, " ".join(names), " ".join(str(counts[n]) for n in _asmmap.COUNTS),
                                                                  " ".join(str(int(x)) for x in by.reshape(-1)), " ".join(map(str, lengths)), " ".join(map(str, genomes)))
        assert ask(report_main, block.encode()).decode() == _asmmap.report_text(counts, by, names, 21, 64, 1000, 16, lengths, genomes), case


def test_block_rows_contig_rows_and_nga50(report_main):
    cols = [np.array(x, dtype=np.uint32) for x in ([0, 0, 1, 7], [0, 1, 1, 9], [0, 1, 0, 1], [0, 50, 3, 1], [50, 100, 2 ** 32 - 1, 2], [5, 6, 7, 8], [55, 56, 57, 58],
                                                   [36, 36, 1, 2], [0, 1, 0, 5])]
    block = "blocks 2 2 4\nc1 c|2\ngA|a gB|b\n" + "".join(" ".join(str(int(c[i])) for c in cols) + "\n" for i in range(4))
    want = ("c1\t0\t50\tgA|a\t5\t55\t+\t36\tnone\nc1\t50\t100\tgB|b\t6\t56\t-\t36\tinter_genome\nc|2\t3\t4294967295\tgB|b\t7\t57\t+\t1\tnone\n"
            "?\t1\t2\t?\t8\t58\t-\t2\tlocal\n")
    assert ask(report_main, block.encode()).decode() == want == _asmmap.block_rows_text(["c1", "c|2"], ["gA|a", "gB|b"], cols)
    ccols = (np.array([100, 2 ** 33, 5], dtype=np.uint64), np.array([72, 0, 1], dtype=np.uint32), np.array([2, 0, 1], dtype=np.uint32),
             np.array([0, NONE, 2], dtype=np.uint32), np.array([100, 0, 2 ** 34], dtype=np.uint64), np.array([1, 0, 5], dtype=np.uint32))
    block = "contigs 2 3\nc1 c2\n" + "".join(" ".join(str(int(c[i])) for c in ccols) + "\n" for i in range(3))
    want = "c1\t100\t72\t2\t0\t100\tinter_genome\nc2\t8589934592\t0\t0\t4294967295\t0\tnone\n?\t5\t1\t1\t2\t17179869184\tlocal\n"
    assert ask(report_main, block.encode()).decode() == want == _asmmap.contig_rows_text(["c1", "c2"], ccols)
    for lengths, target in (([10, 30, 20, 40], 100), ([10, 30, 20, 40], 201), ([], 0), ([], 1), ([5], 10), ([5], 11), ([2 ** 40, 2 ** 40], 2 ** 42)):
        got = ask(report_main, ("nga50 %d %d\n%s\n" % (len(lengths), target, " ".join(map(str, lengths)))).encode()).decode()
        want = _asmmap.nga50(lengths, target)
        assert got == ("NA\n" if want is None else "%d\n" % want), (lengths, target)
