"""Scoring an assembler's contigs against the gold-standard assembly, without a GPU: the plain restatement of the rules
(tests/_asmeval.py) on cases whose numbers are written out here by hand; the symbols of simmr_asmeval_*; the command line's usage
errors and help rows; the build facts of the new translation unit; and the report, contig-row, FASTA-record and contiguity routines
of host.cpp in a stand-alone program under the sanitizers."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _asmeval
from tests._asmeval import NONE, fasta, revcomp_bytes
from tests._scaffold import sorts_through_the_pair_sort
from tests._synth import synthetic_contigs

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "simmr_amd" / "csrc"
HOST = ROOT / "simmr_amd" / "host"

K = 15
S, W = (x.tobytes() for x in synthetic_contigs([40, 40], 77))   # two unrelated sequences of 40 bases: 26 15-mers each, all distinct
G2 = ["gB", "gA"]   # (sorted by the library: gA is row 0)


def run(truth, contigs, genomes=G2, k=K):
    m = _asmeval.evaluate([fasta(truth)], [fasta(contigs)], genomes, k)
    c, by = m.read()
    assert c["contigs_short"] + c["contigs_novel"] + c["contigs_pure"] + c["contigs_mixed"] + c["contigs_shared_only"] == c["records"]
    assert c["novel"] == c["kmers"] - c["found"]
    return m, c, by


def test_the_sequences_have_no_repeat():
    keys = list(_asmeval.canonical_kmers(S, K)) + list(_asmeval.canonical_kmers(W, K))
    assert len(keys) == len(set(keys)) == 52


def test_a_contig_equal_to_a_truth_record_and_its_reverse_complement():
    for contig in (S, revcomp_bytes(S)):
        m, c, by = run([(b"gA|s:0-40 depth_sum=3", S)], [(b"c1", contig)])
        assert (c["truth_records"], c["truth_bases"], c["truth_kmers"], c["truth_distinct"], c["truth_shared_distinct"]) == (1, 40, 26, 26, 0)
        assert (c["records"], c["bases"], c["kmers"], c["found"], c["shared"], c["novel"], c["contigs_pure"]) == (1, 40, 26, 26, 0, 0, 1)
        assert by.tolist() == [[26, 26, 0, 1, 40], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
        assert [int(x[0]) for x in m.contigs()] == [40, 26, 26, 0, 0, 26]
        assert set(m.entries()[2].tolist()) == {1} and set(m.entries()[3].tolist()) == {1}
    keys = m.entries()[0]
    assert np.all(keys[1:] > keys[:-1]) and int(keys.max()) < 4 ** K


def test_one_substitution_loses_k_kmers():
    sub = bytearray(S)
    sub[20] = ord("A") if S[20:21] != b"A" else ord("C")
    m, c, by = run([(b"gA|s", S)], [(b"c1", bytes(sub))])
    assert (c["kmers"], c["found"], c["novel"], c["contigs_pure"]) == (26, 11, 15, 1)
    assert by[0].tolist() == [26, 11, 0, 1, 40]


def test_two_genomes_that_share_a_stretch():
    m, c, by = run([(b"gA|s", S), (b"gB|s", S[10:30] + W[:20])], [(b"c1", S[10:30])])
    # S[10:30] holds 6 15-mers, in both genomes; gB's record has 26 of which 6 are those
    assert (c["truth_kmers"], c["truth_distinct"], c["truth_shared_distinct"]) == (52, 46, 6)
    assert (c["kmers"], c["found"], c["shared"], c["contigs_shared_only"], c["contigs_pure"]) == (6, 6, 6, 1, 0)
    assert [int(x[0]) for x in m.contigs()] == [20, 6, 6, 6, NONE, 0]
    assert by.tolist() == [[20, 0, 0, 0, 0], [20, 0, 0, 0, 0], [6, 6, 0, 0, 0]]
    assert sorted(m.entries()[2].tolist()) == [1] * 40 + [2] * 6


def test_a_chimeric_contig_is_mixed_and_the_tie_goes_to_the_lowest_row():
    m, c, by = run([(b"gA|s", S), (b"gB|s", W)], [(b"c1", W[:20] + S[:20])])
    # 6 15-mers inside either half, 14 across the junction
    assert (c["kmers"], c["found"], c["novel"], c["contigs_mixed"]) == (26, 12, 14, 1)
    assert [int(x[0]) for x in m.contigs()] == [40, 26, 12, 0, 0, 6]
    assert by[0].tolist() == [26, 6, 0, 1, 40] and by[1].tolist() == [26, 6, 0, 0, 0]
    m, c, by = run([(b"gA|s", S), (b"gB|s", W)], [(b"c1", W[:21] + b"N" + S[:20])])
    assert [int(x[0]) for x in m.contigs()][4:] == [1, 7]


def test_a_duplicated_contig_shows_in_over():
    m, c, by = run([(b"gA|s", S)], [(b"c1", S), (b"c2", revcomp_bytes(S)), (b"c3", W)])
    assert by[0].tolist() == [26, 26, 26, 2, 80] and (c["contigs_pure"], c["contigs_novel"], c["novel"]) == (2, 1, 26)
    assert set(m.entries()[3].tolist()) == {2}
    m, c, by = run([(b"gA|s", S), (b"gA|t", S)], [(b"c1", S), (b"c2", S)])   # the truth holds it twice too
    assert by[0].tolist() == [26, 26, 0, 2, 80] and set(m.entries()[2].tolist()) == {2}


def test_an_n_in_either_side():
    n = S[:20] + b"N" + S[21:]
    m, c, by = run([(b"gA|s", n)], [(b"c1", S)])
    assert (c["truth_bases"], c["truth_invalid"], c["truth_kmers"]) == (40, 1, 11) and (c["kmers"], c["found"], c["novel"]) == (26, 11, 15)
    m, c, by = run([(b"gA|s", S)], [(b"c1", n)])
    assert (c["bases"], c["invalid"], c["kmers"], c["found"], c["novel"]) == (40, 1, 11, 11, 0) and by[0].tolist() == [26, 11, 0, 1, 40]
    m, c, by = run([(b"gA|s", S)], [(b"c1", S[:20] + b"-*" + S[20:])])   # any other byte is a position and ends the k-mers
    assert (c["bases"], c["invalid"], c["kmers"]) == (42, 2, 12)


def test_records_of_k_minus_one_k_and_k_plus_one_bases():
    m, c, by = run([(b"gA|s", S)], [(b"c1", S[:K - 1]), (b"c2", S[:K]), (b"c3", S[:K + 1]), (b"c4", b"")])
    assert m.contigs()[0].tolist() == [14, 15, 16, 0] and m.contigs()[1].tolist() == [0, 1, 2, 0]
    assert (c["records"], c["contigs_short"], c["contigs_pure"], c["kmers"]) == (4, 2, 2, 3)
    m, c, by = run([(b"gA|s", S[:K - 1]), (b"gA|t", S[:K])], [])
    assert (c["truth_records"], c["truth_kmers"], c["truth_distinct"]) == (2, 1, 1)


def test_line_ends_case_and_the_last_line():
    want = run([(b"gA|s", S)], [(b"c1", S)])[0]
    for truth, contigs in ((fasta([(b"gA|s", S)], 7, b"\r\n"), fasta([(b"c1", S)], 1, b"\r\n")),
                           (fasta([(b"gA|s", S)])[:-1], fasta([(b"c1", S)], 13)[:-1]),
                           (fasta([(b"gA|s", S.lower())]), b"\n\n" + fasta([(b"c1", S[:9].lower() + S[9:])], 3).replace(b"\n", b"\n\n"))):
        m = _asmeval.evaluate([truth], [contigs], G2, K)
        assert m.read()[0] == want.read()[0] and all(np.array_equal(a, b) for a, b in zip(m.entries() + m.contigs(), want.entries() + want.contigs()))
    # a '\r' that ends a last line without '\n' is a byte like any other; a '>' inside a line is one too
    c = _asmeval.evaluate([b">gA|s\n" + S + b"\r"], [b">c1\n" + S[:20] + b">" + S[20:]], G2, K).read()[0]
    assert (c["truth_bases"], c["truth_invalid"], c["truth_kmers"]) == (41, 1, 26) and (c["bases"], c["invalid"], c["kmers"], c["records"]) == (41, 1, 12, 1)


def test_what_is_malformed():
    for bad in (b"ACGT\n>gA|x\nACGT\n", b">gA\nACGT\n", b">gA x|y\nACGT\n", b">gZ|x\nACGT\n", b">|x\nACGT\n"):
        with pytest.raises(_asmeval.Malformed):
            _asmeval.evaluate([bad], [], G2, K)
    with pytest.raises(_asmeval.Malformed):
        _asmeval.evaluate([], [b"ACGT\n>c\n"], G2, K)
    _asmeval.evaluate([b"\r\n\n>gA|x\n"], [b"\n>c"], G2, K)


# ---- the library's surface ---------------------------------------------------------------------------------------------------------
SYMBOLS = ["simmr_asmeval_create", "simmr_asmeval_destroy", "simmr_asmeval_reset", "simmr_asmeval_truth_add", "simmr_asmeval_truth_plan", "simmr_asmeval_add",
           "simmr_asmeval_read", "simmr_asmeval_emit", "simmr_asmeval_contigs", "simmr_last_asmeval_ms"]


def test_symbols_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in SYMBOLS:
        assert re.search(rf"^(?:int|void) {name}\(", header, re.M), name
        assert name in _abi.SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(_abi.AsmevalCounts) == 8 * len(_abi.ASMEVAL_COUNTS) == 8 * 18 and _abi.ASMEVAL_COUNTS == _asmeval.COUNTS
    fields = re.search(r"typedef struct simmr_asmeval_counts \{(.*?)\} simmr_asmeval_counts;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert tuple(re.findall(r"\b([a-z_]+)\s*[,;]", fields)) == _abi.ASMEVAL_COUNTS
    assert int(re.search(r"#define SIMMR_ASMEVAL_GENOME_COLS (\d+)u", header).group(1)) == len(_abi.ASMEVAL_GENOME_COLS) == len(_asmeval.GENOME_COLS) == 5
    assert int(re.search(r"#define SIMMR_ASMEVAL_MAX_BYTES (0x[0-9a-f]+)ull", header).group(1), 16) == _abi.ASMEVAL_MAX_BYTES == 2 ** 31 - 1
    assert C.sizeof(_abi.AsmevalConfig) == 24 and "#define SIMMR_ABI_VERSION 1\n" in header


def test_calls_need_an_object():
    lib = _abi.load()
    h, n, ms = C.c_void_p(), C.c_uint64(), C.c_float()
    assert lib.simmr_asmeval_create(None, C.byref(h)) == _abi.EINVAL
    assert lib.simmr_asmeval_reset(None, C.byref(_abi.AsmevalConfig())) == _abi.EINVAL
    assert lib.simmr_asmeval_truth_add(None, None, 0) == _abi.EINVAL and lib.simmr_asmeval_add(None, None, 0) == _abi.EINVAL
    assert lib.simmr_asmeval_truth_plan(None, C.byref(n)) == _abi.EINVAL
    assert lib.simmr_asmeval_read(None, C.byref(_abi.AsmevalCounts()), None) == _abi.EINVAL
    assert lib.simmr_asmeval_emit(None, None, None, None, None, 0) == _abi.EINVAL
    assert lib.simmr_asmeval_contigs(None, None, None, None, None, None, None, 0, C.byref(n)) == _abi.EINVAL
    assert lib.simmr_last_asmeval_ms(None, C.byref(ms), None) == _abi.EINVAL
    lib.simmr_asmeval_destroy(None)


def test_the_unit_is_built_without_a_slot_of_the_engine():
    make = (CSRC / "Makefile").read_text()
    assert make.count(" asmeval.hip taxeval.hip vcfeval.hip ") == 2
    srcs = re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
    assert {"asmeval.hip", "asmeval_kernels.hip"} <= set(srcs)
    assert "ENG_EXT_COUNT = 12" in (CSRC / "engine_internal.hpp").read_text()
    unit = (CSRC / "asmeval.hip").read_text()
    assert "eng_ext_slot" not in unit and "unit_state" not in unit and '#include "engine.hip"' not in unit and '#include "kernels.hip"' not in unit
    assert '#include "host_support.hpp"' in unit and "Spans<" in unit and sorts_through_the_pair_sort("asmeval.hip") and "eng_scan_u32(" in unit


# ---- the command line --------------------------------------------------------------------------------------------------------------
EVAL = ["--eval-assembly", "c.fa", "--eval-assembly-truth", "t.fa", "--eval-assembly-report", "r.tsv"]
ONLY = "it takes only --eval-assembly-truth, --eval-assembly-report, --eval-assembly-contigs, --eval-assembly-k and --device"
USAGE_ERRORS = [
    (EVAL + ["--num-reads", "5"], f"error: --eval-assembly runs no simulation: {ONLY} ('--num-reads' given)"),
    (["--genome", "g.fna"] + EVAL, f"error: --eval-assembly runs no simulation: {ONLY} ('--genome' given)"),
    (EVAL + ["--output", "x.fq"], f"error: --eval-assembly runs no simulation: {ONLY} ('--output' given)"),
    (EVAL + ["--gold-assembly", "x.fa"], f"error: --eval-assembly runs no simulation: {ONLY} ('--gold-assembly' given)"),
    (EVAL + ["--devices", "0,1"], f"error: --eval-assembly runs no simulation: {ONLY} ('--devices' given)"),
    (EVAL + ["--eval-vcf", "a.vcf", "--eval-vcf-truth", "t.vcf", "--eval-vcf-report", "r2.tsv"],
     "error: --eval-vcf runs no simulation: it takes only --eval-vcf-truth, --eval-vcf-report, --eval-vcf-sites, --eval-vcf-filtered and --device "
     "('--eval-assembly' given)"),
    (EVAL[:4], "error: --eval-assembly needs --eval-assembly-report"),
    (EVAL[:2] + EVAL[4:], "error: --eval-assembly needs --eval-assembly-truth"),
    (EVAL[2:], "error: --eval-assembly-truth needs --eval-assembly"),
    (["--eval-assembly-contigs", "x.tsv"], "error: --eval-assembly-contigs needs --eval-assembly"),
    (["--eval-assembly-k", "21", "--genome", "g.fna", "--output", "x.fq"], "error: --eval-assembly-k needs --eval-assembly"),
    (EVAL + ["--eval-assembly-k", "16"], "error: invalid value '16' for '--eval-assembly-k': k is odd"),
    (EVAL + ["--eval-assembly-k", "13"], "error: invalid value for --eval-assembly-k"),
    (EVAL + ["--eval-assembly-k", "33"], "error: invalid value for --eval-assembly-k"),
    (["--eval-assembly"], "error: a value is required for '--eval-assembly'"),
    (["--eval-assembly-report="], "error: a file name is required for '--eval-assembly-report'"),
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
    flags = ["--eval-classified-taxa <FILE>", "--eval-assembly <FILE>", "--eval-assembly-truth <FILE>", "--eval-assembly-report <FILE>",
             "--eval-assembly-contigs <FILE>", "--eval-assembly-k <K>", "--stats <FILE>"]
    at = [text.index("            " + f) for f in flags]
    assert at == sorted(at) and "no simulation" in text[at[1]:at[2]] and "--gold-assembly" in text[at[2]:at[3]] and "N50" in text[at[3]:at[4]]


# ---- host.cpp's routines under the sanitizers --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("asmeval") / "asmeval_report_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "asmeval_report_main.cpp"), str(HOST / "host.cpp")])
    return exe


def ask(exe, block: bytes) -> bytes:
    r = subprocess.run([str(exe)], input=block, capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    assert r.stdout.endswith(b"--\n")
    return r.stdout[:-3]


def test_report_formatter(report_main):
    rng = np.random.default_rng(11)
    names = ["gA", "gB", "z|9"]
    for case in range(5):
        counts = {n: int(v) for n, v in zip(_asmeval.COUNTS, rng.integers(0, 2 ** 40, 18))}
        counts["novel"] = 0 if case == 1 else counts["novel"] % (counts["kmers"] + 1)
        if case == 2:
            counts["kmers"] = counts["novel"] = 0
        by = rng.integers(0, 2 ** 40, (4, 5)).astype(np.uint64)
        if case == 3:
            by[:, 0] = 0
        tl = [] if case == 4 else [int(x) for x in rng.integers(0, 5000, 7)]
        cl = [0, 0] if case == 4 else [int(x) for x in rng.integers(1, 90000, 12)]
        block = "report %d 3 %d %d\n%s\n%s\n%s\n%s\n%s\n" % (21, len(tl), len(cl), " ".join(names), " ".join(str(counts[n]) for n in _asmeval.COUNTS),
                                                       " ".join(str(int(x)) for x in by.reshape(-1)), " ".join(map(str, tl)), " ".join(map(str, cl)))
        assert ask(report_main, block.encode()).decode() == _asmeval.report_text(counts, by, names, 21, tl, cl), case
    text = _asmeval.report_text(dict.fromkeys(_asmeval.COUNTS, 0) | {"kmers": 1000, "novel": 10}, np.array([[4, 2, 0, 0, 0], [0, 0, 0, 0, 0]], dtype=np.uint64),
                                ["g"], 21, [10, 30, 20, 40], [5])
    assert "#completeness\t2/4\t0.500000\n" in text and "#truth_contiguity\t4\t100\t40\t30\n" in text and "G\tshared\t0\t0\t0\t0\t0\tNA\n" in text
    assert "#qv\t33.20" in text   # 1 - 0.99^(1/21) = 4.7847e-4, and -10 log10 of that is 33.201


def test_contig_rows_fasta_records_and_contiguity(report_main):
    cols = (np.array([40, 0, 2 ** 33], dtype=np.uint64), np.array([26, 0, 7], dtype=np.uint32), np.array([12, 0, 7], dtype=np.uint32),
            np.array([0, 0, 7], dtype=np.uint32), np.array([1, NONE, NONE], dtype=np.uint32), np.array([6, 0, 0], dtype=np.uint32))
    block = "contigs 2 2 3\nc1 c|2\ngA gB\n" + "".join(" ".join(str(int(c[i])) for c in cols) + "\n" for i in range(3))
    want = "c1\t40\t26\t12\t0\t1\t6\tgB\nc|2\t0\t0\t0\t0\t4294967295\t0\t.\n?\t8589934592\t7\t7\t7\t4294967295\t0\t.\n"
    assert ask(report_main, block.encode()).decode() == want == _asmeval.contig_rows(["c1", "c|2"], ["gA", "gB"], cols)
    for text in (b">a b c\nACG\nT\n>b\tx\n\n>c\r\nAC\r\nG\r", b"ACGT\n>x|y z\nAC", b"", b">", b"\n\n>q\n", b">a\n" + b"A" * 5000):
        got = ask(report_main, b"fasta %d\n" % len(text) + text).decode()
        try:
            names, lens = _asmeval.fasta_records(text)
        except _asmeval.Malformed:
            names, lens = _asmeval.fasta_records(text[text.index(b">"):])
        assert got == "".join("%s\t%d\n" % (n, l) for n, l in zip(names, lens)), text[:20]
