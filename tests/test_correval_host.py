"""Scoring a read error corrector's output, without a GPU: the report, the row writer and the ratio of host.cpp in a stand-alone program
under the sanitizers (no LD_PRELOAD anywhere: the program has its own main), against expectations written out by hand and against the
restatement of tests/_correval.py; the command line's usage errors and help rows; the symbols of simmr_correval_*."""
import subprocess
from pathlib import Path

import pytest

from simmr_amd import _abi
from tests import _correval as M

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"
U64 = 2**64 - 1


@pytest.fixture(scope="module")
def report_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("correval") / "correval_report_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "correval_report_main.cpp"), str(HOST / "host.cpp")])
    return exe


def ask(exe, block: bytes) -> str:
    r = subprocess.run([str(exe)], input=block, capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    assert r.stdout.endswith(b"--\n")
    return r.stdout[:-3].decode()


def test_the_ratio_by_hand(report_main):
    for neg, num, den, want in ((0, 1, 3, "0.333333"), (0, 2, 3, "0.666667"), (1, 1, 3, "-0.333333"), (0, 0, 5, "0.000000"), (1, 0, 5, "0.000000"),
                                (0, 5, 0, "NA"), (0, 0, 0, "NA"), (0, 1, 2000000, "0.000001"), (0, 1, 2000001, "0.000000"), (1, 1, 4000000, "0.000000"),
                                (0, U64, U64, "1.000000"), (0, U64, 1, "%d.000000" % U64), (1, U64, 3, "-6148914691236517205.000000"),
                                (0, U64 - 1, U64, "1.000000"), (0, 7, 7, "1.000000"), (0, 9, 4, "2.250000")):
        assert ask(report_main, b"ratio %d %d %d\n" % (neg, num, den)) == want + "\n", (neg, num, den)
        assert M.ratio(-num if neg else num, den) == want


def test_the_report_by_hand(report_main):
    counts = dict(zip(M.COUNTS, range(100, 129)))
    counts.update(kept=900, damaged=30, fixed=60, left=25, miscorrected=5, trimmed_error=10)
    cells = [(0, 0, 500), (0, 31, 400), (0, 124, 3), (0, 1 * 25 + 0 * 5 + 1, 60), (1, 0 * 5, 7), (1, 40 * 5 + 2, 60), (1, 94 * 5 + 4, 5), (2, 0, 450),
             (2, 3 * 5 + 1, 30), (2, 511 * 5 + 3, 25)]
    block = "sparse %d\n%s\n%s\n" % (len(cells), " ".join(str(counts[n]) for n in M.COUNTS), "\n".join("%d %d %d" % c for c in cells))
    want = "".join("#%s\t%d\n" % (n, counts[n]) for n in M.COUNTS)
    want += "#gain\t30/100\t0.300000\n#sensitivity\t60/100\t0.600000\n#specificity\t900/930\t0.967742\n"
    want += "#Q\tquality\tkept\tdamaged\tfixed\tleft\tmiscorrected\nQ\t0\t7\t0\t0\t0\t0\nQ\t40\t0\t0\t60\t0\t0\nQ\t94\t0\t0\t0\t0\t5\n"
    want += "#P\tposition\tkept\tdamaged\tfixed\tleft\tmiscorrected\nP\t0\t450\t0\t0\t0\t0\nP\t3\t0\t30\t0\t0\t0\nP\t511\t0\t0\t0\t25\t0\n"
    want += "#C\ttrue\toriginal\tA\tC\tG\tT\tN\n"
    cube = [[[0] * 5 for _ in range(5)] for _ in range(5)]
    cube[0][0][0], cube[1][1][1], cube[4][4][4], cube[1][0][1] = 500, 400, 3, 60
    want += "".join("C\t%s\t%s\t%s\n" % ("ACGTN"[t], "ACGTN"[o], "\t".join(map(str, cube[t][o]))) for t in range(5) for o in range(5))
    got = ask(report_main, block.encode())
    assert got == want
    assert "C\tC\tA\t0\t60\t0\t0\t0\n" in got and got.count("\n") == 29 + 3 + 1 + 3 + 1 + 3 + 1 + 25
    by_qual = [[0] * 5 for _ in range(95)]
    by_pos = [[0] * 5 for _ in range(512)]
    by_qual[0][0], by_qual[40][2], by_qual[94][4], by_pos[0][0], by_pos[3][1], by_pos[511][3] = 7, 60, 5, 450, 30, 25
    assert M.report(counts, cube, by_qual, by_pos) == want   # the restatement the GPU test of the command line uses


def test_zero_denominators_and_the_largest_counts(report_main):
    zero = ask(report_main, ("sparse 0\n%s\n" % " ".join(["0"] * 29)).encode())
    assert "#gain\t0/0\tNA\n#sensitivity\t0/0\tNA\n#specificity\t0/0\tNA\n#Q\tquality" in zero
    assert zero.endswith("C\tN\tN\t0\t0\t0\t0\t0\n") and "\nQ\t" not in zero and "\nP\t" not in zero
    counts = dict.fromkeys(M.COUNTS, U64)
    full = "report\n%s\n%s\n" % (" ".join([str(U64)] * 29), " ".join([str(U64)] * (125 + 95 * 5 + 512 * 5)))
    got = ask(report_main, full.encode())
    assert "#worse\t%d\n" % U64 in got
    # the sums of the denominators pass 2^64: they stop at 2^64 - 1 (counts of positions never get near it)
    assert "#gain\t0/%d\t0.000000\n#sensitivity\t%d/%d\t1.000000\n#specificity\t%d/%d\t1.000000\n" % (U64, U64, U64, U64, U64) in got
    assert got.count("\nQ\t") == 95 and got.count("\nP\t") == 512 and ("P\t511" + ("\t%d" % U64) * 5 + "\n") in got
    assert counts["worse"] == U64
    damaged_only = dict.fromkeys(M.COUNTS, 0)
    damaged_only.update(damaged=3, left=1, kept=1)
    got = ask(report_main, ("sparse 0\n%s\n" % " ".join(str(damaged_only[n]) for n in M.COUNTS)).encode())
    assert "#gain\t-3/1\t-3.000000\n#sensitivity\t0/1\t0.000000\n#specificity\t1/4\t0.250000\n" in got
    assert M.report(damaged_only, [[[0] * 5] * 5] * 5, [[0] * 5] * 95, [[0] * 5] * 512) == got


def test_the_rows_by_hand(report_main):
    rows = [(6, 100, 2, 0, 1), (7, 100, 2, 1, 3), (9, 50, 0, 0xffffffff, 0), ((10**18 - 1) << 1 | 1, 0xffffffff, 0xffffffff, 0xfffffffe, 0xffffffff), (12, 1, 0, 0, 2)]
    block = "rows %d\n%s\n" % (len(rows), "\n".join("%d %d %d %d %d 0" % r for r in rows))
    want = "3\t1\t100\t2\t1\t3\n4\t1\t50\t0\t.\t0\n999999999999999999\t1\t4294967295\t4294967295\t4294967294\t4294967295\n"
    assert ask(report_main, block.encode()) == want == M.read_rows(rows)
    assert ask(report_main, b"rows 0\n") == ""


EVAL = ["--eval-corrected", "c.fq", "--eval-corrected-truth", "t.sam", "--eval-corrected-report", "r.tsv"]
ONLY = "it takes only --eval-corrected-truth, --eval-corrected-report, --eval-corrected-reads, --eval-corrected-fasta and --device"
USAGE_ERRORS = [
    (EVAL + ["--num-reads", "5"], f"error: --eval-corrected runs no simulation: {ONLY} ('--num-reads' given)"),
    (["--genome", "g.fna"] + EVAL, f"error: --eval-corrected runs no simulation: {ONLY} ('--genome' given)"),
    (EVAL + ["--output", "x.fq"], f"error: --eval-corrected runs no simulation: {ONLY} ('--output' given)"),
    (EVAL + ["--devices", "0,1"], f"error: --eval-corrected runs no simulation: {ONLY} ('--devices' given)"),
    (EVAL + ["--sam", "x.sam"], f"error: --eval-corrected runs no simulation: {ONLY} ('--sam' given)"),
    (EVAL[:4], "error: --eval-corrected needs --eval-corrected-report"),
    (EVAL[:2] + EVAL[4:], "error: --eval-corrected needs --eval-corrected-truth"),
    (EVAL[2:], "error: --eval-corrected-truth needs --eval-corrected"),
    (["--eval-corrected-reads", "x.tsv"], "error: --eval-corrected-reads needs --eval-corrected"),
    (["--eval-corrected-fasta", "--genome", "g.fna", "--output", "x.fq"], "error: --eval-corrected-fasta needs --eval-corrected"),
    (["--eval-corrected"], "error: a value is required for '--eval-corrected'"),
    (["--eval-corrected-report="], "error: a file name is required for '--eval-corrected-report'"),
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
    flags = ["--eval-bins-contigs <FILE>", "--eval-corrected <FILE>", "--eval-corrected-truth <FILE>", "--eval-corrected-report <FILE>",
             "--eval-corrected-reads <FILE>", "--eval-corrected-fasta"]
    at = [text.index("\n            " + f) for f in flags]   # (a row begins its line with twelve blanks)
    assert at == sorted(at) and "no simulation" in text[at[1]:at[2]] and "--sam" in text[at[2]:at[3]]


def test_symbols_declared_and_bound():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    for name in ("create", "destroy", "reset", "truth_add", "truth_plan", "add", "read", "emit"):
        assert f"simmr_correval_{name}(" in header and f"simmr_correval_{name}" in _abi.SYMBOLS
    assert "simmr_last_correval_ms(" in header and "simmr_last_correval_ms" in _abi.SYMBOLS
    assert "#define SIMMR_CORREVAL_POS 512u" in header and _abi.CORREVAL_POS == M.POS == 512 and _abi.CORREVAL_COUNTS == M.COUNTS
    assert _abi.C.sizeof(_abi.CorrevalCounts) == 8 * len(M.COUNTS) and _abi.C.sizeof(_abi.CorrevalConfig) == 8
