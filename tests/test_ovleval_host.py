"""Scoring an overlapper's PAF against the true overlaps, without a GPU: the plain restatement of the rules (tests/_ovleval.py) on
hand-written records whose verdicts are written out here, the symbols of simmr_ovleval_*, the command line's usage rows and help
text, the build facts of the new translation unit, and the report and pair-row formatters of host.cpp under the sanitizers."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _ovleval
from tests._ovleval import rec

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "simmr_amd" / "csrc"
HOST = ROOT / "simmr_amd" / "host"

# reads 1 and 2 on one strand, the mates 3/1 and 3/2 on opposite strands, read 9 with read 2
TRUTH = rec(1, 1000, 100, 300, "+", 2, 900, 0, 200) + rec("3/1", 500, 0, 500, "-", "3/2", 500, 0, 500) + rec(9, 5000, 4000, 5000, "+", 2, 900, 400, 900)


# ---- the model on hand-written records ----------------------------------------------------------------------------------------------
VERDICTS = [
    (rec(1, 1000, 100, 300, "+", 2, 900, 0, 200), "correct", 0),
    (rec(2, 900, 0, 200, "+", 1, 1000, 100, 300), "correct", 0),          # the pair named in reversed order
    (rec(2, 900, 100, 300, "+", 1, 1000, 0, 110), "wrong_interval", 0),   # ... and one read's comparison alone fails: 10 of 300 on read 1
    (rec(1, 1000, 100, 300, "-", 2, 900, 0, 200), "wrong_strand", 0),
    (rec(1, 1000, 100, 120, "+", 2, 900, 0, 200), "correct", 0),          # 20 of 200 on the query: 100 * 20 == 10 * 200
    (rec(1, 1000, 100, 119, "+", 2, 900, 0, 200), "wrong_interval", 0),   # one base short: 1900 < 2000
    (rec(1, 1000, 100, 300, "+", 2, 900, 180, 200), "correct", 0),        # 20 of the target's 200 exactly, at its far end
    (rec(1, 1000, 300, 400, "+", 2, 900, 0, 200), "wrong_interval", 0),   # abutting: no base shared
    (rec("3/2", 500, 0, 500, "-", "3/1", 500, 0, 500), "correct", 2),     # a /2 name; keys that differ in the mate bit alone
    (rec(3, 500, 0, 500, "-", "3/2", 500, 0, 500), "correct", 2),         # a bare id is mate 0
    (rec(1, 1000, 0, 10, "+", 9, 5000, 0, 10), "no_pair", None),
    (rec(9, 5000, 0, 10, "+", 9, 5000, 0, 10), "self", None),
    (rec(7, 1000, 0, 10, "+", 1, 1000, 0, 10), "unknown_read", None),     # no read of the truth
    (rec("read1", 1000, 0, 10, "+", 1, 1000, 0, 10), "unknown_read", None),
    (rec("7/1", 10, 0, 10, "+", 7, 10, 0, 10), "unknown_read", None),     # unknown is asked before self
]


def test_every_verdict_written_out():
    m = _ovleval.evaluate([TRUTH], [])
    assert m.order == [(2, 4), (4, 18), (6, 7)] and m.reads == {2, 4, 6, 7, 18}
    for ln, want, at in VERDICTS:
        assert m.verdict(ln[:-1]) == (want, at), ln
    m = _ovleval.evaluate([TRUTH], [b"".join(v[0] for v in VERDICTS)])
    c, by = m.read()
    assert c == {"truth_lines": 3, "truth_entries": 3, "truth_reads": 5, "lines": 15, "records": 15, "unknown_read": 3, "self": 1, "no_pair": 1,
                 "wrong_strand": 1, "wrong_interval": 3, "correct": 6, "wrong": 8, "pairs_found": 2, "pairs_wrong": 0, "pairs_missed": 1, "pairs_multiple": 2}
    ka, kb, ov, best, hits = m.pairs()
    assert ka.tolist() == [2, 4, 6] and kb.tolist() == [4, 18, 7] and ov.tolist() == [200, 1000, 500]
    assert best.tolist() == [3, 0, 3] and hits.tolist() == [8, 0, 2]
    assert by[8].tolist() == [1, 0] and by[9].tolist() == [1, 0] and by[10].tolist() == [0, 1] and by.sum() == 3   # 200, 500 and 1000 bases


def test_the_percent_criterion_and_wrong_beats_nothing():
    m = _ovleval.evaluate([TRUTH], [VERDICTS[3][0]], 10)
    assert m.pairs()[3].tolist() == [2, 0, 0] and m.read()[0]["pairs_wrong"] == 1 and m.read()[1][8].tolist() == [0, 1]
    whole = rec(1, 1000, 100, 300, "+", 2, 900, 0, 200)
    for pct, cand, want in ((100, whole, "correct"), (100, rec(1, 1000, 100, 299, "+", 2, 900, 0, 200), "wrong_interval"),
                            (1, rec(1, 1000, 100, 102, "+", 2, 900, 0, 2), "correct"), (1, rec(1, 1000, 100, 101, "+", 2, 900, 0, 2), "wrong_interval"),
                            (50, rec(1, 1000, 200, 400, "+", 2, 900, 0, 200), "wrong_interval"), (50, rec(1, 1000, 167, 367, "+", 2, 900, 0, 200), "wrong_interval"),
                            (50, rec(1, 1000, 100, 200, "+", 2, 900, 100, 200), "correct")):
        assert _ovleval.evaluate([TRUTH], [], pct).verdict(cand[:-1])[0] == want, (pct, cand)
    assert _ovleval.shrink_below((0, 200), 10) == (0, 19) and _ovleval.shrink_below((5, 14), 10) is None


def test_names_lines_and_what_is_malformed():
    assert _ovleval.name_key(b"0") == 0 and _ovleval.name_key(b"12/1") == 24 and _ovleval.name_key(b"12/2") == 25
    assert _ovleval.name_key(b"9" * 18) == (10 ** 18 - 1) << 1
    for bad in (b"", b"9" * 19, b"12/3", b"12/", b"/1", b"a1", b"1 ", b"-1", b"12/1/1"):
        assert _ovleval.name_key(bad) is None, bad
    assert _ovleval.key_name(24) == "12" and _ovleval.key_name(25) == "12/2"
    assert _ovleval.lines(b"\na\n\nb") == [b"a", b"b"] and _ovleval.lines(b"") == []
    ok = rec(1, 10, 0, 10, "+", 2, 10, 0, 10)
    assert _ovleval.parse(ok[:-1] + b"\ttp:A:S") == (b"1", b"2", False, (0, 10), (0, 10))
    assert _ovleval.parse(rec(1, 2 ** 40 - 1, 0, 0, "-", 2, 10, 10, 10)[:-1])[2] is True
    for bad in (ok[:-5], rec(1, "x", 0, 10, "+", 2, 10, 0, 10), rec(1, 10, 0, 10, "", 2, 10, 0, 10), rec(1, 10, 0, 10, "++", 2, 10, 0, 10),
                rec(1, 10, 11, 10, "+", 2, 10, 0, 10), rec(1, 10, 0, 11, "+", 2, 10, 0, 10), rec(1, 2 ** 40, 0, 1, "+", 2, 10, 0, 10),
                rec(1, 10, 0, 10, "+", 2, 10, 0, 10, tail=(0, 0, "")), rec(1, 10, 0, 10, "+", 2, 10, 0, 10, tail=(0, "1" * 19, 0)), ok[:-1] + b"\r\n"):
        with pytest.raises(_ovleval.Malformed):
            _ovleval.parse(bad[:-1])
    for bad in (rec("r", 10, 0, 10, "+", 2, 10, 0, 10), rec("4/1", 10, 0, 10, "+", 4, 10, 0, 10)):   # on the truth's side only
        with pytest.raises(_ovleval.Malformed):
            _ovleval.evaluate([bad], [])
        assert _ovleval.evaluate([TRUTH], [bad]).read()[0]["records"] == 1
    with pytest.raises(_ovleval.DuplicatePair):
        _ovleval.evaluate([TRUTH + rec(2, 900, 0, 1, "-", 1, 1000, 0, 1)], [])
    with pytest.raises(_ovleval.Malformed):
        _ovleval.evaluate([TRUTH], [ok[:-5] + b"\n"]).read()


def test_the_perturbation_helper():
    truth = b"".join(rec(i, 5000, 1000, 2000 + i, "+", i + 1, 5000, 0, 1000 + i) for i in range(1, 1 + 13 * 11 * 7))
    cand = _ovleval.derive(truth, outside_id=10 ** 9)
    c, by = _ovleval.evaluate([truth], [cand]).read()
    n = 13 * 11 * 7
    assert c["truth_entries"] == n and c["pairs_missed"] >= n // 3 and c["pairs_multiple"] > 0 and c["unknown_read"] > 0
    assert c["wrong_strand"] > 0 and c["wrong_interval"] > 0 and c["correct"] > c["pairs_found"] > 0 and c["self"] == 0


# ---- the library's surface ---------------------------------------------------------------------------------------------------------
SYMBOLS = ["simmr_ovleval_create", "simmr_ovleval_destroy", "simmr_ovleval_reset", "simmr_ovleval_truth_add", "simmr_ovleval_truth_plan",
           "simmr_ovleval_add", "simmr_ovleval_read", "simmr_ovleval_emit", "simmr_last_ovleval_ms"]


def test_symbols_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in SYMBOLS:
        assert re.search(rf"^(?:int|void) {name}\(", header, re.M), name
        assert name in _abi.SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(_abi.OvlevalCounts) == 8 * len(_abi.OVLEVAL_COUNTS) == 8 * 16 and _abi.OVLEVAL_COUNTS == _ovleval.COUNTS
    fields = re.search(r"typedef struct simmr_ovleval_counts \{(.*?)\} simmr_ovleval_counts;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert tuple(re.findall(r"\b([a-z_]+)\s*[,;]", fields)) == _abi.OVLEVAL_COUNTS
    assert int(re.search(r"#define SIMMR_OVLEVAL_LEN_ROWS (\d+)u", header).group(1)) == _abi.OVLEVAL_LEN_ROWS == _ovleval.LEN_ROWS == 41
    assert "#define SIMMR_ABI_VERSION 1\n" in header


def test_calls_need_an_object():
    lib = _abi.load()
    h, n, ms = C.c_void_p(), C.c_uint64(), C.c_float()
    assert lib.simmr_ovleval_create(None, C.byref(h)) == _abi.EINVAL
    assert lib.simmr_ovleval_reset(None, 10) == _abi.EINVAL
    assert lib.simmr_ovleval_truth_add(None, None, 0) == _abi.EINVAL and lib.simmr_ovleval_add(None, None, 0) == _abi.EINVAL
    assert lib.simmr_ovleval_truth_plan(None, C.byref(n), C.byref(n)) == _abi.EINVAL
    assert lib.simmr_ovleval_read(None, C.byref(_abi.OvlevalCounts()), None) == _abi.EINVAL
    assert lib.simmr_ovleval_emit(None, None, None, None, None, None, 0) == _abi.EINVAL
    assert lib.simmr_last_ovleval_ms(None, C.byref(ms)) == _abi.EINVAL
    lib.simmr_ovleval_destroy(None)


def test_the_unit_is_built_without_a_slot_of_the_engine():
    make = (CSRC / "Makefile").read_text()
    tail = " mapeval.hip bam_index.hip bam.hip fit_sam.hip fit.hip overlap.hip sam_sort.hip sam.hip pileup.hip engine.hip depth.hip strain.hip regions.hip\n"
    assert make.count(tail) == 2 and make.count(" ovleval.hip" + tail) == 2
    srcs = re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
    assert {"ovleval.hip", "ovleval_kernels.hip"} <= set(srcs)
    assert "ENG_EXT_COUNT = 12" in (CSRC / "engine_internal.hpp").read_text()
    unit = (CSRC / "ovleval.hip").read_text()
    assert "eng_ext_slot" not in unit and "unit_state" not in unit and '#include "engine.hip"' not in unit and '#include "kernels.hip"' not in unit
    assert '#include "host_support.hpp"' in unit and "Spans<" in unit
    for text in (unit, (CSRC / "ovleval_kernels.hip").read_text()):
        assert not re.search(r"\bhipFree\(|\bhipEventDestroy\(|\bhipEventElapsedTime\(|#\s*define\s+\w*_TRY\b", text)
    kernels = (CSRC / "ovleval_kernels.hip").read_text()
    assert set(re.findall(r"^(k_[a-z0-9_]+)\(", kernels, re.M)) == {
        "k_ove_index", "k_ove_scan", "k_ove_truth", "k_ove_heads", "k_ove_keys", "k_ove_gather", "k_ove_record", "k_ove_reduce"}
    assert "oracle" not in unit.lower() and "oracle" not in kernels.lower()


# ---- the command line --------------------------------------------------------------------------------------------------------------
EVAL = ["--eval-overlaps", "c.paf", "--eval-overlaps-truth", "t.paf", "--eval-overlaps-report", "r.tsv"]
ONLY = "it takes only --eval-overlaps-truth, --eval-overlaps-report, --eval-overlaps-pairs, --eval-overlaps-min-pct and --device"
USAGE_ERRORS = [
    (EVAL + ["--num-reads", "5"], f"error: --eval-overlaps runs no simulation: {ONLY} ('--num-reads' given)"),
    (["--genome", "g.fna"] + EVAL, f"error: --eval-overlaps runs no simulation: {ONLY} ('--genome' given)"),
    (EVAL + ["--output", "x.fq"], f"error: --eval-overlaps runs no simulation: {ONLY} ('--output' given)"),
    (EVAL + ["--overlaps", "x.paf"], f"error: --eval-overlaps runs no simulation: {ONLY} ('--overlaps' given)"),
    (EVAL + ["--devices", "0,1"], f"error: --eval-overlaps runs no simulation: {ONLY} ('--devices' given)"),
    (EVAL + ["--fit-from-sam", "x.sam", "--fit-model", "m.bin"],
     "error: --fit-from-sam runs no simulation: it takes only --fit-model, --fit-k, --fit-max-alt, --single-reads and --device ('--eval-overlaps' given)"),
    (EVAL + ["--eval-sam", "a.sam", "--eval-truth", "t.sam", "--eval-report", "r2.tsv"],
     "error: --eval-sam runs no simulation: it takes only --eval-truth, --eval-report, --eval-reads, --eval-min-overlap and --device ('--eval-overlaps' given)"),
    (EVAL[:4], "error: --eval-overlaps needs --eval-overlaps-report"),
    (EVAL[:2] + EVAL[4:], "error: --eval-overlaps needs --eval-overlaps-truth"),
    (EVAL[2:], "error: --eval-overlaps-truth needs --eval-overlaps"),
    (["--eval-overlaps-pairs", "x.tsv"], "error: --eval-overlaps-pairs needs --eval-overlaps"),
    (["--eval-overlaps-min-pct", "10", "--genome", "g.fna", "--output", "x.fq"], "error: --eval-overlaps-min-pct needs --eval-overlaps"),
    (EVAL + ["--eval-overlaps-min-pct", "0"], "error: invalid value for --eval-overlaps-min-pct (1 .. 100)"),
    (EVAL + ["--eval-overlaps-min-pct", "101"], "error: invalid value for --eval-overlaps-min-pct (1 .. 100)"),
    (EVAL + ["--eval-overlaps-min-pct"], "error: invalid value for --eval-overlaps-min-pct (1 .. 100)"),
    (["--eval-overlaps"], "error: a value is required for '--eval-overlaps'"),
    (["--eval-overlaps-report="], "error: a file name is required for '--eval-overlaps-report'"),
]


@pytest.mark.parametrize("argv,first", USAGE_ERRORS, ids=[" ".join(a)[-60:] for a, _ in USAGE_ERRORS])
def test_cli_usage_errors(argv, first, tmp_path):
    subprocess.check_call(["make", "-s", "-C", str(HOST), "simmr-hip"])
    r = subprocess.run([str(HOST / "simmr-hip")] + argv, capture_output=True, text=True, cwd=tmp_path)
    assert (r.returncode, r.stderr.split("\n")[0]) == (2, first)
    assert not list(tmp_path.iterdir())  # nothing was written


def test_help_rows_stand_behind_the_overlaps_rows():
    subprocess.check_call(["make", "-s", "-C", str(HOST), "simmr-hip"])
    text = subprocess.run([str(HOST / "simmr-hip"), "--help"], capture_output=True, text=True, check=True).stdout
    flags = ["--overlaps <FILE>", "--min-overlap <N>", "--eval-overlaps <FILE>", "--eval-overlaps-truth <FILE>", "--eval-overlaps-report <FILE>",
             "--eval-overlaps-pairs <FILE>", "--eval-overlaps-min-pct <PCT>", "--stats <FILE>"]
    at = [text.index("            " + f) for f in flags]
    assert at == sorted(at) and text.endswith("[default: 10]\n")
    assert text[at[1]:at[2]].count("\n") == 1   # directly behind the --min-overlap row
    assert "no simulation" in text[at[2]:at[3]] and "ava-ont" in text[at[2]:at[3]]
    last = text.index("            --eval-min-overlap <PCT>")
    assert last > at[-1] and not re.search(r"^\s+--[a-z-]+ ", text[last:].split("\n", 1)[1], re.M)  # nothing behind the last existing row


# ---- host.cpp's formatters under the sanitizers ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ovleval") / "ovleval_report_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "ovleval_report_main.cpp"), str(HOST / "host.cpp")])
    return exe


def ask(exe, block: bytes) -> bytes:
    r = subprocess.run([str(exe)], input=block, capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    assert r.stdout.endswith(b"--\n")
    return r.stdout[:-3]


def test_report_formatter(report_main):
    rng = np.random.default_rng(3)
    for case in range(4):
        counts = {n: int(v) for n, v in zip(_ovleval.COUNTS, rng.integers(0, 2 ** 40, 16))}
        by = np.zeros((41, 2), dtype=np.uint64)
        if case < 3:
            for b in rng.choice(41, size=(1, 7, 41)[case], replace=False):
                by[b] = rng.integers(0, (5, 10 ** 6, 2 ** 33)[case], 2)
            by[40 if case else 0] = (3, 0)
        rows = [(b, int(by[b, 0]), int(by[b, 1])) for b in range(41) if by[b].sum()]
        block = "report\n" + " ".join(str(counts[n]) for n in _ovleval.COUNTS) + f"\n{len(rows)}\n" + "".join(f"{b} {x} {y}\n" for b, x, y in rows)
        got = ask(report_main, block.encode())
        assert got == _ovleval.report(counts, by), case
        assert got.count(b"\nL\t") == len(rows)
    zero = dict.fromkeys(_ovleval.COUNTS, 0)
    by = np.zeros((41, 2), dtype=np.uint64)
    got = ask(report_main, ("report\n" + " ".join(["0"] * 16) + "\n0\n").encode())
    assert got == _ovleval.report(zero, by) and got.endswith(b"#sensitivity\t0\n#precision\t0\n")
    # everything found and correct; a third found, two of three records correct
    c = dict(zero, truth_entries=7, pairs_found=7, correct=9)
    block = "report\n" + " ".join(str(c[n]) for n in _ovleval.COUNTS) + "\n0\n"
    assert ask(report_main, block.encode()).endswith(b"#sensitivity\t1.000000\n#precision\t1.000000\n")
    c = dict(zero, truth_entries=3, pairs_found=1, correct=2, wrong=1)
    by[12] = (1, 2)
    block = "report\n" + " ".join(str(c[n]) for n in _ovleval.COUNTS) + "\n1\n12 1 2\n"
    got = ask(report_main, block.encode())
    assert got.endswith(b"#sensitivity\t0.333333\n#precision\t0.666667\nL\t12\t1\t2\n") and got == _ovleval.report(c, by)


def test_pair_rows(report_main):
    ka = np.array([0, 1, 24, 2 ** 61 - 2], dtype=np.uint64)
    kb = np.array([1, 7, 25, 2 ** 61 - 1], dtype=np.uint64)
    ov = np.array([0, 1, 2 ** 40 - 1, 500], dtype=np.uint64)
    best = np.array([0, 2, 3, 3], dtype=np.uint32)
    hits = np.array([0, 1, 2 ** 32 - 1, 2], dtype=np.uint32)
    block = f"pairs {len(ka)}\n" + "".join(f"{a} {b} {o} {x} {h}\n" for a, b, o, x, h in zip(ka, kb, ov, best, hits))
    got = ask(report_main, block.encode())
    assert got == _ovleval.pair_rows(ka, kb, ov, best, hits)
    assert got.split(b"\n")[:3] == [b"0\t0/2\t0\t0\t0", b"0/2\t3/2\t1\t2\t1", b"12\t12/2\t1099511627775\t3\t4294967295"]
    assert ask(report_main, b"pairs 0\n") == b""
