"""Scoring an aligner's SAM against the true alignments, without a GPU: the plain restatement of the rules (tests/_mapeval.py) on
hand-written records, the symbols of simmr_mapeval_*, the command line's usage rows and help text, the build facts the new
translation unit must leave as they are, and the report formatter and @SQ reader of host.cpp under the sanitizers."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _mapeval

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "simmr_amd" / "csrc"
HOST = ROOT / "simmr_amd" / "host"
NAMES = ["c0", "c1"]


def line(qname, flag, rname, pos, mapq, cigar):
    return b"\t".join(str(x).encode() for x in (qname, flag, rname, pos, mapq, cigar)) + b"\t*\t0\t0\t*\t*\n"


def classes(truth, aligned, pct=10, names=NAMES):
    """the class of every aligned record's entry, from best[] of a one-record evaluation each"""
    out = []
    for rec in _mapeval.lines(aligned):
        m = _mapeval.evaluate(names, [truth], [rec + b"\n"], pct)
        out.append(int(m.entries()[1].max()) >> 8)
    return out


# ---- the model on hand-written records --------------------------------------------------------------------------------------------
def test_overlap_rule_at_equality_and_one_below():
    truth = line(1, 0, "c0", 101, 255, "110M")  # [100, 210)
    # moved by 90: ov 20, un 200: 100 * 20 == 10 * 200; by 91: ov 19, un 201: 1900 < 2010
    assert classes(truth, line(1, 0, "c0", 191, 60, "110M") + line(1, 0, "c0", 192, 60, "110M")) == [3, 2]
    assert classes(truth, line(1, 0, "c0", 11, 60, "110M") + line(1, 0, "c0", 10, 60, "110M")) == [3, 2]
    assert _mapeval.threshold_shift(110, 10) == 90 and _mapeval.threshold_shift(150, 10) == 122
    # 100 percent: the same interval only; 1 percent: one shared base of at most a hundred
    assert classes(truth, line(1, 0, "c0", 101, 60, "110M") + line(1, 0, "c0", 101, 60, "109M"), pct=100) == [3, 2]
    assert classes(line(1, 0, "c0", 1, 255, "50M"), line(1, 0, "c0", 50, 1, "51M") + line(1, 0, "c0", 50, 1, "52M"), pct=1) == [3, 2]


def test_abutting_intervals_other_strand_other_name():
    truth = line(1, 16, "c0", 101, 255, "50M")
    assert classes(truth, line(1, 16, "c0", 151, 60, "50M") + line(1, 16, "c0", 51, 60, "50M")) == [2, 2]   # ov == 0 on either side
    assert classes(truth, line(1, 16, "c0", 150, 60, "50M"), pct=1) == [3]                                  # one base
    assert classes(truth, line(1, 0, "c0", 101, 60, "50M") + line(1, 16, "c1", 101, 60, "50M") + line(1, 16, "c0", 101, 60, "50M")) == [2, 2, 3]
    m = _mapeval.evaluate(NAMES, [truth], [line(1, 16, "c9", 101, 60, "50M") + line(1, 20, "c0", 101, 3, "50M") + line(1, 16, "*", 0, 0, "*")])
    c, by = m.read()
    assert (c["unknown_ref"], c["wrong"], c["unmapped"], c["multiple"], c["reads_wrong"]) == (1, 1, 2, 1, 1) and by[60, 1] == 1 and by.sum() == 1
    assert m.entries()[1].tolist() == [2 << 8 | 60] and m.entries()[2].tolist() == [3]


def test_clips_and_indels_change_the_span():
    assert _mapeval.cigar_span(b"5H10S20M5I30=2X7D3S") == (59, False) and _mapeval.cigar_span(b"*") == (0, False)
    assert _mapeval.cigar_span(b"10M5N10M") == (20, True) and _mapeval.cigar_span(b"10M2P")[1]
    truth = line(1, 0, "c0", 101, 255, "100M")
    # a 90-base soft clip leaves [100, 110): ov 10 of un 100; an insertion adds nothing; a deletion adds its bases
    assert classes(truth, line(1, 0, "c0", 101, 9, "90S10M") + line(1, 0, "c0", 101, 9, "91S9M")) == [3, 2]
    assert classes(truth, line(1, 0, "c0", 101, 9, "10M900I"), pct=10) == [3]
    assert classes(truth, line(1, 0, "c0", 101, 9, "10M991D"), pct=10) == [2] and classes(truth, line(1, 0, "c0", 101, 9, "10M990D"), pct=10) == [3]
    for bad in (b"10", b"M10M", b"1234567890M", b"", b"10M*"):
        with pytest.raises(_mapeval.Malformed):
            _mapeval.cigar_span(bad)


def test_empty_interval_truth_entry_and_the_filters():
    truth = line(1, 0, "c0", 101, 255, "*") + line(2, 0x900, "c0", 5, 255, "9M") + line(3, 4, "c0", 5, 255, "9M") + line(4, 0, "c0", 5, 255, "4M3N5M") + \
        b"@CO\tx\n\n" + line(5, 0x80, "c1", 7, 255, "9M")
    aligned = line(1, 0, "c0", 101, 60, "*") + line(1, 0, "c0", 101, 60, "50M") + line(2, 0, "c0", 5, 60, "9M") + line(5, 0, "c1", 7, 60, "9M") + \
        line(5, 0x80, "c1", 7, 60, "9M") + line(5, 0x180, "c1", 7, 60, "9M") + line(5, 0x80, "c1", 7, 60, "4M3N5M") + line("read5", 0x80, "c1", 7, 60, "9M")
    m = _mapeval.evaluate(NAMES, [truth], [aligned])
    c, by = m.read()
    assert (c["truth_lines"], c["truth_header"], c["truth_entries"], c["truth_skipped"]) == (6, 1, 2, 3)
    assert (c["records"], c["secondary"], c["cigar_op"], c["unknown_read"], c["wrong"], c["correct"]) == (8, 1, 1, 3, 2, 1)  # nothing overlaps nothing
    assert m.entries()[0].tolist() == [2, 11] and m.entries()[1].tolist() == [2 << 8 | 60, 3 << 8 | 60] and m.entries()[2].tolist() == [2, 1]
    with pytest.raises(_mapeval.DuplicateKey):
        _mapeval.evaluate(NAMES, [line(1, 0, "c0", 5, 255, "9M") + line(1, 16, "c1", 5, 255, "9M")], [])
    for bad in (line("r1", 0, "c0", 5, 255, "9M"), line(1, 0, "c9", 5, 255, "9M"), line(1, 0, "c0", 0, 255, "9M"), line(1, 0, "c0", 5, 256, "9M"),
                line(1, 0, "c0", 2 ** 31, 255, "9M"), b"1\t0\tc0\t5\t255\t9M\t*\t0\t0\t*\n"):
        with pytest.raises(_mapeval.Malformed):
            _mapeval.Model(NAMES).truth_add(bad)


def test_the_perturbation_helper():
    truth = b"@SQ\tSN:c0\tLN:9\n" + b"".join(line(i, 0, "c0", 100 + i, 255, "50M") for i in range(12))
    plan = [("same", None), ("drop", None), ("double", 5), ("unmapped", None)]
    a = _mapeval.derive(truth, plan, seed=1)
    assert a.startswith(b"@SQ\t") and len(_mapeval.lines(a)) == 1 + 3 + 0 + 6 + 3
    c, _ = _mapeval.evaluate(["c0"], [truth], [a]).read()
    assert (c["missing"], c["multiple"], c["reads_unmapped"], c["reads_correct"]) == (3, 3, 3, 6)
    assert _mapeval.sq_names(truth) == [b"c0"]


# ---- the library's surface ---------------------------------------------------------------------------------------------------------
SYMBOLS = ["simmr_mapeval_create", "simmr_mapeval_destroy", "simmr_mapeval_reset", "simmr_mapeval_truth_add", "simmr_mapeval_truth_plan",
           "simmr_mapeval_add", "simmr_mapeval_read", "simmr_mapeval_emit", "simmr_last_mapeval_ms"]


def test_symbols_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in SYMBOLS:
        assert re.search(rf"^(?:int|void) {name}\(", header, re.M), name
        assert name in _abi.SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(_abi.MapevalCounts) == 8 * len(_abi.MAPEVAL_COUNTS) == 8 * 19 and _abi.MAPEVAL_COUNTS == _mapeval.COUNTS
    fields = re.search(r"typedef struct simmr_mapeval_counts \{(.*?)\} simmr_mapeval_counts;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert tuple(re.findall(r"\b([a-z_]+)\s*[,;]", fields)) == _abi.MAPEVAL_COUNTS
    assert C.sizeof(_abi.MapevalConfig) == 16


def test_calls_need_an_object():
    lib = _abi.load()
    h, n, ms = C.c_void_p(), C.c_uint64(), C.c_float()
    cfg = _abi.MapevalConfig(0, 10, None)
    assert lib.simmr_mapeval_create(None, C.byref(h)) == _abi.EINVAL
    assert lib.simmr_mapeval_reset(None, C.byref(cfg)) == _abi.EINVAL
    assert lib.simmr_mapeval_truth_add(None, None, 0) == _abi.EINVAL and lib.simmr_mapeval_add(None, None, 0) == _abi.EINVAL
    assert lib.simmr_mapeval_truth_plan(None, C.byref(n)) == _abi.EINVAL
    assert lib.simmr_mapeval_read(None, C.byref(_abi.MapevalCounts()), None) == _abi.EINVAL
    assert lib.simmr_mapeval_emit(None, None, None, None, 0) == _abi.EINVAL
    assert lib.simmr_last_mapeval_ms(None, C.byref(ms)) == _abi.EINVAL
    lib.simmr_mapeval_destroy(None)


def test_the_unit_is_built_without_a_slot_of_the_engine():
    make = (CSRC / "Makefile").read_text()
    tail = " bam_index.hip bam.hip fit_sam.hip fit.hip overlap.hip sam_sort.hip sam.hip pileup.hip engine.hip depth.hip strain.hip regions.hip\n"
    assert make.count(tail) == 2 and make.count(" mapeval.hip" + tail) == 2
    srcs = re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
    assert {"mapeval.hip", "mapeval_kernels.hip"} <= set(srcs)
    internal = (CSRC / "engine_internal.hpp").read_text()
    assert "ENG_EXT_BAM = 9," in internal and "ENG_EXT_COUNT = 12" in internal
    unit = (CSRC / "mapeval.hip").read_text()
    assert "eng_ext_slot" not in unit and '#include "engine.hip"' not in unit and '#include "kernels.hip"' not in unit
    kernels = (CSRC / "mapeval_kernels.hip").read_text()
    assert "#define FSAM_ROUTINES_ONLY" in kernels and set(re.findall(r"^(k_[a-z0-9_]+)\(", kernels, re.M)) == {
        "k_mev_index", "k_mev_scan", "k_mev_truth", "k_mev_gather", "k_mev_record", "k_mev_reduce"}
    assert "#define SIMMR_ABI_VERSION 1\n" in (ROOT / "include" / "simmr_hip.h").read_text()


# ---- the command line --------------------------------------------------------------------------------------------------------------
EVAL = ["--eval-sam", "a.sam", "--eval-truth", "t.sam", "--eval-report", "r.tsv"]
ONLY = "it takes only --eval-truth, --eval-report, --eval-reads, --eval-min-overlap and --device"
USAGE_ERRORS = [
    (EVAL + ["--num-reads", "5"], f"error: --eval-sam runs no simulation: {ONLY} ('--num-reads' given)"),
    (["--genome", "g.fna"] + EVAL, f"error: --eval-sam runs no simulation: {ONLY} ('--genome' given)"),
    (EVAL + ["--output", "x.fq"], f"error: --eval-sam runs no simulation: {ONLY} ('--output' given)"),
    (EVAL + ["--sam", "x.sam"], f"error: --eval-sam runs no simulation: {ONLY} ('--sam' given)"),
    (EVAL + ["--devices", "0,1"], f"error: --eval-sam runs no simulation: {ONLY} ('--devices' given)"),
    (EVAL + ["--fit-model", "m.bin"], f"error: --eval-sam runs no simulation: {ONLY} ('--fit-model' given)"),
    (EVAL + ["--fit-from-sam", "x.sam", "--fit-model", "m.bin"],
     "error: --fit-from-sam runs no simulation: it takes only --fit-model, --fit-k, --fit-max-alt, --single-reads and --device ('--eval-sam' given)"),
    (EVAL[:4], "error: --eval-sam needs --eval-report"),
    (EVAL[:2] + EVAL[4:], "error: --eval-sam needs --eval-truth"),
    (EVAL[2:], "error: --eval-truth needs --eval-sam"),
    (["--eval-reads", "x.tsv"], "error: --eval-reads needs --eval-sam"),
    (["--eval-min-overlap", "10", "--genome", "g.fna", "--output", "x.fq"], "error: --eval-min-overlap needs --eval-sam"),
    (EVAL + ["--eval-min-overlap", "0"], "error: invalid value for --eval-min-overlap (1 .. 100)"),
    (EVAL + ["--eval-min-overlap", "101"], "error: invalid value for --eval-min-overlap (1 .. 100)"),
    (EVAL + ["--eval-min-overlap"], "error: invalid value for --eval-min-overlap (1 .. 100)"),
    (["--eval-sam"], "error: a value is required for '--eval-sam'"),
    (["--eval-report="], "error: a file name is required for '--eval-report'"),
]


@pytest.mark.parametrize("argv,first", USAGE_ERRORS, ids=[" ".join(a)[-60:] for a, _ in USAGE_ERRORS])
def test_cli_usage_errors(argv, first, tmp_path):
    subprocess.check_call(["make", "-s", "-C", str(HOST), "simmr-hip"])
    r = subprocess.run([str(HOST / "simmr-hip")] + argv, capture_output=True, text=True, cwd=tmp_path)
    assert (r.returncode, r.stderr.split("\n")[0]) == (2, first)
    assert not list(tmp_path.iterdir())  # nothing was written


def test_help_rows_stand_behind_the_last_existing_row():
    subprocess.check_call(["make", "-s", "-C", str(HOST), "simmr-hip"])
    text = subprocess.run([str(HOST / "simmr-hip"), "--help"], capture_output=True, text=True, check=True).stdout
    flags = ["--strain-vcf <FILE>", "--eval-sam <FILE>", "--eval-truth <FILE>", "--eval-report <FILE>", "--eval-reads <FILE>", "--eval-min-overlap <PCT>"]
    at = [text.index("            " + f) for f in flags]
    assert at == sorted(at) and text.endswith("[default: 10]\n")
    assert "paftools mapeval" in text[at[1]:at[2]] and "no simulation" in text[at[1]:at[2]]
    assert not re.search(r"^\s+--[a-z-]+ ", text[at[5]:].split("\n", 1)[1], re.M)  # no row behind the new ones


# ---- host.cpp's formatter and @SQ reader under the sanitizers -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mapeval") / "mapeval_report_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "mapeval_report_main.cpp"), str(HOST / "host.cpp")])
    return exe


def ask(exe, block: bytes) -> bytes:
    r = subprocess.run([str(exe)], input=block, capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    assert r.stdout.endswith(b"--\n")
    return r.stdout[:-3]


def test_report_formatter(report_main):
    rng = np.random.default_rng(2)
    for case in range(4):
        counts = {n: int(v) for n, v in zip(_mapeval.COUNTS, rng.integers(0, 2 ** 40, 19))}
        by = np.zeros((256, 2), dtype=np.uint64)
        if case < 3:
            for q in rng.choice(256, size=(1, 7, 256)[case], replace=False):
                by[q] = rng.integers(0, (5, 10 ** 6, 2 ** 33)[case], 2)
            by[255 if case else 0] = (3, 0)
        rows = [(q, int(by[q, 0]), int(by[q, 1])) for q in range(256) if by[q].sum()]
        block = "report\n" + " ".join(str(counts[n]) for n in _mapeval.COUNTS) + f"\n{len(rows)}\n" + "".join(f"{q} {a} {b}\n" for q, a, b in rows)
        got = ask(report_main, block.encode())
        assert got == _mapeval.report(counts, by), case
        assert got.count(b"\nQ\t") == len(rows)
    # a third: the ratio as %.6g prints it
    by = np.zeros((256, 2), dtype=np.uint64)
    by[60], by[0] = (2, 0), (0, 1)
    got = ask(report_main, ("report\n" + " ".join(["0"] * 19) + "\n2\n60 2 0\n0 0 1\n").encode())
    assert got.endswith(b"Q\t60\t2\t0\t0\t2\nQ\t0\t1\t1\t0.333333\t3\n") and got == _mapeval.report(dict.fromkeys(_mapeval.COUNTS, 0), by)


def test_read_rows(report_main):
    key = np.array([0, 1, 7, 2 ** 63 - 1, 2 ** 63 - 2], dtype=np.uint64)
    best = np.array([0, 1 << 8 | 255, 3 << 8 | 60, 2 << 8, 3 << 8], dtype=np.uint32)
    hits = np.array([0, 1, 2, 2 ** 32 - 1, 1], dtype=np.uint32)
    block = f"reads {len(key)}\n" + "".join(f"{k} {b} {h}\n" for k, b, h in zip(key, best, hits))
    got = ask(report_main, block.encode())
    assert got == _mapeval.reads_file(key, best, hits) == b"0\t0\t0\t0\t0\n0\t1\t1\t255\t1\n4611686018427387903\t1\t2\t0\t4294967295\n"
    assert ask(report_main, b"reads 0\n") == b""


def test_sq_reader(report_main):
    texts = [b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:c0\tLN:5\n@SQ\tLN:7\tSN:g1|c1\tM5:x\n@SQ\tLN:9\n@PG\tID:SN:no\n@SQ\tSN:last\tLN:1",
             b"", b"\n\n", b"@SQ\t", b"@SQ\tSN:", b"@SQ\tSN:\n@SQ", b"@SQ\tSN:a", b"1\t0\tc0\t5\t60\t9M\t*\t0\t0\t*\t*\n@SQ\tSN:behind\n", b"@SQX\tSN:no\n@SQ\tXSN:no\tSN:yes\n"]
    for text in texts:
        got = ask(report_main, b"sq %d\n" % len(text) + text).split(b"\n")
        want = _mapeval.sq_names(text)
        assert got[0] == b"names %d" % len(want) and got[1:1 + len(want)] == want, text
    assert _mapeval.sq_names(texts[0]) == [b"c0", b"g1|c1", b"last"]
