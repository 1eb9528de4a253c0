"""Scoring a variant caller's VCF against the strain's sites, without a GPU: the plain restatement of the rules
(tests/_vcfeval.py) on hand-written records whose counts are written out here, one case per rule and per QUAL form; the symbols of
simmr_vcfeval_*; the command line's usage rows; the build facts of the new translation unit; and the report, site-row and
##contig routines of host.cpp in a stand-alone program under the sanitizers."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _vcfeval
from tests._vcfeval import rec, site
from tests._scaffold import sorts_through_the_pair_sort

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "simmr_amd" / "csrc"
HOST = ROOT / "simmr_amd" / "host"

NAMES = ["chr2", "chr1"]   # (sorted by the library: chr1 is row 0)
# chr1:100 A>T seen by 7 reads, chr1:102 G>A by one, chr1:200 c>t (lower case) by 300, chr2:5 T>C without an AD item
TRUTH = (b"##fileformat=VCFv4.2\n##contig=<ID=chr1,length=1000>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
         + site("chr1", 100, "A", "T", 5, 7) + site("chr1", 102, "G", "A", 0, 1) + site("chr1", 200, "c", "t", 9, 300) + rec("chr2", 5, "T", "C", info="DP=3"))


def outcome(cand: bytes, **kw):
    """the non-zero counts of the candidate side behind lines / header / records, and the model"""
    m = _vcfeval.evaluate([TRUTH], [cand], NAMES, **kw)
    c = m.read()[0]
    assert c["calls"] == c["correct"] + c["wrong"] and c["wrong"] == c["unknown_contig"] + c["no_site"] + c["ref_mismatch"] + c["wrong_allele"]
    return {k: v for k, v in c.items() if v and k in _vcfeval.COUNTS[6:20]}, m


def test_the_truth_written_out():
    m = _vcfeval.evaluate([TRUTH], [], NAMES)
    c, by_qual, by_ad = m.read()
    assert (c["truth_lines"], c["truth_header"], c["truth_entries"], c["sites_missed"], c["sites_found"]) == (7, 3, 4, 4, 0)
    key, alleles, ad, best, hits = m.sites()
    assert key.tolist() == [99, 101, 199, 1 << 40 | 4] and alleles.tolist() == [0 << 2 | 3, 2 << 2 | 0, 1 << 2 | 3, 3 << 2 | 1] and ad.tolist() == [7, 1, 300, 0]
    assert best.tolist() == hits.tolist() == [0] * 4 and by_qual.sum() == 0
    assert by_ad[3].tolist() == [0, 1] and by_ad[1].tolist() == [0, 1] and by_ad[9].tolist() == [0, 1] and by_ad[0].tolist() == [0, 1] and by_ad.sum() == 4


QUAL_ROWS = [(".", 0), ("0", 0), ("30", 30), ("225.417", 225), ("254.9", 254), ("255", 255), ("1e3", 255), ("2.5e1", 25), ("5.02e-14", 0), ("12345.6", 255),
             ("25.", 25), ("0.999e3", 255), ("0.0254e4", 254), ("2559e-1", 255), ("2549e-1", 254), ("9e-1", 0), ("1E+2", 100), ("0e999", 0), ("1e999", 255),
             ("000000000000000255", 255), ("123456789012345678e-16", 12)]


@pytest.mark.parametrize("text,row", QUAL_ROWS)
def test_each_qual_form(text, row):
    assert _vcfeval.qual_row(text.encode()) == (row, text == ".")
    got, m = outcome(rec("chr1", 100, "A", "T", qual=text))
    assert got == dict(calls=1, correct=1, **({"qual_missing": 1} if text == "." else {}))
    c, by_qual, by_ad = m.read()
    assert by_qual[row].tolist() == [1, 0] and by_qual.sum() == 1 and m.sites()[3][0] == 3 << 8 | row
    assert (c["sites_found"], c["sites_missed"]) == (1, 3) and by_ad[3].tolist() == [1, 0]


@pytest.mark.parametrize("text", ["", "-1", "+5", ".5", "1e", "1e+", "1e1000", "1.2.3", "1,5", "nan", "inf", "1 ", "1234567890123456789", "1e5x", ".."])
def test_a_qual_that_is_no_number(text):
    with pytest.raises(_vcfeval.Malformed):
        _vcfeval.qual_row(text.encode())
    with pytest.raises(_vcfeval.Malformed):
        _vcfeval.evaluate([TRUTH], [rec("chr1", 100, "A", "T", qual=text)], NAMES).read()


GT_FORMS = [   # the record chr1:100 A>T,C with a sample column
    ("0/0", dict(ref_call=1)), ("./.", dict(ref_call=1)), (".", dict(ref_call=1)), ("0", dict(ref_call=1)),
    ("0/1", dict(calls=1, correct=1)),
    ("1|2", dict(calls=2, correct=1, wrong=1, wrong_allele=1)),
    ("2", dict(calls=1, wrong=1, wrong_allele=1)),
    ("2/2/1", dict(calls=2, correct=1, wrong=1, wrong_allele=1)),
    (None, dict(calls=2, correct=1, wrong=1, wrong_allele=1)),          # no FORMAT: every allele
]


@pytest.mark.parametrize("gt,want", GT_FORMS, ids=[str(g[0]) for g in GT_FORMS])
def test_each_gt_form(gt, want):
    cand = rec("chr1", 100, "A", "T,C", qual=40) if gt is None else rec("chr1", 100, "A", "T,C", qual=40, fmt="GT:DP", sample=gt + ":12")
    got, m = outcome(cand)
    assert got == want
    if "calls" in want:
        assert m.sites()[4][0] == want["calls"] and m.sites()[3][0] == (3 if want.get("correct") else 2) << 8 | 40
    # a FORMAT that does not begin with GT, and a FORMAT without a sample column: every allele
    for other in (rec("chr1", 100, "A", "T,C", fmt="DP:GT", sample="12:0/0"), rec("chr1", 100, "A", "T,C", fmt="GT"), rec("chr1", 100, "A", "T,C", fmt="GTX", sample="0/0")):
        assert outcome(other)[0] == dict(calls=2, correct=1, wrong=1, wrong_allele=1, qual_missing=1)
    assert outcome(rec("chr1", 100, "A", "T,C", fmt="GT", sample="0/0"))[0] == dict(ref_call=1, qual_missing=1)


RULES = [
    ("an allele that is REF, and <*>", rec("chr1", 100, "A", "A,<*>", qual=9), dict(ref_call_allele=1, symbolic=1)),
    ("the overlapping-deletion star", rec("chr1", 100, "A", "*", qual=9), dict(symbolic=1)),
    ("a breakend", rec("chr1", 100, "A", "A]chr2:5]", qual=9), dict(symbolic=1)),
    ("an MNP of three with two changed bases", rec("chr1", 100, "ACG", "TCA", qual=9), dict(calls=2, correct=2)),
    ("an MNP that changes an N", rec("chr1", 100, "ANG", "TCA", qual=9), dict(calls=2, correct=2)),
    ("an allele that differs in N alone", rec("chr1", 100, "AN", "AC", qual=9), dict()),
    ("an insertion", rec("chr1", 100, "A", "AT", qual=9), dict(indel=1)),
    ("a deletion", rec("chr1", 100, "AC", "A", qual=9), dict(indel=1)),
    ("a byte that is no base", rec("chr1", 100, "A", "R", qual=9), dict(indel=1)),
    ("an empty allele of the list", rec("chr1", 100, "A", "T,", qual=9), dict(calls=1, correct=1, indel=1)),
    ("lower-case bases", rec("chr1", 200, "C", "t", qual=9) + rec("chr1", 100, "a", "t", qual=9), dict(calls=2, correct=2)),
    ("filtered", rec("chr1", 100, "A", "T", qual=9, filt="q10"), dict(filtered=1)),
    ("PASS", rec("chr1", 100, "A", "T", qual=9, filt="PASS"), dict(calls=1, correct=1)),
    ("an unknown contig", rec("chr9", 100, "A", "T", qual=9), dict(calls=1, wrong=1, unknown_contig=1)),
    ("a position without a site", rec("chr1", 101, "C", "T", qual=9) + rec("chr2", 100, "A", "T", qual=9), dict(calls=2, wrong=2, no_site=2)),
    ("another reference base", rec("chr1", 100, "C", "T", qual=9), dict(calls=1, wrong=1, ref_mismatch=1)),
    ("another allele", rec("chr1", 100, "A", "G", qual=9), dict(calls=1, wrong=1, wrong_allele=1)),
    ("65 bases", rec("chr1", 100, "A" * 65, "T" * 65, qual=9), dict(long_allele=1)),
    ("the last position and one behind it", rec("chr2", 2 ** 40, "AC", "TG", qual=9), dict(calls=2, wrong=2, no_site=2)),
]


@pytest.mark.parametrize("what,cand,want", RULES, ids=[r[0] for r in RULES])
def test_each_rule(what, cand, want):
    assert outcome(cand)[0] == want


def test_filtered_records_on_request_and_the_best_call():
    cand = rec("chr1", 100, "A", "G", qual=90, filt="q10;dp") + rec("chr1", 100, "A", "T", qual=20) + rec("chr1", 100, "A", "T", qual=3)
    got, m = outcome(cand)
    assert got == dict(filtered=1, calls=2, correct=2) and m.sites()[3][0] == 3 << 8 | 20 and m.sites()[4][0] == 2
    got, m = outcome(cand, use_filtered=True)
    assert got == dict(calls=3, correct=2, wrong=1, wrong_allele=1) and m.sites()[3][0] == 3 << 8 | 20 and m.sites()[4][0] == 3   # class before QUAL
    c = m.read()[0]
    assert (c["sites_found"], c["sites_wrong"], c["sites_missed"], c["sites_multiple"]) == (1, 0, 3, 1)
    got, m = outcome(rec("chr1", 102, "G", "C", qual=77))
    assert m.read()[0]["sites_wrong"] == 1 and m.sites()[3][1] == 2 << 8 | 77 and m.read()[2][1].tolist() == [0, 1]


MALFORMED = {
    "seven fields": b"chr1\t100\t.\tA\tT\t9\t.\n",
    "a POS that is no number": rec("chr1", "1e2", "A", "T"),
    "a POS of 0": rec("chr1", 0, "A", "T"),
    "a POS above 2^40": rec("chr1", 2 ** 40 + 1, "A", "T"),
    "nineteen digits": rec("chr1", "0" * 18 + "5", "A", "T"),
    "an empty REF": rec("chr1", 100, "", "T"),
    "a REF with another byte": rec("chr1", 100, "AXG", "T"),
    "an empty ALT": rec("chr1", 100, "A", ""),
    "a QUAL that is no number": rec("chr1", 100, "A", "T", qual="high"),
}
CANDIDATE_ONLY = {
    "a GT index above the alleles": rec("chr1", 100, "A", "T,C", fmt="GT", sample="1/3"),
    "a GT item that is no number": rec("chr1", 100, "A", "T", fmt="GT", sample="1/x"),
    "an empty GT": rec("chr1", 100, "A", "T", fmt="GT", sample=":5"),
}
TRUTH_ONLY = {
    "two bases": rec("chr1", 300, "AC", "TG"),
    "an N": rec("chr1", 300, "N", "T"),
    "REF equal to ALT": rec("chr1", 300, "a", "A"),
    "two alleles": rec("chr1", 300, "A", "T,C"),
    "a contig outside the names": rec("chr3", 300, "A", "T"),
    "AD with one number": rec("chr1", 300, "A", "T", info="DP=1;AD=5"),
    "AD with three": rec("chr1", 300, "A", "T", info="AD=1,2,3;DP=1"),
    "AD with eleven digits": rec("chr1", 300, "A", "T", info="AD=1,12345678901"),
    "AD of 2^32": rec("chr1", 300, "A", "T", info="AD=1,4294967296"),
    "AD without its first number": rec("chr1", 300, "A", "T", info="AD=,4"),
}


def test_what_is_malformed_and_where():
    for what, bad in {**MALFORMED, **CANDIDATE_ONLY}.items():
        with pytest.raises(_vcfeval.Malformed):
            _vcfeval.evaluate([TRUTH], [bad], NAMES).read()
    for what, bad in {**MALFORMED, **TRUTH_ONLY}.items():
        with pytest.raises(_vcfeval.Malformed):
            _vcfeval.evaluate([TRUTH + bad], [], NAMES)
    for what, ok in TRUTH_ONLY.items():   # ... and a candidate may hold them
        assert _vcfeval.evaluate([TRUTH], [ok], NAMES).read()[0]["records"] == 1, what
    for what, ok in CANDIDATE_ONLY.items():   # the sample columns are not read on the truth's side, nor behind a filter
        line = ok.replace(b"\t100\t", b"\t300\t").replace(b"T,C", b"T")
        assert _vcfeval.evaluate([TRUTH + line], [], NAMES).read()[0]["truth_entries"] == 5, what
        assert _vcfeval.evaluate([TRUTH], [ok.replace(b"\t.\t.\t.\t", b"\t.\tlow\t.\t")], NAMES).read()[0]["filtered"] == 1, what
    assert _vcfeval.evaluate([TRUTH + rec("chr1", 2 ** 40, "A", "T", info="XAD=1;AD=4,4294967295;AD=x")], [], NAMES).sites()[2].tolist() == [7, 1, 300, 2 ** 32 - 1, 0]
    with pytest.raises(_vcfeval.DuplicateKey):
        _vcfeval.evaluate([TRUTH + rec("chr1", 102, "G", "C")], [], NAMES)
    assert _vcfeval.lines(b"\na\n\nb") == [b"a", b"b"] and _vcfeval.contig_names(TRUTH) == [b"chr1"]


def test_the_perturbation_helper():
    truth = b"".join(site("chr1", 10 + 3 * i, "ACGT"[i % 4], "CGTA"[i % 4], 5, i) for i in range(210))
    c, by_qual, by_ad = _vcfeval.evaluate([truth], [_vcfeval.derive(truth, b"chrX")], NAMES).read()
    assert c["truth_entries"] == 210 and c["sites_missed"] == 70 and c["wrong_allele"] == 28 and c["no_site"] == 20 and c["unknown_contig"] == 1
    assert c["sites_found"] == 210 - 70 - 28 and c["qual_missing"] > 0 and (by_qual[:, 0] > 0).sum() > 30 and by_ad[:, 0].sum() == c["sites_found"]


# ---- the library's surface ---------------------------------------------------------------------------------------------------------
SYMBOLS = ["simmr_vcfeval_create", "simmr_vcfeval_destroy", "simmr_vcfeval_reset", "simmr_vcfeval_truth_add", "simmr_vcfeval_truth_plan",
           "simmr_vcfeval_add", "simmr_vcfeval_read", "simmr_vcfeval_emit", "simmr_last_vcfeval_ms"]


def test_symbols_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in SYMBOLS:
        assert re.search(rf"^(?:int|void) {name}\(", header, re.M), name
        assert name in _abi.SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(_abi.VcfevalCounts) == 8 * len(_abi.VCFEVAL_COUNTS) == 8 * 24 and _abi.VCFEVAL_COUNTS == _vcfeval.COUNTS
    fields = re.search(r"typedef struct simmr_vcfeval_counts \{(.*?)\} simmr_vcfeval_counts;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert tuple(re.findall(r"\b([a-z_]+)\s*[,;]", fields)) == _abi.VCFEVAL_COUNTS
    assert int(re.search(r"#define SIMMR_VCFEVAL_AD_ROWS (\d+)u", header).group(1)) == _abi.VCFEVAL_AD_ROWS == _vcfeval.AD_ROWS == 33
    assert C.sizeof(_abi.VcfevalConfig) == 16 and "#define SIMMR_ABI_VERSION 1\n" in header
    kernels = (CSRC / "vcfeval_kernels.hip").read_text()
    assert re.search(r"#define VCE_MIN_LINE 15u", kernels) and "Room for an entry per 15 bytes" in header


def test_calls_need_an_object():
    lib = _abi.load()
    h, n, ms = C.c_void_p(), C.c_uint64(), C.c_float()
    assert lib.simmr_vcfeval_create(None, C.byref(h)) == _abi.EINVAL
    assert lib.simmr_vcfeval_reset(None, C.byref(_abi.VcfevalConfig())) == _abi.EINVAL
    assert lib.simmr_vcfeval_truth_add(None, None, 0) == _abi.EINVAL and lib.simmr_vcfeval_add(None, None, 0) == _abi.EINVAL
    assert lib.simmr_vcfeval_truth_plan(None, C.byref(n)) == _abi.EINVAL
    assert lib.simmr_vcfeval_read(None, C.byref(_abi.VcfevalCounts()), None, None) == _abi.EINVAL
    assert lib.simmr_vcfeval_emit(None, None, None, None, None, None, 0) == _abi.EINVAL
    assert lib.simmr_last_vcfeval_ms(None, C.byref(ms)) == _abi.EINVAL
    lib.simmr_vcfeval_destroy(None)


def test_the_unit_is_built_without_a_slot_of_the_engine():
    make = (CSRC / "Makefile").read_text()
    assert make.count(" vcfeval.hip ovleval.hip mapeval.hip ") == 2
    srcs = re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
    assert {"vcfeval.hip", "vcfeval_kernels.hip"} <= set(srcs)
    assert "ENG_EXT_COUNT = 12" in (CSRC / "engine_internal.hpp").read_text()
    unit = (CSRC / "vcfeval.hip").read_text()
    assert "eng_ext_slot" not in unit and "unit_state" not in unit and '#include "engine.hip"' not in unit and '#include "kernels.hip"' not in unit
    assert '#include "host_support.hpp"' in unit and "Spans<" in unit and sorts_through_the_pair_sort("vcfeval.hip")
    for text in (unit, (CSRC / "vcfeval_kernels.hip").read_text()):
        assert not re.search(r"\bhipFree\(|\bhipEventDestroy\(|\bhipEventElapsedTime\(|#\s*define\s+\w*_TRY\b", text)


# ---- the command line --------------------------------------------------------------------------------------------------------------
EVAL = ["--eval-vcf", "c.vcf", "--eval-vcf-truth", "t.vcf", "--eval-vcf-report", "r.tsv"]
ONLY = "it takes only --eval-vcf-truth, --eval-vcf-report, --eval-vcf-sites, --eval-vcf-filtered and --device"
USAGE_ERRORS = [
    (EVAL + ["--num-reads", "5"], f"error: --eval-vcf runs no simulation: {ONLY} ('--num-reads' given)"),
    (["--genome", "g.fna"] + EVAL, f"error: --eval-vcf runs no simulation: {ONLY} ('--genome' given)"),
    (EVAL + ["--output", "x.fq"], f"error: --eval-vcf runs no simulation: {ONLY} ('--output' given)"),
    (EVAL + ["--strain-vcf", "x.vcf"], f"error: --eval-vcf runs no simulation: {ONLY} ('--strain-vcf' given)"),
    (EVAL + ["--with-ani", "95"], f"error: --eval-vcf runs no simulation: {ONLY} ('--with-ani' given)"),
    (EVAL + ["--devices", "0,1"], f"error: --eval-vcf runs no simulation: {ONLY} ('--devices' given)"),
    (EVAL + ["--eval-overlaps", "a.paf", "--eval-overlaps-truth", "t.paf", "--eval-overlaps-report", "r2.tsv"],
     "error: --eval-overlaps runs no simulation: it takes only --eval-overlaps-truth, --eval-overlaps-report, --eval-overlaps-pairs, --eval-overlaps-min-pct "
     "and --device ('--eval-vcf' given)"),
    (EVAL[:4], "error: --eval-vcf needs --eval-vcf-report"),
    (EVAL[:2] + EVAL[4:], "error: --eval-vcf needs --eval-vcf-truth"),
    (EVAL[2:], "error: --eval-vcf-truth needs --eval-vcf"),
    (["--eval-vcf-sites", "x.tsv"], "error: --eval-vcf-sites needs --eval-vcf"),
    (["--eval-vcf-filtered", "--genome", "g.fna", "--output", "x.fq"], "error: --eval-vcf-filtered needs --eval-vcf"),
    (["--eval-vcf"], "error: a value is required for '--eval-vcf'"),
    (["--eval-vcf-report="], "error: a file name is required for '--eval-vcf-report'"),
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
    flags = ["--eval-overlaps-min-pct <PCT>", "--eval-vcf <FILE>", "--eval-vcf-truth <FILE>", "--eval-vcf-report <FILE>", "--eval-vcf-sites <FILE>",
             "--eval-vcf-filtered", "--stats <FILE>"]
    at = [text.index("            " + f) for f in flags]
    assert at == sorted(at) and text[at[0]:at[1]].count("\n") == 1
    assert "no simulation" in text[at[1]:at[2]] and "##contig" in text[at[2]:at[3]]


# ---- host.cpp's routines under the sanitizers --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("vcfeval") / "vcfeval_report_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "vcfeval_report_main.cpp"), str(HOST / "host.cpp")])
    return exe


def ask(exe, block: bytes) -> bytes:
    r = subprocess.run([str(exe)], input=block, capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    assert r.stdout.endswith(b"--\n")
    return r.stdout[:-3]


def report_block(counts, by_qual, by_ad) -> bytes:
    out = "report\n" + " ".join(str(counts[n]) for n in _vcfeval.COUNTS) + "\n"
    for by in (by_qual, by_ad):
        rows = [(b, int(by[b, 0]), int(by[b, 1])) for b in range(len(by)) if by[b].sum()]
        out += f"{len(rows)}\n" + "".join(f"{b} {x} {y}\n" for b, x, y in rows)
    return out.encode()


def test_report_formatter(report_main):
    rng = np.random.default_rng(5)
    for case in range(4):
        counts = {n: int(v) for n, v in zip(_vcfeval.COUNTS, rng.integers(0, 2 ** 40, 24))}
        by_qual, by_ad = np.zeros((256, 2), dtype=np.uint64), np.zeros((33, 2), dtype=np.uint64)
        if case < 3:
            for q in rng.choice(256, size=(1, 9, 256)[case], replace=False):
                by_qual[q] = rng.integers(0, (5, 10 ** 6, 2 ** 33)[case], 2)
            for b in rng.choice(33, size=(1, 5, 33)[case], replace=False):
                by_ad[b] = rng.integers(0, (5, 10 ** 6, 2 ** 33)[case], 2)
            by_qual[255 if case else 0] = (3, 0)
            by_ad[32 if case else 0] = (0, 2)
        got = ask(report_main, report_block(counts, by_qual, by_ad))
        assert got == _vcfeval.report(counts, by_qual, by_ad), case
        assert got.count(b"\nQ\t") == int((by_qual.sum(axis=1) > 0).sum()) and got.count(b"\nAD\t") == int((by_ad.sum(axis=1) > 0).sum())
    zero = dict.fromkeys(_vcfeval.COUNTS, 0)
    by_qual, by_ad = np.zeros((256, 2), dtype=np.uint64), np.zeros((33, 2), dtype=np.uint64)
    got = ask(report_main, report_block(zero, by_qual, by_ad))
    assert got == _vcfeval.report(zero, by_qual, by_ad) and got.endswith(b"#precision\t0/0\t0\n#recall\t0/0\t0\n")
    # two of three calls correct, one of four sites found; the better QUAL first
    c = dict(zero, truth_entries=4, calls=3, correct=2, wrong=1, no_site=1, sites_found=1, sites_missed=3, sites_multiple=1)
    by_qual[30], by_qual[7], by_ad[3], by_ad[0] = (1, 0), (1, 1), (1, 0), (0, 3)
    got = ask(report_main, report_block(c, by_qual, by_ad))
    assert got == _vcfeval.report(c, by_qual, by_ad)
    assert got.endswith(b"#precision\t2/3\t66.6667\n#recall\t1/4\t25.0000\nQ\t30\t1\t0\t1/1\t100.0000\t1/4\t25.0000\nQ\t7\t1\t1\t2/3\t66.6667\t2/4\t50.0000\n"
                        b"AD\t0\t0\t3\nAD\t3\t1\t0\n")


def test_site_rows_and_contig_names(report_main):
    names = [b"chr1", b"g|c2"]
    key = np.array([0, 99, 2 ** 40 - 1, 1 << 40 | 4], dtype=np.uint64)
    alleles = np.array([0 << 2 | 1, 3 << 2 | 0, 2 << 2 | 3, 1 << 2 | 2], dtype=np.uint32)
    ad = np.array([0, 7, 2 ** 32 - 1, 12], dtype=np.uint32)
    best = np.array([0, 3 << 8 | 255, 2 << 8, 3 << 8 | 30], dtype=np.uint32)
    hits = np.array([0, 1, 2 ** 32 - 1, 2], dtype=np.uint32)
    block = f"sites 2 {len(key)}\nchr1 g|c2\n" + "".join(f"{k} {a} {d} {b} {h}\n" for k, a, d, b, h in zip(key, alleles, ad, best, hits))
    got = ask(report_main, block.encode())
    assert got == _vcfeval.site_rows(names, key, alleles, ad, best, hits)
    assert got.split(b"\n")[:4] == [b"chr1\t1\tA\tC\t0\t0\t0\t0", b"chr1\t100\tT\tA\t7\t3\t255\t1", b"chr1\t1099511627776\tG\tT\t4294967295\t2\t0\t4294967295",
                                    b"g|c2\t5\tC\tG\t12\t3\t30\t2"]
    assert ask(report_main, b"sites 0 0\n") == b""
    head = b"##fileformat=VCFv4.2\n##contig=<ID=g0|c1,length=5>\n##contig=<ID=>\n##contig=<ID=last>\n#CHROM\n##contig=<ID=open"
    assert ask(report_main, b"contigs %d\n" % len(head) + head) == b"g0|c1\nlast\nopen\n"
    assert _vcfeval.contig_names(head) == [b"g0|c1", b"last", b"open"]
    assert ask(report_main, b"contigs 0\n") == b""
