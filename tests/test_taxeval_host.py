"""Scoring a read classifier's calls against each read's true genome, without a GPU: the plain restatement of the rules
(tests/_taxeval.py) on hand-written records whose classes and counts are written out here, one case per row of the class table,
per step of the record order and per malformed form; every refusal of the taxonomy; the symbols of simmr_taxeval_*; the command
line's usage rows and usage errors; the build facts of the new translation unit; and the formatters and small-file readers of
host.cpp in a stand-alone program under the sanitizers."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _taxeval
from tests._taxeval import Malformed, Refused, call, small_tree, tree_of, truth_line

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "simmr_amd" / "csrc"
HOST = ROOT / "simmr_amd" / "host"

TAXONOMY, GENOMES = small_tree()
HEADER = b"read_id\tpair\tgenome_id\tsequence_id\tstart\tend\tstrand\tlength\tNM\tedits\n"
# read 1 is a pair from the strain, 2 a read of the genome placed at species, 3 the one under the unranked clade, 4 the other genus,
# 5 the one whose lineage lacks phylum .. genus, 6 a second read of the strain
TRUTH = (HEADER + truth_line(1, 1, "gStrain") + truth_line(1, 2, "gStrain") + truth_line(2, 0, "gSpecies") + truth_line(3, 0, "gClade")
         + truth_line(4, 0, "gOther") + truth_line(5, 0, "gArch") + truth_line(6, 0, "gStrain"))

# what one record gives: the count it goes to, its class at the ranks 1 .. 8 as digits, and the node its lca count goes to
RULES = [
    ("correct down to the strain", call(1, 61), "scored", "44444444", 61),
    ("a genome placed at species, a call at a strain below it", call(2, 61), "scored", "44444440", 60),
    ("a genome placed at a strain, a call at its genus: above", call(1, 50), "scored", "44444433", 50),
    ("a call at an unranked clade on the path", call(3, 55), "scored", "44444430", 55),
    ("a call at an unranked clade off the path", call(3, 45), "scored", "44444220", 40),
    ("a lineage that lacks ranks: absent", call(5, 90), "scored", "40000040", 90),
    ("the other domain: the lca is the root", call(5, 61), "scored", "20000020", 1),
    ("another species of the genus", call(1, 70), "scored", "44444422", 50),
    ("another genus of the family", call(4, 60), "scored", "44444220", 40),
    ("the root itself: above at every rank", call(6, 1), "scored", "33333333", 1),
    ("unclassified", call(1, 0), "unclassified", "11111111", None),
    ("unclassified where ranks are absent", call(5, 0), "unclassified", "10000010", None),
    ("C with taxid 0", call(2, 0, classified=True), "unclassified", "11111110", None),
    ("U with a taxid", call(2, 61, classified=False), "unclassified", "11111110", None),
    ("a taxid that is no node", call(2, 999), "unknown_taxon", "22222220", None),
    ("the largest taxid", call(3, 2 ** 32 - 1), "unknown_taxon", "22222220", None),
    ("the --use-names form", call(1, 61, names="Escherichia coli K-12 (x)"), "scored", "44444444", 61),
    ("the --use-names form, unclassified", call(1, 0, names="unclassified"), "unclassified", "11111111", None),
    ("a name glued to the bracket", b"C\t1\tx(taxid 61)\n", "scored", "44444444", 61),
    ("mate 1", call("1/1", 61), "scored", "44444444", 61),
    ("mate 2", call("1/2", 60), "scored", "44444443", 60),
    ("three fields and no more", b"C\t2\t60", "scored", "44444440", 60),
    ("a name that is no read id", call("read7", 61), "unknown_read", None, None),
    ("a mate that is none", call("1/3", 61), "unknown_read", None, None),
    ("an id without an entry", call(7, 61), "unknown_read", None, None),
    ("nineteen digits", call("1" * 19, 61), "unknown_read", None, None),
]
MALFORMED_TRUTH = {
    "two fields": b"9\t0\n",
    "an id that is no number": truth_line("r9", 0, "gStrain"),
    "an empty id": truth_line("", 0, "gStrain"),
    "nineteen digits": truth_line("1" * 19, 0, "gStrain"),
    "a pair of 3": truth_line(9, 3, "gStrain"),
    "a pair of two digits": truth_line(9, "01", "gStrain"),
    "an empty pair": truth_line(9, "", "gStrain"),
    "a genome outside the names": truth_line(9, 0, "gStrai"),
    "a longer genome id": truth_line(9, 0, "gStrainX"),
    "an empty genome id": truth_line(9, 0, ""),
}
MALFORMED_CALLS = {
    "two fields": b"C\t1\n",
    "a lower-case c": b"c\t1\t61\n",
    "two letters": b"CU\t1\t61\n",
    "an empty first field": b"\t1\t61\n",
    "an empty taxon": b"C\t1\t\t5\n",
    "a taxon with a letter": b"C\t1\t61a\n",
    "eleven digits": b"C\t1\t00000000061\n",
    "2^32": b"C\t1\t4294967296\n",
    "a sign": b"C\t1\t-1\n",
    "a bracket without digits": b"C\t1\tx (taxid )\n",
    "a bracket that is not closed": b"C\t1\tx (taxid 61\n",
    "another word in the bracket": b"C\t1\tx (taxi 61)\n",
    "2^32 in the bracket": b"C\t1\tx (taxid 4294967296)\n",
    "eleven digits in the bracket": b"C\t1\tx (taxid 00000000061)\n",
    "a bracket alone": b"U\t1\t)\n",
}
TREE_REFUSALS = {   # rows of (taxid, parent, rank), the genomes, the error
    "a taxid of 0": ([(1, 1, 0), (0, 1, 7)], [], "EINVAL"),
    "a taxid given twice": ([(1, 1, 0), (5, 1, 7), (5, 1, 6)], [], "EINVAL"),
    "a parent that is no node": ([(1, 1, 0), (5, 4, 7)], [], "EINVAL"),
    "a cycle": ([(1, 1, 0), (5, 6, 0), (6, 5, 0)], [], "EINVAL"),
    "a rank code of 9": ([(1, 1, 0), (5, 1, 9)], [], "EINVAL"),
    "a rank twice in a lineage": ([(1, 1, 0), (5, 1, 7), (6, 5, 0), (7, 6, 7)], [], "EINVAL"),
    "a genome whose taxid is no node": ([(1, 1, 0), (5, 1, 7)], [("g", 6)], "EINVAL"),
    "a genome whose taxid is 0": ([(1, 1, 0), (5, 1, 7)], [("g", 0)], "EINVAL"),
    "a genome id given twice": ([(1, 1, 0), (5, 1, 7)], [("g", 5), ("h", 5), ("g", 1)], "EINVAL"),
    "an empty genome id": ([(1, 1, 0)], [("", 1)], "ENOTSUP"),
    "a genome id of 255 bytes": ([(1, 1, 0)], [("g" * 255, 1)], "ENOTSUP"),
    "a genome id with a tab": ([(1, 1, 0)], [("g\th", 1)], "ENOTSUP"),
    "a genome id with a newline": ([(1, 1, 0)], [("g\n", 1)], "ENOTSUP"),
}


def one(cand: bytes):
    m = _taxeval.evaluate([TRUTH], [cand], TAXONOMY, GENOMES)
    return m, m.read()


def test_the_truth_written_out():
    m = _taxeval.evaluate([TRUTH], [], TAXONOMY, GENOMES)
    c, by_rank, reads_by_rank = m.read()
    assert c == dict(truth_lines=8, truth_header=1, truth_entries=6, truth_paired=1, lines=0, header=0, records=0, unknown_read=0, unclassified=0,
                     unknown_taxon=0, scored=0, missing=6, multiple=0)
    rid, genome, mates, seen, hits = m.reads()
    assert m.tree.genome_ids == [b"gArch", b"gClade", b"gOther", b"gSpecies", b"gStrain"]
    assert rid.tolist() == [1, 2, 3, 4, 5, 6] and genome.tolist() == [4, 3, 1, 2, 0, 4] and mates.tolist() == [2, 1, 1, 1, 1, 1]
    assert seen.tolist() == hits.tolist() == [0] * 6 and by_rank.sum() == 0
    # a read without a record is unclassified at the ranks its genome has: all six have a domain and a species, two a strain
    assert reads_by_rank[:, 1].tolist() == [6, 5, 5, 5, 5, 5, 6, 2] and reads_by_rank[:, 0].tolist() == [0, 1, 1, 1, 1, 1, 0, 4] and reads_by_rank[:, 2:].sum() == 0
    assert all(col.sum() == 0 for col in m.taxa()[1:]) and m.taxa()[0].tolist() == sorted(t for t, _, _ in _taxeval.SMALL_ROWS)


def test_the_lineages_written_out():
    T = _taxeval.Tree(TAXONOMY, GENOMES)
    assert T.lineage(61) == ([2, 10, 20, 30, 40, 50, 60, 61], 8) and T.lineage(60) == ([2, 10, 20, 30, 40, 50, 60, 0], 7)
    assert T.lineage(71) == ([2, 10, 20, 30, 40, 50, 71, 0], 8) and T.lineage(55) == ([2, 10, 20, 30, 40, 50, 0, 0], 7)
    assert T.lineage(45) == ([2, 10, 20, 30, 40, 0, 0, 0], 6) and T.lineage(90) == ([3, 0, 0, 0, 0, 0, 90, 0], 2)
    assert T.lineage(1) == ([0] * 8, 0) and T.lineage(3) == ([3, 0, 0, 0, 0, 0, 0, 0], 1)
    assert _taxeval.Tree(_taxeval.chain(255), []).lineage(256) == ([0, 0, 0, 0, 0, 0, 256, 0], 255)
    with pytest.raises(Refused):
        _taxeval.Tree(_taxeval.chain(256), [])
    two_roots = _taxeval.Tree(tree_of([(5, 0, 1), (6, 6, 1), (7, 5, 7), (8, 6, 7)]), [])   # a parent of 0 is a root too
    assert two_roots.depth == [0, 0, 1, 1] and two_roots.lca(2, 3) == _taxeval.NONE and two_roots.lca(2, 0) == 0


@pytest.mark.parametrize("what,cand,count,classes,lca", RULES, ids=[r[0] for r in RULES])
def test_each_rule(what, cand, count, classes, lca):
    m, (c, by_rank, reads_by_rank) = one(cand)
    assert {k: v for k, v in c.items() if v and k in _taxeval.COUNTS[4:11]} == {"lines": 1, "records": 1, count: 1}
    rid, genome, mates, seen, hits = m.reads()
    taxid, true, called, both = m.taxa()
    if classes is None:
        assert by_rank.sum() == 0 and hits.sum() == 0 and seen.sum() == 0 and c["missing"] == 6 and true.sum() == called.sum() == 0
        return
    want = [int(k) for k in classes]
    assert [int(np.argmax(by_rank[r])) for r in range(8)] == want and by_rank.sum() == 8 and by_rank.max() == 1
    e = int(np.flatnonzero(hits)[0])
    assert hits.sum() == 1 and int(seen[e]) == sum(1 << (4 * r + k - 1) for r, k in enumerate(want) if k) and m.best(e) == want
    assert c["missing"] == 5 and [int(reads_by_rank[r, k]) for r, k in enumerate(want)] >= [1] * 8
    # the clade sums: the genome's node and everything above it hold the read; the lca and everything above it hold the true positive
    T, t = m.tree, m.tree.genome_node[genome[e]]
    path = lambda x: [] if x == T.parent[x] and False else ([x] + ([] if T.parent[x] == x else path(T.parent[x])))
    assert sorted(np.flatnonzero(true)) == sorted(path(t)) and true.max() == 1
    if lca is None:
        assert called.sum() == both.sum() == 0
    else:
        assert sorted(np.flatnonzero(both)) == sorted(path(T.row[lca])) and called.sum() >= both.sum()


def test_the_order_of_the_steps_and_the_best_class():
    # a malformed third field beats an unknown read; an unknown read beats U; U beats an unknown taxon
    with pytest.raises(Malformed):
        one(b"U\tnobody\tx\n")[0].read()
    assert one(call("nobody", 0))[1][0]["unknown_read"] == 1 and one(call(1, 999, classified=False))[1][0]["unclassified"] == 1
    # read 1: unclassified, wrong species, then its genus; read 2 twice: multiple; the pair 1 has two lines, so three records are multiple too
    m, (c, by_rank, reads_by_rank) = one(call("1/1", 0) + call("1/2", 70) + call(1, 50) + call(2, 61) + call(2, 999) + call(6, 61))
    assert (c["records"], c["scored"], c["unclassified"], c["unknown_taxon"], c["missing"], c["multiple"]) == (6, 4, 1, 1, 3, 2)
    assert m.best(0) == [4, 4, 4, 4, 4, 4, 3, 3] and m.best(1) == [4, 4, 4, 4, 4, 4, 4, 0] and m.reads()[4].tolist() == [3, 2, 0, 0, 0, 1]
    assert by_rank[6].tolist() == [0, 1, 2, 1, 2] and by_rank[7].tolist() == [2, 1, 1, 1, 1]
    assert reads_by_rank[6].tolist() == [0, 3, 0, 1, 2] and reads_by_rank[7].tolist() == [4, 0, 0, 1, 1]
    taxid, true, called, both = m.taxa()
    at = {int(t): i for i, t in enumerate(taxid)}
    assert [int(true[at[t]]) for t in (1, 50, 60, 61)] == [6, 6, 6, 4] and [int(called[at[t]]) for t in (1, 50, 60, 61, 70)] == [4, 4, 2, 2, 1]
    assert [int(both[at[t]]) for t in (1, 50, 60, 61, 70)] == [4, 4, 2, 1, 0]
    assert np.array_equal(m.taxa()[2], called)   # a second call gives the same answer


def test_what_is_malformed_and_where():
    for what, bad in MALFORMED_TRUTH.items():
        with pytest.raises(Malformed):
            _taxeval.evaluate([TRUTH + bad], [], TAXONOMY, GENOMES)
        if bad.count(b"\t") >= 2:   # ... and a candidate may hold them: their first field is no C or U, so they are malformed there too
            with pytest.raises(Malformed):
                one(bad)[0].read()
    for what, bad in MALFORMED_CALLS.items():
        with pytest.raises(Malformed):
            one(call(1, 61) + bad + call(2, 60))[0].read()
    assert _taxeval.lines(b"\na\n\nb") == [b"a", b"b"] and _taxeval.is_header(b"#x") and _taxeval.is_header(b"read_id\tx") and not _taxeval.is_header(b"read_id")
    for text, code in (([truth_line(1, 0, "gStrain"), truth_line(1, 0, "gArch")], "EINVAL"), ([truth_line(1, 1, "gArch") * 3], "EINVAL")):
        with pytest.raises(Refused) as err:
            _taxeval.evaluate(text, [], TAXONOMY, GENOMES)
        assert err.value.code == code
    assert _taxeval.taxon(b"9 (taxid 4294967295)") == 2 ** 32 - 1 and _taxeval.taxon(b"(taxid 7)") == 7 and _taxeval.taxon(b"0000000061") == 61


@pytest.mark.parametrize("what", list(TREE_REFUSALS))
def test_taxonomy_refusals(what):
    rows, genomes, code = TREE_REFUSALS[what]
    with pytest.raises(Refused) as err:
        _taxeval.Tree(tree_of(rows), genomes)
    assert err.value.code == code


# ---- the library's surface ---------------------------------------------------------------------------------------------------------
SYMBOLS = ["simmr_taxeval_create", "simmr_taxeval_destroy", "simmr_taxeval_reset", "simmr_taxeval_lineage", "simmr_taxeval_truth_add",
           "simmr_taxeval_truth_plan", "simmr_taxeval_add", "simmr_taxeval_read", "simmr_taxeval_emit", "simmr_taxeval_taxa", "simmr_last_taxeval_ms"]


def test_symbols_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in SYMBOLS:
        assert re.search(rf"^(?:int|void) {name}\(", header, re.M), name
        assert name in _abi.SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(_abi.TaxevalCounts) == 8 * len(_abi.TAXEVAL_COUNTS) == 8 * 13 and _abi.TAXEVAL_COUNTS == _taxeval.COUNTS
    fields = re.search(r"typedef struct simmr_taxeval_counts \{(.*?)\} simmr_taxeval_counts;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert tuple(re.findall(r"\b([a-z_]+)\s*[,;]", fields)) == _abi.TAXEVAL_COUNTS
    for name, value in (("RANKS", 8), ("CLASSES", 5), ("MAX_DEPTH", 255)):
        assert int(re.search(rf"#define SIMMR_TAXEVAL_{name} (\d+)u", header).group(1)) == getattr(_abi, "TAXEVAL_" + name) == getattr(_taxeval, name) == value
    assert C.sizeof(_abi.TaxevalConfig) == 56 and "Replaces nothing in the reference" in header[header.index("a read classifier's calls"):]
    kernels = (CSRC / "taxeval_kernels.hip").read_text()
    assert re.search(r"#define TXE_MIN_LINE 5u", kernels) and "Room for a line per 5 bytes" in header


def test_calls_need_an_object():
    lib = _abi.load()
    h, n, ms = C.c_void_p(), C.c_uint64(), C.c_float()
    assert lib.simmr_taxeval_create(None, C.byref(h)) == _abi.EINVAL
    assert lib.simmr_taxeval_reset(None, C.byref(_abi.TaxevalConfig())) == _abi.EINVAL
    assert lib.simmr_taxeval_truth_add(None, None, 0) == _abi.EINVAL and lib.simmr_taxeval_add(None, None, 0) == _abi.EINVAL
    assert lib.simmr_taxeval_truth_plan(None, C.byref(n)) == _abi.EINVAL and lib.simmr_taxeval_lineage(None, 1, None, None) == _abi.EINVAL
    assert lib.simmr_taxeval_read(None, C.byref(_abi.TaxevalCounts()), None, None) == _abi.EINVAL
    assert lib.simmr_taxeval_emit(None, None, None, None, None, None, 0) == _abi.EINVAL
    assert lib.simmr_taxeval_taxa(None, None, None, None, None, 0) == _abi.EINVAL
    assert lib.simmr_last_taxeval_ms(None, C.byref(ms)) == _abi.EINVAL
    lib.simmr_taxeval_destroy(None)


def test_the_unit_is_built_without_a_slot_of_the_engine():
    make = (CSRC / "Makefile").read_text()
    assert make.count(" taxeval.hip vcfeval.hip ovleval.hip mapeval.hip ") == 2
    srcs = re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
    assert {"taxeval.hip", "taxeval_kernels.hip"} <= set(srcs)
    unit = (CSRC / "taxeval.hip").read_text()
    assert "eng_ext_slot" not in unit and "unit_state" not in unit and '#include "engine.hip"' not in unit and '#include "kernels.hip"' not in unit
    assert '#include "host_support.hpp"' in unit and "Spans<" in unit and unit.count("samsort_sort_pairs(") >= 2 and "DevBuf" in unit and "HIP_TRY(" in unit
    for text in (unit, (CSRC / "taxeval_kernels.hip").read_text()):
        assert not re.search(r"\bhipFree\(|\bhipEventDestroy\(|\bhipEventElapsedTime\(|#\s*define\s+\w*_TRY\b", text)
    from simmr_amd import engine
    assert {"truth_add", "truth_plan", "add", "read", "reads", "taxa", "lineage", "close"} <= set(dir(engine.TaxEval))
    assert hasattr(engine.Engine, "classify_eval_open") and hasattr(engine.Engine, "classify_eval")


# ---- the command line --------------------------------------------------------------------------------------------------------------
EVAL = ["--eval-classified", "c.txt", "--eval-classified-truth", "t.tsv", "--eval-taxonomy", "nodes.dmp", "--eval-genome-taxa", "m.tsv",
        "--eval-classified-report", "r.tsv"]
ONLY = ("it takes only --eval-classified-truth, --eval-taxonomy, --eval-genome-taxa, --eval-classified-report, --eval-classified-reads, "
        "--eval-classified-taxa and --device")


def without(flag):
    at = EVAL.index(flag)
    return EVAL[:at] + EVAL[at + 2:]


USAGE_ERRORS = [
    (EVAL + ["--num-reads", "5"], f"error: --eval-classified runs no simulation: {ONLY} ('--num-reads' given)"),
    (["--genome", "g.fna"] + EVAL, f"error: --eval-classified runs no simulation: {ONLY} ('--genome' given)"),
    (EVAL + ["--output", "x.fq"], f"error: --eval-classified runs no simulation: {ONLY} ('--output' given)"),
    (EVAL + ["--truth", "x.tsv"], f"error: --eval-classified runs no simulation: {ONLY} ('--truth' given)"),
    (EVAL + ["--devices", "0,1"], f"error: --eval-classified runs no simulation: {ONLY} ('--devices' given)"),
    (EVAL + ["--eval-vcf", "a.vcf", "--eval-vcf-truth", "t.vcf", "--eval-vcf-report", "r2.tsv"],
     "error: --eval-vcf runs no simulation: it takes only --eval-vcf-truth, --eval-vcf-report, --eval-vcf-sites, --eval-vcf-filtered and --device "
     "('--eval-classified' given)"),
    (without("--eval-classified-report"), "error: --eval-classified needs --eval-classified-report"),
    (without("--eval-classified-truth"), "error: --eval-classified needs --eval-classified-truth"),
    (without("--eval-taxonomy"), "error: --eval-classified needs --eval-taxonomy"),
    (without("--eval-genome-taxa"), "error: --eval-classified needs --eval-genome-taxa"),
    (EVAL[2:], "error: --eval-classified-truth needs --eval-classified"),
    (["--eval-classified-reads", "x.tsv"], "error: --eval-classified-reads needs --eval-classified"),
    (["--eval-classified-taxa", "x.tsv", "--genome", "g.fna", "--output", "x.fq"], "error: --eval-classified-taxa needs --eval-classified"),
    (["--eval-classified"], "error: a value is required for '--eval-classified'"),
    (["--eval-taxonomy="], "error: a file name is required for '--eval-taxonomy'"),
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
    flags = ["--eval-vcf-filtered", "--eval-classified <FILE>", "--eval-classified-truth <FILE>", "--eval-taxonomy <FILE>", "--eval-genome-taxa <FILE>",
             "--eval-classified-report <FILE>", "--eval-classified-reads <FILE>", "--eval-classified-taxa <FILE>", "--stats <FILE>"]
    at = [text.index("            " + f) for f in flags]
    assert at == sorted(at) and text[at[0]:at[1]].count("\n") == 1
    assert "no simulation" in text[at[1]:at[2]] and "nodes.dmp" in text[at[3]:at[4]] and "L1 distance" in text[at[5]:at[6]]


# ---- host.cpp's routines under the sanitizers --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("taxeval") / "taxeval_report_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "taxeval_report_main.cpp"), str(HOST / "host.cpp")])
    return exe


def ask(exe, block: bytes) -> bytes:
    r = subprocess.run([str(exe)], input=block, capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    assert r.stdout.endswith(b"--\n")
    return r.stdout[:-3]


def report_block(counts, by_rank, reads_by_rank, rank, true, called) -> bytes:
    out = f"report {len(rank)}\n" + " ".join(str(counts[n]) for n in _taxeval.COUNTS) + "\n"
    out += " ".join(str(int(v)) for v in by_rank.ravel()) + "\n" + " ".join(str(int(v)) for v in reads_by_rank.ravel()) + "\n"
    return (out + "".join(f"{int(r)} {int(t)} {int(c)}\n" for r, t, c in zip(rank, true, called))).encode()


def test_report_formatter(report_main):
    rng = np.random.default_rng(11)
    for case in range(3):
        counts = {n: int(v) for n, v in zip(_taxeval.COUNTS, rng.integers(0, 2 ** 40, 13))}
        by_rank, reads_by_rank = (rng.integers(0, (7, 10 ** 6, 2 ** 40)[case], (8, 5)).astype(np.uint64) for _ in range(2))
        n = (1, 40, 500)[case]
        rank, true, called = rng.integers(0, 9, n), rng.integers(0, (3, 10 ** 4, 2 ** 36)[case], n), rng.integers(0, (3, 10 ** 4, 2 ** 36)[case], n)
        got = ask(report_main, report_block(counts, by_rank, reads_by_rank, rank, true, called))
        assert got == _taxeval.report(counts, by_rank, reads_by_rank, rank, true, called), case
    zero = dict.fromkeys(_taxeval.COUNTS, 0)
    none = np.zeros((8, 5), dtype=np.uint64)
    got = ask(report_main, report_block(zero, none, none, [], [], []))
    assert got == _taxeval.report(zero, none, none, [], [], []) and got.count(b"NA") == 8 * 6 + 8
    assert got.endswith(b"A\t8\tstrain\t0\tNA\n") and b"P\t1\tdomain\tNA\tNA\tNA\tNA\tNA\tNA\n" in got
    # the model on the hand-written run: three of four species calls correct ... and an NA row where no record reached the rank
    m = _taxeval.evaluate([TRUTH], [call(1, 61) + call(2, 61) + call(3, 71) + call(4, 70) + call(5, 0)], TAXONOMY, GENOMES)
    c, by_rank, reads_by_rank = m.read()
    taxid, true, called, both = m.taxa()
    got = ask(report_main, report_block(c, by_rank, reads_by_rank, m.tree.rank, true, called))
    assert got == _taxeval.report(c, by_rank, reads_by_rank, m.tree.rank, true, called)
    assert b"R\t7\tspecies\t0\t1\t1\t0\t3\t0\t2\t1\t0\t3\n" in got and b"P\t7\tspecies\t0.750000\t0.600000\t0.666667\t0.750000\t0.500000\t0.600000\n" in got
    assert b"P\t8\tstrain\t1.000000\t1.000000\t1.000000\t1.000000\t0.500000\t0.666667\n" in got
    # the five species: true 60 x 2, 71, 81, 90 against called 60 x 2, 71, 70: |2/5 - 2/4| + |1/5 - 1/4| + |0 - 1/4| + 1/5 + 1/5
    assert b"A\t7\tspecies\t5\t0.800000\n" in got and b"A\t1\tdomain\t2\t0.400000\n" in got


def test_read_rows_and_taxa_rows(report_main):
    m = _taxeval.evaluate([TRUTH], [call("1/1", 0) + call("1/2", 70) + call(1, 50) + call(2, 61) + call(5, 90)], TAXONOMY, GENOMES)
    rid, genome, mates, seen, hits = m.reads()
    has = _taxeval.genome_has(m)
    want = _taxeval.read_rows(m.tree.genome_ids, has, rid, genome, mates, seen, hits)
    block = f"reads {len(has)} {len(rid)}\n" + "".join(f"{g.decode()} {h}\n" for g, h in zip(m.tree.genome_ids, has))
    block += "".join(f"{a} {b} {c} {d} {e}\n" for a, b, c, d, e in zip(rid, genome, mates, seen, hits))
    assert ask(report_main, block.encode()) == want
    assert want.split(b"\n")[:3] == [b"1\tgStrain\t2\t3\t4\t4\t4\t4\t4\t4\t3\t3", b"2\tgSpecies\t1\t1\t4\t4\t4\t4\t4\t4\t4\t0", b"3\tgClade\t1\t0\t1\t1\t1\t1\t1\t1\t1\t0"]
    assert want.split(b"\n")[4] == b"5\tgArch\t1\t1\t4\t0\t0\t0\t0\t0\t4\t0"
    assert ask(report_main, b"reads 0 1\n18446744073709551615 3 1 4294967295 4294967295\n") == b"18446744073709551615\t?\t1\t4294967295" + b"\t4" * 8 + b"\n"
    taxid, true, called, both = m.taxa()
    want = _taxeval.taxa_rows(taxid, m.tree.rank, true, called, both)
    block = f"taxa {len(taxid)}\n" + "".join(f"{t} {r} {a} {b} {c}\n" for t, r, a, b, c in zip(taxid, m.tree.rank, true, called, both))
    assert ask(report_main, block.encode()) == want
    assert b"61\tstrain\t3\t1\t0\t0.000000\t0.000000\n" in want and b"70\tspecies\t0\t1\t0\t0.000000\tNA\n" in want and b"3\tdomain\t1\t1\t1\t1.000000\t1.000000\n" in want
    assert b"\n45\t" not in want and ask(report_main, b"taxa 0\n") == b"" and ask(report_main, b"taxa 1\n7 0 5 0 0\n") == b"7\tno_rank\t5\t0\t0\tNA\t0.000000\n"


def test_the_small_file_readers(report_main):
    dmp = b"1\t|\t1\t|\tno rank\t|\t\t|\t8\t|\n2\t|\t131567\t|\tsuperkingdom\t|\t\t|\t0\t|\n\n562\t|\t561\t|\tspecies\t|\tEC\t|\n9\t|\t2\t|\tstrain\t|\n"
    assert ask(report_main, b"nodes %d\n" % len(dmp) + dmp) == b"1 1 0\n2 131567 1\n562 561 7\n9 2 8\n"
    tsv = b"1\t0\tdomain\n5\t1\tgenus\textra\r\n4294967295\t5\tsubspecies"
    assert ask(report_main, b"nodes %d\n" % len(tsv) + tsv) == b"1 0 1\n5 1 6\n4294967295 5 0\n"
    for bad, line in ((b"1\t1\n", 1), (b"1\t1\tx\nx\t1\tgenus\n", 2), (b"4294967296\t1\tgenus\n", 1), (b"1\t|\t-1\t|\tgenus\t|\n", 1), (b"\n\n1\t\tgenus\n", 3)):
        assert ask(report_main, b"nodes %d\n" % len(bad) + bad) == b"error: line %d is not 'taxid | parent | rank'\n" % line
    assert ask(report_main, b"nodes 0\n") == b""
    ok = b"genome_id\ttaxid\ng1\t562\n\ng|2 x\t7\tmore\r\n"
    assert ask(report_main, b"map %d\n" % len(ok) + ok) == b"g1 562\ng|2 x 7\n".replace(b"g|2 x 7", b"g|2 x 7")
    assert ask(report_main, b"map 7\ng1\t562\n") == b"g1 562\n" and ask(report_main, b"map 0\n") == b""
    for bad, line in ((b"g1\t5\ng2\ttaxid\n", 2), (b"g1\n", 1), (b"h\tt\n\tx\n", 2), (b"g1\t5\n\t6\n", 2)):
        assert ask(report_main, b"map %d\n" % len(bad) + bad) == b"error: line %d is not 'genome_id <tab> taxid'\n" % line
    for name, code in (("superkingdom", 1), ("domain", 1), ("phylum", 2), ("class", 3), ("order", 4), ("family", 5), ("genus", 6), ("species", 7), ("strain", 8),
                       ("no rank", 0), ("clade", 0), ("subspecies", 0), ("", 0)):
        assert _taxeval.RANK_CODES.get(name, 0) == code
