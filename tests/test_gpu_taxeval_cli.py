"""`simmr-hip --eval-classified CALLS --eval-classified-truth TRUTH --eval-taxonomy NODES --eval-genome-taxa MAP
--eval-classified-report OUT [--eval-classified-reads FILE] [--eval-classified-taxa FILE]` on the GPU box: the truth is the file a
two-genome run on tests/golden/sample.fna wrote with --truth; a candidate derived from it here is part right, part wrong, part above
and part unclassified, with a mate given as /1, a pair given twice, an unknown name and a line in the --use-names form; the three
files must be, byte for byte, what the plain restatement of the rules (tests/_taxeval.py) prints; the usage errors."""
import subprocess
from pathlib import Path

import pytest

from tests import _taxeval
from tests._taxeval import call

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "simmr_amd" / "host" / "simmr-hip"
SAMPLE = ROOT / "tests" / "golden" / "sample.fna"

# genomeA is placed at a strain, genomeB at a species of another genus of the same family
ROWS = [(1, 1, "no rank"), (2, 1, "superkingdom"), (1224, 2, "phylum"), (1236, 1224, "class"), (91347, 1236, "order"), (543, 91347, "family"),
        (561, 543, "genus"), (562, 561, "species"), (83333, 562, "strain"), (590, 543, "genus"), (28901, 590, "species"), (2157, 1, "superkingdom"),
        (131567, 543, "clade")]
GENOMES = [("genomeA", 83333), ("genomeB", 28901)]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "simmr_amd" / "host")])
    d = tmp_path_factory.mktemp("taxeval_cli")
    (d / "genomes.tsv").write_text("path\tid\n" + f"{SAMPLE}\tgenomeA\n{SAMPLE}\tgenomeB\n")
    subprocess.check_call([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "reads.fq"), "--num-reads", "600", "--seed", "11",
                           "--error-profile", "perfect-short", "--read-length", "20", "--insert-size", "20", "--truth", str(d / "truth.tsv")])
    (d / "nodes.dmp").write_text("".join(f"{t}\t|\t{p}\t|\t{r}\t|\t\t|\t11\t|\n" for t, p, r in ROWS))
    (d / "map.tsv").write_text("genome_id\ttaxid\n" + "".join(f"{g}\t{t}\n" for g, t in GENOMES))
    return d


def derive(truth: bytes) -> bytes:
    """a candidate for the truth's reads, by the read's place i in the file"""
    out, seen = [], set()
    for ln in _taxeval.lines(truth):
        if _taxeval.is_header(ln):
            continue
        rid, pair, genome = ln.split(b"\t")[:3]
        rid, first = int(rid), int(rid) not in seen
        seen.add(rid)
        if not first:
            if rid % 50 == 3:   # a pair given twice: both mates, and the first once more
                out.append(call(f"{rid}/2", 562) + call(f"{rid}/1", 562))
            continue
        own = dict(GENOMES)[genome.decode()]
        name = f"{rid}/1" if rid % 9 == 0 else rid                                # one mate of a pair (or a single read) given with /1
        k = rid % 7
        taxid = (own, own, 562, 561, 131567, 0, 99999)[k]                        # right, right, species, genus, an unranked clade, none, no node
        out.append(call(name, taxid, names=("Some taxon" if rid % 10 == 1 else None)))   # the --use-names form
    return b"".join(out) + call("read_x", 562) + call(10 ** 9, 562)               # an unknown name, and an id without an entry


def outputs(d, calls: Path, reads=True, taxa=True):
    report, rows, tx = d / "report.tsv", d / "reads.tsv", d / "taxa.tsv"
    r = subprocess.run([str(EXE), "--eval-classified", str(calls), "--eval-classified-truth", str(d / "truth.tsv"), "--eval-taxonomy", str(d / "nodes.dmp"),
                        "--eval-genome-taxa", str(d / "map.tsv"), "--eval-classified-report", str(report)]
                       + (["--eval-classified-reads", str(rows)] if reads else []) + (["--eval-classified-taxa", str(tx)] if taxa else []),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return report.read_bytes(), rows.read_bytes() if reads else None, tx.read_bytes() if taxa else None


def test_the_three_files_against_the_model(run):
    d = run
    truth = (d / "truth.tsv").read_bytes()
    cand = derive(truth).rstrip(b"\n")   # no newline at the end
    (d / "calls.txt").write_bytes(cand)
    taxonomy = _taxeval.tree_of(ROWS)
    m = _taxeval.evaluate([truth], [cand], taxonomy, GENOMES)
    c, by_rank, reads_by_rank = m.read()
    assert c["truth_header"] == 1 and c["truth_entries"] >= 300 and c["unknown_read"] == 2 and c["multiple"] >= 1 and c["missing"] == 0
    assert min(c["unclassified"], c["unknown_taxon"], c["scored"], by_rank[6, 4], by_rank[6, 3], by_rank[6, 2], by_rank[7, 3], by_rank[7, 0]) > 0
    taxid, true, called, both = m.taxa()
    report, rows, taxa = outputs(d, d / "calls.txt")
    assert report == _taxeval.report(c, by_rank, reads_by_rank, m.tree.rank, true, called)
    assert rows == _taxeval.read_rows(m.tree.genome_ids, _taxeval.genome_has(m), *m.reads()) and rows.count(b"\n") == c["truth_entries"]
    assert taxa == _taxeval.taxa_rows(taxid, m.tree.rank, true, called, both) and b"\n2157\t" not in taxa and b"\n131567\tno_rank\t0\t" in taxa
    assert b"NA" not in report.split(b"#A\t")[1]
    # the truth alone against itself as a classifier would print it: every read right at every rank its genome has
    perfect = b"".join(call(int(ln.split(b"\t")[0]), dict(GENOMES)[ln.split(b"\t")[2].decode()]) for ln in _taxeval.lines(truth) if not _taxeval.is_header(ln))
    (d / "perfect.txt").write_bytes(perfect)
    report, _, _ = outputs(d, d / "perfect.txt", reads=False, taxa=False)
    m = _taxeval.evaluate([truth], [perfect], taxonomy, GENOMES)
    assert report == _taxeval.report(*m.read(), m.tree.rank, m.taxa()[1], m.taxa()[2])
    assert b"P\t7\tspecies\t1.000000\t1.000000\t1.000000\t1.000000\t1.000000\t1.000000\n" in report and b"A\t7\tspecies\t2\t0.000000\n" in report


def test_refusals_name_their_flag(run):
    d = run
    (d / "bad_nodes.dmp").write_text("1\t|\t1\t|\tno rank\t|\n5\t|\t4\t|\tgenus\t|\n")
    (d / "bad_calls.txt").write_bytes(call(1, 562) + b"X\t2\t562\n")
    base = ["--eval-classified-truth", str(d / "truth.tsv"), "--eval-genome-taxa", str(d / "map.tsv"), "--eval-classified-report", str(d / "none.tsv")]
    for argv, word in ((["--eval-classified", str(d / "perfect.txt"), "--eval-taxonomy", str(d / "bad_nodes.dmp")], "--eval-taxonomy: "),
                       (["--eval-classified", str(d / "bad_calls.txt"), "--eval-taxonomy", str(d / "nodes.dmp")], "malformed candidate record"),
                       (["--eval-classified", str(d / "absent.txt"), "--eval-taxonomy", str(d / "nodes.dmp")], "--eval-classified: cannot open")):
        r = subprocess.run([str(EXE)] + argv + base, capture_output=True, text=True)
        assert r.returncode != 0 and word in r.stderr, r.stderr
        assert not (d / "none.tsv").exists()


@pytest.mark.parametrize("extra,given", [(["--num-reads", "5"], "--num-reads"), (["--devices", "0,1"], "--devices")])
def test_usage_errors(run, extra, given):
    d = run
    r = subprocess.run([str(EXE), "--eval-classified", "c.txt", "--eval-classified-truth", str(d / "truth.tsv"), "--eval-taxonomy", str(d / "nodes.dmp"),
                        "--eval-genome-taxa", str(d / "map.tsv"), "--eval-classified-report", str(d / "usage.tsv")] + extra, capture_output=True, text=True)
    assert r.returncode == 2 and r.stderr.startswith("error: --eval-classified runs no simulation: it takes only ") and f"('{given}' given)" in r.stderr.split("\n")[0]
    assert not (d / "usage.tsv").exists()
