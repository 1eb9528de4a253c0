"""`simmr-hip --eval-vcf CALLS --eval-vcf-truth TRUTH --eval-vcf-report OUT [--eval-vcf-sites FILE] [--eval-vcf-filtered]` on the GPU
box: the truth is the file a run on tests/golden/sample.fna wrote with --with-ani 95 --strain-vcf; scored against itself every
site is found; a candidate derived here on the host has counts that are known from how it was made, and the report and the site
rows must be, byte for byte, what the plain restatement of the rules (tests/_vcfeval.py) prints; the usage errors."""
import subprocess
from pathlib import Path

import pytest

from tests import _vcfeval
from tests._vcfeval import rec

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "simmr_amd" / "host" / "simmr-hip"
SAMPLE = ROOT / "tests" / "golden" / "sample.fna"


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "simmr_amd" / "host")])
    d = tmp_path_factory.mktemp("vcfeval_cli")
    (d / "genomes.tsv").write_text("path\tid\n" + f"{SAMPLE}\tgenomeA\n{SAMPLE}\tgenomeB\n")   # (two contigs of 160 bases, twice)
    subprocess.check_call([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "reads.fq"), "--num-reads", "600", "--seed", "11",
                           "--error-profile", "perfect-short", "--read-length", "20", "--insert-size", "20", "--with-ani", "95", "--strain-vcf", str(d / "truth.vcf")])
    return d


def evaluate(d, calls: Path, extra=(), sites=True):
    report, rows = d / (calls.name + ".report.tsv"), d / (calls.name + ".sites.tsv")
    r = subprocess.run([str(EXE), "--eval-vcf", str(calls), "--eval-vcf-truth", str(d / "truth.vcf"), "--eval-vcf-report", str(report)]
                       + (["--eval-vcf-sites", str(rows)] if sites else []) + list(extra), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return report.read_bytes(), rows.read_bytes() if sites else None


def test_the_truth_as_the_calls(run):
    d = run
    truth = (d / "truth.vcf").read_bytes()
    names = _vcfeval.contig_names(truth)
    n = sum(1 for ln in _vcfeval.lines(truth) if ln[:1] != b"#")
    assert len(names) == 4 and n >= 12
    m = _vcfeval.evaluate([truth], [truth], names)
    report, rows = evaluate(d, d / "truth.vcf")
    assert report == _vcfeval.report(*m.read()) and rows == _vcfeval.site_rows(sorted(names), *m.sites())
    assert f"#calls\t{n}\n".encode() in report and f"#correct\t{n}\n#wrong\t0\n#sites_found\t{n}\n#sites_wrong\t0\n#sites_missed\t0\n#sites_multiple\t0\n".encode() in report
    assert f"#precision\t{n}/{n}\t100.0000\n#recall\t{n}/{n}\t100.0000\nQ\t0\t{n}\t0\t".encode() in report and rows.count(b"\n") == n
    # the by_ad rows are the ones the truth's AD implies
    by = {}
    for ln in _vcfeval.lines(truth):
        if ln[:1] != b"#":
            ad = int(dict(item.split(b"=") for item in ln.split(b"\t")[7].split(b";"))[b"AD"].split(b",")[1])
            by[ad.bit_length()] = by.get(ad.bit_length(), 0) + 1
    assert len(by) >= 1 and [ln for ln in report.split(b"\n") if ln[:3] == b"AD\t"] == [b"AD\t%d\t%d\t0" % (b, by[b]) for b in sorted(by)]


def test_a_derived_candidate_with_known_counts(run):
    d = run
    truth = (d / "truth.vcf").read_bytes()
    names = _vcfeval.contig_names(truth)
    records = [ln for ln in _vcfeval.lines(truth) if ln[:1] != b"#"]
    n = len(records)
    first = records[0].split(b"\t")
    taken = {int(ln.split(b"\t")[1]) for ln in records if ln.split(b"\t")[0] == first[0]}
    free = [p for p in range(1, 161) if p not in taken and p - 1 not in taken][:3]   # three spurious sites of the test's own
    cand = (b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n" + _vcfeval.derive(truth, b"chrX")
            + b"".join(rec(first[0], p, "A", "C", qual="3.7e1") for p in free)
            + rec(first[0], first[1], first[3] + b"A", first[3], qual=50)                        # one indel
            + rec(first[0], first[1], first[3], first[4], qual=60, filt="LowQual")).rstrip(b"\n")   # one filtered record; no newline at the end
    (d / "cand.vcf").write_bytes(cand)
    m = _vcfeval.evaluate([truth], [cand], names)
    c = m.read()[0]
    dropped, other = n // 3, len([i for i in range(n) if i % 5 == 4 and i % 3 != 2])
    spurious = c["no_site"]
    assert (c["sites_missed"], c["wrong_allele"], c["sites_wrong"], c["unknown_contig"], c["indel"], c["filtered"]) == (dropped, other, other, 1, 1, 1)
    assert len(free) == 3 <= spurious <= 3 + len([i for i in range(n) if i % 7 == 6 and i % 3 != 2]) and c["correct"] == c["sites_found"] == n - dropped - other
    assert c["calls"] == n - dropped + spurious + 1 and c["qual_missing"] > 0 and c["sites_multiple"] == 0
    report, rows = evaluate(d, d / "cand.vcf")
    assert report == _vcfeval.report(*m.read()) and rows == _vcfeval.site_rows(sorted(names), *m.sites())
    assert report.count(b"\nQ\t") >= 4 and b"\nQ\t37\t" in report and report.count(b"\nAD\t") >= 1 and rows.count(b"\n") == n
    # with the filtered record: one more call, and the first site called twice
    m = _vcfeval.evaluate([truth], [cand], names, use_filtered=True)
    report, _ = evaluate(d, d / "cand.vcf", ["--eval-vcf-filtered"], sites=False)
    assert report == _vcfeval.report(*m.read()) and b"#filtered\t0\n" in report and b"#sites_multiple\t1\n" in report
    # a malformed record in either file ends the run and writes nothing
    (d / "bad.vcf").write_bytes(cand + b"\n" + rec(first[0], 0, "A", "T"))
    for argv, side in ((["--eval-vcf", str(d / "bad.vcf"), "--eval-vcf-truth", str(d / "truth.vcf")], "candidate"),
                       (["--eval-vcf", str(d / "cand.vcf"), "--eval-vcf-truth", str(d / "bad.vcf")], "truth")):
        r = subprocess.run([str(EXE)] + argv + ["--eval-vcf-report", str(d / "bad.tsv"), "--eval-vcf-sites", str(d / "bad_sites.tsv")], capture_output=True, text=True)
        if side == "truth":   # (the candidate has no ##contig lines: the names are asked for first)
            assert r.returncode == 1 and "##contig" in r.stderr
        else:
            assert r.returncode == 1 and f"malformed {side} record" in r.stderr
        assert not (d / "bad.tsv").exists() and not (d / "bad_sites.tsv").exists()
    (d / "bad_truth.vcf").write_bytes(truth + rec(first[0], 0, "A", "T"))
    r = subprocess.run([str(EXE), "--eval-vcf", str(d / "cand.vcf"), "--eval-vcf-truth", str(d / "bad_truth.vcf"), "--eval-vcf-report", str(d / "bad.tsv")],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "malformed truth record" in r.stderr and not (d / "bad.tsv").exists()


def test_refusals(run):
    d = run
    report, rows = d / "r.tsv", d / "r_sites.tsv"
    base = [str(EXE), "--eval-vcf", str(d / "truth.vcf"), "--eval-vcf-report", str(report), "--eval-vcf-sites", str(rows)]
    for extra in (["--devices", "0,0"], ["--num-reads", "5"], ["--genome", str(SAMPLE)], ["--strain-vcf", str(d / "x.vcf")], ["--with-ani", "95"]):
        r = subprocess.run(base + ["--eval-vcf-truth", str(d / "truth.vcf")] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "--eval-vcf runs no simulation" in r.stderr and f"'{extra[0]}' given" in r.stderr
        assert not report.exists() and not rows.exists()
    (d / "no_contig.vcf").write_bytes(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + rec("c", 5, "A", "T"))
    r = subprocess.run(base + ["--eval-vcf-truth", str(d / "no_contig.vcf")], capture_output=True, text=True)
    assert r.returncode == 1 and "has no ##contig=<ID=...> lines" in r.stderr and not report.exists()
    r = subprocess.run(base + ["--eval-vcf-truth", str(d / "none.vcf")], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open" in r.stderr and not report.exists()
    r = subprocess.run([str(EXE), "--eval-vcf", str(d / "none.vcf"), "--eval-vcf-truth", str(d / "truth.vcf"), "--eval-vcf-report", str(report)], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open" in r.stderr and not report.exists()
    (d / "twice.vcf").write_bytes(b"##contig=<ID=c,length=9>\n" + rec("c", 5, "A", "T") + rec("c", 5, "A", "G"))
    r = subprocess.run(base + ["--eval-vcf-truth", str(d / "twice.vcf")], capture_output=True, text=True)
    assert r.returncode == 1 and "one position" in r.stderr and not report.exists() and not rows.exists()
