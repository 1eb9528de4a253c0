"""End-to-end on the GPU box: a small run of simmr-hip with --sam, its FASTQ "corrected" here in Python from the SAM, and
simmr-hip --eval-corrected over the two files: the report and the reads file equal what the plain model of tests/_correval.py and its
restatement of the formatter give, byte for byte."""
import random
import subprocess
from pathlib import Path

import pytest

from tests import _correval as M
from tests import _synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "simmr_amd" / "host" / "simmr-hip"


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "simmr_amd" / "host")])
    d = tmp_path_factory.mktemp("correval_cli")
    _synth.write_fasta(d / "g.fna", _synth.synthetic_contigs([60_000, 9_000], 31), ["chr1", "plasmid"])
    subprocess.check_call([str(EXE), "--genome", str(d / "g.fna"), "--output", str(d / "reads.fq"), "--num-reads", "400", "--seed", "17",
                           "--error-profile", "minimal-short", "--sam", str(d / "truth.sam"), "--read-header-format", "@{:read_id:}/{:pair:}"])
    truth = (d / "truth.sam").read_bytes()
    _, entries = M.truth_of([truth])
    lines = (d / "reads.fq").read_text().split("\n")
    assert lines[-1] == "" and len(lines) % 4 == 1 and len(entries) == len(lines) // 4 > 100
    rng = random.Random(23)
    out, n_changed = [], 0
    for k in range(len(lines) // 4):
        name, bases, plus, qual = lines[4 * k:4 * k + 4]
        e = entries[M.name_key(name[1:])]
        assert [M.base_class(ch) for ch in bases] == e["o"]   # the FASTQ is the read in its own orientation, the SAM's SEQ turned back
        if rng.random() < 0.04:
            continue                                         # dropped
        b = list(bases)
        for i, t in enumerate(e["t"]):
            if e["o"][i] != t and t < 4 and rng.random() < 0.7:
                b[i] = "acgt"[t]                             # fixed, in lower case
                n_changed += 1
            elif rng.random() < 0.004:
                b[i] = rng.choice("acgtn")                   # damaged (or, by chance, left as it was)
        if rng.random() < 0.1:
            b = b[:rng.randrange(len(b) + 1)]                # trimmed, some to nothing
        out.append("%s\n%s\n%s\n%s\n" % (name, "".join(b), plus, qual[:len(b)]))
    assert n_changed > 20
    (d / "corrected.fq").write_text("".join(out))
    return d, truth, "".join(out).encode()


def test_the_report_and_the_reads_file(run):
    d, truth, corrected = run
    r = subprocess.run([str(EXE), "--eval-corrected", str(d / "corrected.fq"), "--eval-corrected-truth", str(d / "truth.sam"), "--eval-corrected-report",
                        str(d / "report.tsv"), "--eval-corrected-reads", str(d / "reads.tsv")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    counts, cube, by_qual, by_pos, rows = M.score([truth], [corrected])
    assert counts["fixed"] > 20 and counts["damaged"] > 0 and counts["trimmed_records"] > 0 and counts["missing"] > 0 and counts["left"] > 0
    assert (d / "report.tsv").read_text() == M.report(counts, cube, by_qual, by_pos)
    assert (d / "reads.tsv").read_text() == M.read_rows(rows)
    assert "Wrote " + str(d / "report.tsv") in r.stderr + r.stdout


def test_two_line_fasta(run):
    d, truth, corrected = run
    lines = corrected.decode().split("\n")[:-1]
    fasta = "".join(">%s\n%s\n" % (lines[k][1:], lines[k + 1]) for k in range(0, len(lines), 4))
    (d / "corrected.fa").write_text(fasta)
    subprocess.check_call([str(EXE), "--eval-corrected", str(d / "corrected.fa"), "--eval-corrected-truth", str(d / "truth.sam"), "--eval-corrected-report",
                           str(d / "report_fa.tsv"), "--eval-corrected-fasta"])
    assert (d / "report_fa.tsv").read_text() == (d / "report.tsv").read_text().replace("#lines\t%d\n" % len(lines), "#lines\t%d\n" % (len(lines) // 2))


def test_refusals(run, tmp_path):
    d, _, _ = run
    base = ["--eval-corrected", str(d / "corrected.fq"), "--eval-corrected-truth", str(d / "truth.sam"), "--eval-corrected-report", str(tmp_path / "r.tsv")]
    r = subprocess.run([str(EXE)] + base + ["--devices", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and r.stderr.startswith("error: --eval-corrected runs no simulation")
    r = subprocess.run([str(EXE)] + base + ["--num-reads", "10"], capture_output=True, text=True)
    assert r.returncode == 2 and "'--num-reads' given" in r.stderr
    r = subprocess.run([str(EXE)] + base[:1] + [str(d / "nothing.fq")] + base[2:], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot open" in r.stderr
    # a FASTQ read as FASTA is malformed: its third line does not start with '>'
    r = subprocess.run([str(EXE)] + base + ["--eval-corrected-fasta"], capture_output=True, text=True)
    assert r.returncode != 0 and "malformed corrected text" in r.stderr
    assert not list(tmp_path.iterdir())  # nothing was written
