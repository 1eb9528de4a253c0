"""`simmr-hip --eval-sam ALIGNED --eval-truth TRUTH --eval-report OUT [--eval-reads FILE] [--eval-min-overlap PCT]` on the GPU box: the
truth is the file a run wrote with --sam, the aligner's file a perturbed copy of it, and the report and the reads file must be, byte
for byte, what the plain restatement of the rules (tests/_mapeval.py) prints.  A truth file without @SQ lines and the mode mixed with
a flag of a run fail and write nothing."""
import subprocess

import pytest

from tests import _mapeval
from tests.test_gpu_cli import EXE, workdir  # noqa: F401  (the two-genome FASTA fixture)
from tests.test_gpu_mapeval import span_of

pytestmark = pytest.mark.gpu


def want_files(truth: bytes, aligned: bytes, pct: int):
    m = _mapeval.evaluate(_mapeval.sq_names(truth), [truth], [aligned], pct)
    return _mapeval.report(*m.read()), _mapeval.reads_file(*m.entries())


def test_report_and_reads_of_a_perturbed_copy(workdir):
    d, _ = workdir
    truth_path, aligned_path = d / "ev_truth.sam", d / "ev_aligned.sam"
    subprocess.check_call([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "ev.fq"), "--num-reads", "2001", "--seed", "42",
                           "--error-profile", "minimal-short", "--sam", str(truth_path), "--device-chunk-reads", "700"])
    truth = truth_path.read_bytes()
    names = _mapeval.sq_names(truth)
    assert len(names) >= 3 and len(_mapeval.lines(truth)) >= 2000
    plan = [("same", None), ("shift", 3), ("shift", lambda ln: _mapeval.threshold_shift(span_of(ln), 10) + 1), ("strand", None), ("contig", names[0]),
            ("shift", lambda ln: _mapeval.threshold_shift(span_of(ln), 10)),  # correct at 10 per cent, wrong at 60
            ("unmapped", None), ("drop", None), ("double", 20), ("secondary", None), ("mapq", 0), ("mapq", 37), ("cigar", lambda ln: f"5S{span_of(ln) - 5}M".encode()),
            ("qname", b"nobody"), ("contig", b"chrUn"), ("cigar", lambda ln: f"9M50N{span_of(ln) - 9}M".encode())]
    aligned = _mapeval.derive(truth, plan, seed=8).rstrip(b"\n")  # the last line without its newline
    aligned_path.write_bytes(aligned)
    for pct, extra in ((10, []), (60, ["--eval-min-overlap", "60"])):
        report, reads = d / f"ev_report{pct}.tsv", d / f"ev_reads{pct}.tsv"
        reads.write_text("an older file\n")
        r = subprocess.run([str(EXE), "--eval-sam", str(aligned_path), "--eval-truth", str(truth_path), "--eval-report", str(report),
                            "--eval-reads", str(reads)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        want_report, want_reads = want_files(truth, aligned, pct)
        assert report.read_bytes() == want_report and reads.read_bytes() == want_reads
        assert want_report.count(b"\nQ\t") >= 4 and want_reads.count(b"\n") > 500
    assert (d / "ev_report10.tsv").read_bytes() != (d / "ev_report60.tsv").read_bytes()
    # the truth against itself, without --eval-reads: every read correct at MAPQ 255
    report = d / "ev_self.tsv"
    r = subprocess.run([str(EXE), "--eval-sam", str(truth_path), "--eval-truth", str(truth_path), "--eval-report", str(report)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    n = len(_mapeval.lines(truth)) - truth.count(b"\n@") - 1
    assert report.read_bytes() == want_files(truth, truth, 10)[0] and report.read_bytes().endswith(f"Q\t255\t{n}\t0\t0\t{n}\n".encode())
    # a malformed record in the aligner's file ends the run and writes nothing
    bad = d / "ev_bad.sam"
    bad.write_bytes(aligned + b"\n7\t0\t" + names[0] + b"\t5\t60\t9M9\t*\t0\t0\t*\t*\n")
    r = subprocess.run([str(EXE), "--eval-sam", str(bad), "--eval-truth", str(truth_path), "--eval-report", str(d / "ev_bad.tsv")], capture_output=True, text=True)
    assert r.returncode == 1 and "malformed" in r.stderr and not (d / "ev_bad.tsv").exists()


def test_refusals(workdir):
    d, _ = workdir
    body = b"7\t0\tc0\t5\t255\t9M\t*\t0\t0\t*\t*\n"
    (d / "ev_nosq.sam").write_bytes(b"@HD\tVN:1.6\n" + body)
    (d / "ev_ok.sam").write_bytes(b"@SQ\tSN:c0\tLN:100\n" + body)
    report, reads = d / "ev_r.tsv", d / "ev_r_reads.tsv"
    base = [str(EXE), "--eval-sam", str(d / "ev_ok.sam"), "--eval-report", str(report), "--eval-reads", str(reads)]
    r = subprocess.run(base + ["--eval-truth", str(d / "ev_nosq.sam")], capture_output=True, text=True)
    assert r.returncode == 1 and "no @SQ lines" in r.stderr and not report.exists() and not reads.exists()
    for extra in (["--num-reads", "5"], ["--genome", str(d / "g0.fna")], ["--sam", str(d / "x.sam")], ["--devices", "0,0"]):
        r = subprocess.run(base + ["--eval-truth", str(d / "ev_ok.sam")] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "--eval-sam runs no simulation" in r.stderr and f"'{extra[0]}' given" in r.stderr
        assert not report.exists() and not reads.exists()
    r = subprocess.run(base + ["--eval-truth", str(d / "none.sam")], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open" in r.stderr and not report.exists()
    r = subprocess.run(base + ["--eval-truth", str(d / "ev_ok.sam")], capture_output=True, text=True)
    assert r.returncode == 0 and report.read_bytes().endswith(b"Q\t255\t1\t0\t0\t1\n") and reads.read_bytes() == b""


def test_a_file_of_more_than_one_piece(workdir):
    """The file walker's carry (PieceReader): a file just over FILE_PIECE whose cut falls inside a line, against itself, so the truth's
    and the aligner's walk both carry an open line over; then the same file without its last newline"""
    import re

    import numpy as np

    from tests import _seams
    from tests.test_gpu_cli import ROOT
    d, _ = workdir
    piece = re.search(r"FILE_PIECE = (\d+)u? << (\d+)", (ROOT / "simmr_amd" / "host" / "simmr_host.hpp").read_text())
    piece = int(piece.group(1)) << int(piece.group(2))
    header = b"@HD\tVN:1.6\n@SQ\tSN:a\tLN:100000\n@SQ\tSN:b\tLN:100000\n@SQ\tSN:c\tLN:100000\n"
    width = 38  # 7 + 3 + 1 + 4 + 3 + 4 bytes of fields, 16 of tabs, the fixed fields and the newline
    n = (piece - len(header)) // width + 3000
    i = np.arange(n, dtype=np.int64)
    cols = dict(id=(i * 1_000_003) % n, mate=1 + (i & 1), strand=(i >> 1) & 1, row=i % 3, pos=1 + i % 9000, span=100 + i % 100, mapq=i % 256)
    res = _seams.mapeval_from_columns([b"a", b"b", b"c"], cols, dict(cols, bits=0), header=header)
    text = res["truth"]
    assert text == res["aligned"] and len(text) == len(header) + n * width > piece and (piece - len(header)) % width != 0
    assert text[len(header) + width - 1:len(header) + width] == b"\n" and text[piece - 1:piece] != b"\n"  # lines of one width; the cut is inside one
    want = _mapeval.report(res["counts"], res["by_mapq"])
    assert res["counts"]["correct"] == res["counts"]["reads_correct"] == n and want.count(b"\nQ\t") == 256
    for name, body in (("ev_two_pieces.sam", text), ("ev_two_pieces_open.sam", text[:-1])):
        path, report = d / name, d / (name + ".tsv")
        path.write_bytes(body)
        r = subprocess.run([str(EXE), "--eval-sam", str(path), "--eval-truth", str(path), "--eval-report", str(report)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert report.read_bytes() == want, name
        path.unlink()
