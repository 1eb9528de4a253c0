"""`simmr-hip --eval-overlaps CANDIDATE --eval-overlaps-truth TRUTH --eval-overlaps-report OUT [--eval-overlaps-pairs FILE]
[--eval-overlaps-min-pct PCT]` on the GPU box: the truth is the file a long-read run wrote with --overlaps, the candidate a copy
perturbed on the host, and the report and the pair file must be, byte for byte, what the plain restatement of the rules
(tests/_ovleval.py) prints and what the Python path (Engine.overlap_eval) gives for the same input; a file of more than one piece."""
import re
import subprocess

import pytest

from simmr_amd.engine import Engine
from tests import _ovleval
from tests._ovleval import rec
from tests.test_gpu_overlap_cli import EXE, ROOT, run  # noqa: F401  (the two-genome FASTA fixture)

pytestmark = pytest.mark.gpu


def files_of_the_python_path(truth: bytes, cand: bytes, pct: int, pairs: bool = True):
    eng = Engine(0)
    try:
        ev = eng.overlap_eval(pct)
        ev.truth_add(truth)
        ev.truth_plan()
        ev.add(cand)
        return _ovleval.report(*ev.read()), _ovleval.pair_rows(*ev.pairs()) if pairs else None
    finally:
        eng.close()


def test_report_and_pairs_of_a_run(run):
    d = run
    truth_path, cand_path = d / "ove_truth.paf", d / "ove_cand.paf"
    subprocess.check_call([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "ove.fq"), "--num-reads", "400", "--seed", "5",
                           "--error-profile", "minimal-long", "--rng", "philox", "--gamma", "3000,2500", "--per-read-lengths", "--overlaps", str(truth_path),
                           "--min-overlap", "200", "--device-chunk-reads", "150"])
    truth = truth_path.read_bytes()
    n = len(_ovleval.lines(truth))
    assert n > 1000
    # the run against itself: every pair found once, nothing wrong
    report = d / "ove_self.tsv"
    r = subprocess.run([str(EXE), "--eval-overlaps", str(truth_path), "--eval-overlaps-truth", str(truth_path), "--eval-overlaps-report", str(report)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m = _ovleval.evaluate([truth], [truth])
    text = report.read_bytes()
    assert text == _ovleval.report(*m.read()) and b"#sensitivity\t1.000000\n#precision\t1.000000\n" in text
    assert f"#pairs_found\t{n}\n#pairs_wrong\t0\n#pairs_missed\t0\n#pairs_multiple\t0\n".encode() in text
    # a perturbed copy, its last line without the newline
    halved = []   # every seventeenth record once more with half its query interval: correct at 10 per cent, wrong at 60
    for ln in _ovleval.lines(truth)[::17]:
        f = ln.split(b"\t")
        f[3] = str(int(f[2]) + (int(f[3]) - int(f[2])) // 2).encode()
        halved.append(b"\t".join(f) + b"\n")
    cand = (_ovleval.derive(truth, outside_id=10 ** 9) + b"".join(halved)).rstrip(b"\n")
    cand_path.write_bytes(cand)
    for pct, extra in ((10, []), (60, ["--eval-overlaps-min-pct", "60"])):
        report, pairs = d / f"ove_report{pct}.tsv", d / f"ove_pairs{pct}.tsv"
        pairs.write_text("an older file\n")
        r = subprocess.run([str(EXE), "--eval-overlaps", str(cand_path), "--eval-overlaps-truth", str(truth_path), "--eval-overlaps-report", str(report),
                            "--eval-overlaps-pairs", str(pairs)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        m = _ovleval.evaluate([truth], [cand], pct)
        want = _ovleval.report(*m.read()), _ovleval.pair_rows(*m.pairs())
        assert (report.read_bytes(), pairs.read_bytes()) == want == files_of_the_python_path(truth, cand, pct)
        assert want[1].count(b"\n") == n and want[0].count(b"\nL\t") >= 3 and b"#sensitivity\t0." in want[0] and b"#precision\t0." in want[0]
    assert (d / "ove_report10.tsv").read_bytes() != (d / "ove_report60.tsv").read_bytes()
    # a malformed record in either file ends the run and writes nothing
    bad = d / "ove_bad.paf"
    bad.write_bytes(cand + b"\n" + rec(1, 10, 0, 11, "+", 2, 10, 0, 10))
    for argv, side in ((["--eval-overlaps", str(bad), "--eval-overlaps-truth", str(truth_path)], "candidate"),
                       (["--eval-overlaps", str(cand_path), "--eval-overlaps-truth", str(bad)], "truth")):
        r = subprocess.run([str(EXE)] + argv + ["--eval-overlaps-report", str(d / "ove_bad.tsv"), "--eval-overlaps-pairs", str(d / "ove_bad_pairs.tsv")],
                           capture_output=True, text=True)
        assert r.returncode == 1 and f"malformed {side} record" in r.stderr and not (d / "ove_bad.tsv").exists() and not (d / "ove_bad_pairs.tsv").exists()


def test_refusals(run):
    d = run
    (d / "ove_ok.paf").write_bytes(rec(1, 10, 0, 10, "+", 2, 10, 0, 10))
    (d / "ove_twice.paf").write_bytes(rec(1, 10, 0, 10, "+", 2, 10, 0, 10) + rec(2, 10, 0, 10, "+", 1, 10, 0, 10))
    report, pairs = d / "ove_r.tsv", d / "ove_r_pairs.tsv"
    base = [str(EXE), "--eval-overlaps", str(d / "ove_ok.paf"), "--eval-overlaps-report", str(report), "--eval-overlaps-pairs", str(pairs)]
    for extra in (["--num-reads", "5"], ["--genome", str(d / "g0.fna")], ["--overlaps", str(d / "x.paf")], ["--devices", "0,0"]):
        r = subprocess.run(base + ["--eval-overlaps-truth", str(d / "ove_ok.paf")] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "--eval-overlaps runs no simulation" in r.stderr and f"'{extra[0]}' given" in r.stderr
        assert not report.exists() and not pairs.exists()
    r = subprocess.run(base + ["--eval-overlaps-truth", str(d / "none.paf")], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open" in r.stderr and not report.exists()
    r = subprocess.run(base + ["--eval-overlaps-truth", str(d / "ove_twice.paf")], capture_output=True, text=True)
    assert r.returncode == 1 and "one pair" in r.stderr and not report.exists() and not pairs.exists()
    r = subprocess.run(base + ["--eval-overlaps-truth", str(d / "ove_ok.paf")], capture_output=True, text=True)
    assert r.returncode == 0 and report.read_bytes().endswith(b"#sensitivity\t1.000000\n#precision\t1.000000\nL\t4\t1\t0\n") and pairs.read_bytes() == b"1\t2\t10\t3\t1\n"


def test_a_file_of_more_than_one_piece(run):
    """The file walker's carry (PieceReader): a file just over FILE_PIECE whose cut falls inside a line, against itself, so the truth's
    and the candidate's walk both carry an open line over; then the same file without its last newline.  The tables are those of
    the Python path, which takes the text in one add."""
    d = run
    piece = re.search(r"FILE_PIECE = (\d+)u? << (\d+)", (ROOT / "simmr_amd" / "host" / "simmr_host.hpp").read_text())
    piece = int(piece.group(1)) << int(piece.group(2))
    width = len(rec(1_000_000, 5000, 1000, 3000, "+", 1_000_001, 5000, 1000, 3000, tail=(2000, 2000, 255)))
    n = piece // width + 3000
    text = b"".join(b"%d\t5000\t%d\t%d\t%s\t%d\t5000\t1000\t3000\t2000\t2000\t255\n" % (1_000_000 + i, 1000 + i % 1000, 3000 + i % 1000, b"+-"[i % 3 == 0:][:1], 1_000_001 + i)
                    for i in range(n))
    assert len(text) == n * width > piece and piece % width != 0 and text[piece - 1:piece] != b"\n"
    want, _ = files_of_the_python_path(text, text, 10, pairs=False)
    assert f"#truth_entries\t{n}\n#truth_reads\t{n + 1}\n#lines\t{n}\n#records\t{n}\n".encode() in want and f"#correct\t{n}\n#wrong\t0\n#pairs_found\t{n}\n".encode() in want
    for name, body in (("ove_two_pieces.paf", text), ("ove_two_pieces_open.paf", text[:-1])):
        path, report = d / name, d / (name + ".tsv")
        path.write_bytes(body)
        r = subprocess.run([str(EXE), "--eval-overlaps", str(path), "--eval-overlaps-truth", str(path), "--eval-overlaps-report", str(report)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert report.read_bytes() == want, name
        path.unlink()
