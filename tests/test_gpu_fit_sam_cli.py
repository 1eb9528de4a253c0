"""`simmr-hip --fit-from-sam FILE --fit-model OUT [--fit-k K] [--fit-max-alt N] [--single-reads]` on the GPU box: the model fitted
from the SAM file a run wrote is, byte for byte, the model that run fitted from its own columns; the counts on stderr are the
file's; a simulation flag beside it is refused; the custom profiles load the file and run."""
import re
import subprocess

import pytest

from tests.test_gpu_cli import EXE, workdir  # noqa: F401  (the two-genome FASTA fixture)

pytestmark = pytest.mark.gpu


def counts_of(stderr: str):
    return {m.group(2): int(m.group(1)) for m in re.finditer(r"Skipped (\d+) alignments? (.*)", stderr)}


def test_model_from_the_runs_own_sam(workdir):
    d, _ = workdir
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "3001", "--seed", "42", "--error-profile", "minimal-short"]
    sam, m1, m2, m5 = d / "fs.sam", d / "fs_m1.bin", d / "fs_m2.bin", d / "fs_m5.bin"
    subprocess.check_call([str(EXE), "--output", str(d / "fs.fq"), "--sam", str(sam), "--fit-model", str(m1), "--device-chunk-reads", "1000"] + argv)
    m2.write_text("an older file\n")
    r = subprocess.run([str(EXE), "--fit-from-sam", str(sam), "--fit-model", str(m2)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert m1.read_bytes() == m2.read_bytes() and len(m2.read_bytes()) > 10_000
    # the counts are the file's
    lines = sam.read_bytes().splitlines()
    header = sum(1 for l in lines if l.startswith(b"@"))
    assert header >= 3 and len(lines) - header == 3000
    assert f"Read {len(lines)} lines: {header} header lines, 3000 alignments" in r.stderr
    assert "Using 3000 alignments (3000 for read lengths and qualities)" in r.stderr
    skipped = counts_of(r.stderr)
    assert len(skipped) == 10 and set(skipped.values()) == {0}, skipped
    # the options; unpaired: no insert sizes, another model
    r = subprocess.run([str(EXE), "--fit-from-sam", str(sam), "--fit-model", str(m5), "--fit-k", "5", "--fit-max-alt", "3", "--single-reads"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and m5.read_bytes() != m2.read_bytes(), r.stderr
    # a record the filters drop shows in the counts; a malformed one ends the run
    rec = next(l for l in lines if not l.startswith(b"@")).split(b"\t")
    extra = d / "fs_extra.sam"
    extra.write_bytes(sam.read_bytes() + b"\t".join([rec[0], rec[1], rec[2], rec[3], b"0"] + rec[5:]))  # MAPQ 0, no final newline
    r = subprocess.run([str(EXE), "--fit-from-sam", str(extra), "--fit-model", str(d / "fs_m3.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and counts_of(r.stderr)["with MAPQ == 0"] == 1 and "3001 alignments" in r.stderr, r.stderr
    extra.write_bytes(sam.read_bytes() + b"\t".join(rec[:10]) + b"\n")
    r = subprocess.run([str(EXE), "--fit-from-sam", str(extra), "--fit-model", str(d / "fs_m4.bin")], capture_output=True, text=True)
    assert r.returncode == 1 and "malformed" in r.stderr and not (d / "fs_m4.bin").exists()
    # the custom profiles load the model and run
    out = d / "fs_custom.fq"
    subprocess.check_call([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(out), "--num-reads", "500", "--seed", "7",
                           "--error-profile", "custom-short", "--custom-profile", str(m2)])
    assert out.read_bytes().count(b"\n") >= 4 * 400


def test_refusals(workdir):
    d, _ = workdir
    base = [str(EXE), "--fit-from-sam", str(d / "none.sam"), "--fit-model", str(d / "r.bin")]
    for extra in (["--num-reads", "5"], ["--genome", str(d / "g0.fna")], ["--output", str(d / "r.fq")], ["--sam", str(d / "r.sam")], ["--seed", "1"]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 2 and f"--fit-from-sam runs no simulation" in r.stderr and f"'{extra[0]}' given" in r.stderr
    r = subprocess.run(base + ["--devices", "0,0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--fit-from-sam does not combine with --devices" in r.stderr
    r = subprocess.run(base[:3], capture_output=True, text=True)
    assert r.returncode == 2 and "--fit-from-sam needs --fit-model" in r.stderr
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open" in r.stderr
    r = subprocess.run([str(EXE), "--genome", str(d / "g0.fna"), "--output", str(d / "r.fq"), "--single-reads"], capture_output=True, text=True)
    assert r.returncode == 2 and "--single-reads needs --fit-from-sam" in r.stderr
