"""`simmr-hip --truth FILE` on the GPU box: the FASTQ does not change, and the TSV is what the FASTQ's own headers
(positions, strand, sequence id) and the FASTA say — derived here without any of the truth pass's output."""
import re
import subprocess

import numpy as np
import pytest

from tests import _truth
from tests.test_gpu_cli import EXE, workdir  # noqa: F401  (the two-genome FASTA fixture and its default header format)

pytestmark = pytest.mark.gpu
HEAD = re.compile(rb"^@(\d+)\|([^/]+)/([12]) metadata:sid=(.*)\|sp=(\d+)\|ep=(\d+)\|rc=([tf])$")
HEADER = "read_id\tpair\tgenome_id\tsequence_id\tstart\tend\tstrand\tlength\tNM\tedits\n"


def tsv_from_fastq(oracle, fastq: bytes, contig_of, paired=True):
    comp = _truth.complement_lut(oracle)
    lines = fastq.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    out = [HEADER]
    for i in range(0, len(lines) - 1, 4):
        m = HEAD.match(lines[i])
        assert m, lines[i]
        rid, gid, pair, sid, sp, ep, rc = m.groups()
        sp, ep, rev = int(sp), int(ep), rc == b"t"
        seq, qual = np.frombuffer(lines[i + 1], dtype=np.uint8), np.frombuffer(lines[i + 3], dtype=np.uint8)
        lo, L = min(sp, ep), abs(ep - sp)
        assert seq.size == L == qual.size
        want = contig_of[(gid.decode(), sid.decode())][lo:lo + L]
        if rev:
            want = comp[want[::-1]]
        d = np.flatnonzero(seq != want)
        edits = ",".join("%d:%s>%s:%d" % (j, chr(want[j]), chr(seq[j]), int(qual[j]) - 33) for j in d) or "*"
        out.append("\t".join([rid.decode(), pair.decode() if paired else "0", gid.decode(), sid.decode(), str(sp), str(ep),
                              "-" if rev else "+", str(L), str(d.size), edits]) + "\n")
    return "".join(out)


@pytest.mark.parametrize("rng", ["reference", "philox"])
def test_cli_truth_tsv(workdir, oracle, rng):
    d, genomes = workdir
    contig_of = {(f"genome{gi}", names[i]): contigs[i] for gi, (contigs, names) in enumerate(genomes) for i in range(len(names))}
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "3001", "--seed", "42", "--error-profile", "minimal-short",
            "--rng", rng]  # (mean Phred 30, the default: by the oracle's law about one read in seven has no edit and half have several)
    plain, with_truth, chunked = d / f"plain_{rng}.fq", d / f"truth_{rng}.fq", d / f"chunk_{rng}.fq"
    subprocess.check_call([str(EXE), "--output", str(plain)] + argv)
    subprocess.check_call([str(EXE), "--output", str(with_truth), "--truth", str(d / f"t_{rng}.tsv")] + argv)
    fq = plain.read_bytes()
    assert with_truth.read_bytes() == fq and len(fq) > 100_000
    want = tsv_from_fastq(oracle, fq, contig_of)
    got = (d / f"t_{rng}.tsv").read_text()
    assert got.splitlines()[0] + "\n" == HEADER and got.count("\n") == 1 + fq.count(b"\n") // 4
    assert got == want
    assert any(line.endswith("\t*") for line in got.splitlines()) and any("," in line.split("\t")[-1] for line in got.splitlines())
    # the same TSV (and FASTQ) when the run is cut into several ranges
    subprocess.check_call([str(EXE), "--output", str(chunked), "--truth", str(d / f"tc_{rng}.tsv"), "--device-chunk-reads", "334"] + argv)
    assert chunked.read_bytes() == fq and (d / f"tc_{rng}.tsv").read_text() == want


def test_cli_truth_refuses_devices(workdir):
    d, _ = workdir
    r = subprocess.run([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "x.fq"), "--truth", str(d / "x.tsv"),
                        "--devices", "0,0"], capture_output=True)
    assert r.returncode == 1 and b"--truth does not combine with --devices" in r.stderr
