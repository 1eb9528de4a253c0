"""`simmr-hip --with-ani N --strain-sites FILE` on the GPU box: the site list is the numpy model's (tests/_strain.py) under
the command line's seed rule, a perfect-short run's reads are the diverged sequences at their coordinates, several engines
write the same bytes, and 100 percent changes nothing."""
import re
import subprocess

import numpy as np
import pytest

from tests import _strain
from tests.test_gpu_cli import EXE, ROOT

pytestmark = pytest.mark.gpu
SAMPLE = ROOT / "tests" / "golden" / "sample.fna"
COMPLEMENT = bytes.maketrans(b"ACGTN-", b"TGCAN-")
HEADER = re.compile(rb"@(\d+)\|(\S+)/([12]) metadata:sid=(.*)\|sp=(\d+)\|ep=(\d+)\|rc=([tf])$")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "simmr_amd" / "host")])
    d = tmp_path_factory.mktemp("strain_cli")
    (d / "genomes.tsv").write_text("path\tid\n" + f"{SAMPLE}\tgenomeA\n{SAMPLE}\tgenomeB\n")
    records = SAMPLE.read_text().split(">")[1:]
    ids = [r.split("\n", 1)[0] for r in records]
    contigs = [np.frombuffer("".join(r.split("\n")[1:]).encode(), dtype=np.uint8) for r in records]
    assert len(contigs) == 2 and all(c.size > 100 for c in contigs)
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "600", "--seed", "7", "--error-profile", "perfect-short",
            "--read-length", "20", "--insert-size", "20"]
    return d, ids, contigs, argv


def reads_of(fastq):
    lines = fastq.split(b"\n")
    for h, s in zip(lines[0::4], lines[1::4]):
        m = HEADER.match(h)
        assert m, h
        yield m.group(2).decode(), m.group(4).decode(), int(m.group(5)), int(m.group(6)), m.group(7) == b"t", s


def test_sites_and_reads_of_a_two_genome_run(run):
    d, ids, contigs, argv = run
    fq, tsv = d / "ani.fq", d / "sites.tsv"
    subprocess.check_call([str(EXE), "--output", str(fq), "--with-ani", "98.5", "--strain-sites", str(tsv)] + argv)
    want, strains, n_sites = _strain.TSV_HEADER, {}, 0
    for i, gid in enumerate(("genomeA", "genomeB")):
        diverged, cols = _strain.diverge(contigs, 98.5 / 100.0, _strain.genome_seed(7, i))
        want += _strain.tsv_rows(cols, gid, ids)
        strains[gid] = {sid: c.tobytes() for sid, c in zip(ids, diverged)}
        n_sites += cols["pos"].size
    assert tsv.read_text() == want and n_sites > 0
    assert strains["genomeA"] != strains["genomeB"]  # the same assembly twice: two strains of it
    n = 0
    for gid, sid, sp, ep, rc, seq in reads_of(fq.read_bytes()):
        lo, hi = min(sp, ep), max(sp, ep)
        expect = strains[gid][sid][lo:hi]
        assert seq == (expect.translate(COMPLEMENT)[::-1] if rc else expect), (gid, sid, sp, ep, rc)
        n += 1
    assert n == 600
    # several engines: every one stages and diverges its own copy, the sites are listed from the first
    fq2, tsv2 = d / "ani2.fq", d / "sites2.tsv"
    subprocess.check_call([str(EXE), "--output", str(fq2), "--with-ani", "98.5", "--strain-sites", str(tsv2), "--devices", "0,0",
                           "--device-chunk-reads", "100"] + argv)
    assert fq2.read_bytes() == fq.read_bytes() and tsv2.read_text() == want
    # the flag alone, and the run written over an older site list
    subprocess.check_call([str(EXE), "--output", str(d / "ani3.fq"), "--with-ani=98.5"] + argv)
    assert (d / "ani3.fq").read_bytes() == fq.read_bytes()


def test_full_identity_changes_nothing(run):
    d, ids, contigs, argv = run
    plain, full, tsv = d / "plain.fq", d / "full.fq", d / "none.tsv"
    tsv.write_text("an older file\n")
    subprocess.check_call([str(EXE), "--output", str(plain)] + argv)
    subprocess.check_call([str(EXE), "--output", str(full), "--with-ani", "100", "--strain-sites", str(tsv)] + argv)
    assert full.read_bytes() == plain.read_bytes() and len(plain.read_bytes()) > 20_000
    assert tsv.read_text() == _strain.TSV_HEADER


def test_side_outputs_see_the_strain(run):
    """--truth diffs the reads against the genome they were drawn from: a perfect-short run of a strain has no edits; --depth is
    laid out after the divergence and still adds up"""
    d, ids, contigs, argv = run
    subprocess.check_call([str(EXE), "--output", str(d / "side.fq"), "--with-ani", "90", "--truth", str(d / "truth.tsv"),
                           "--depth", str(d / "depth.tsv")] + argv)
    rows = (d / "truth.tsv").read_text().splitlines()[1:]
    assert len(rows) == 600 and all(r.split("\t")[8] == "0" for r in rows)
    assert len((d / "depth.tsv").read_text().splitlines()) == 1 + 4
