"""`simmr-hip --stats FILE` on the GPU box: the FASTQ does not change, and the TSV is the Python formatter's text
(tests/_stats.tsv) of Engine.stats() over the same run made through the Python host."""
import subprocess

import numpy as np
import pytest

from simmr_amd import MinimalShortErrorProfile
from tests import _stats
from tests.test_gpu_cli import EXE, workdir  # noqa: F401  (the two-genome FASTA fixture)

pytestmark = pytest.mark.gpu


def test_cli_stats_tsv(workdir):
    from simmr_amd.engine import Engine
    d, genomes = workdir
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "3001", "--seed", "42", "--error-profile", "minimal-short"]
    plain, with_stats, chunked = d / "plain_s.fq", d / "stats.fq", d / "stats_chunked.fq"
    subprocess.check_call([str(EXE), "--output", str(plain)] + argv)
    subprocess.check_call([str(EXE), "--output", str(with_stats), "--stats", str(d / "s.tsv")] + argv)
    fq = plain.read_bytes()
    assert with_stats.read_bytes() == fq and len(fq) > 100_000
    # the same run through the Python host: 1501 reads of each genome with the run's seed (uniform abundances,
    # tests/test_gpu_cli.py::test_cli_pe_fastq_bytes), sequences of at most 450 bases dropped (main.rs:117-162)
    eng = Engine(0)
    try:
        eng.stats_reset()
        for gi, (contigs, _) in enumerate(genomes):
            eng.stage_genome(gi, [c for c in contigs if c.size > 450])
            eng.stats_add(eng.simulate_pe_reads_from_genome(gi, MinimalShortErrorProfile().pod(), 1501, 42, qual_offset=33), 2)
        st = eng.stats()
    finally:
        eng.close()
    want = _stats.tsv(st)
    got = (d / "s.tsv").read_text()
    assert got == want
    lines = fq.split(b"\n")
    assert int(st["bases"].sum()) == sum(len(s) for s in lines[1::4]) and int(st["reads"].sum()) == len(lines) // 4 == 3000
    assert int(st["qual_n"].sum()) == int(st["bases"].sum()) and st["qual_mismatch"].sum() > 0 and st["pair"][:, 4].sum() > 0
    # several ranges, together with --truth: the same FASTQ and the same tables, and NM of the truth TSV sums to the edits
    subprocess.check_call([str(EXE), "--output", str(chunked), "--stats", str(d / "sc.tsv"), "--truth", str(d / "sc_truth.tsv"),
                           "--device-chunk-reads", "334"] + argv)
    assert chunked.read_bytes() == fq and (d / "sc.tsv").read_text() == want
    nm = [int(line.split("\t")[8]) for line in (d / "sc_truth.tsv").read_text().splitlines()[1:]]
    assert len(nm) == 3000 and sum(nm) == int(st["qual_mismatch"].sum())
    assert np.array_equal(np.bincount(np.minimum(nm, 63), minlength=64).astype(np.uint64), st["nm_hist"])


def test_cli_stats_refuses_devices(workdir):
    d, _ = workdir
    r = subprocess.run([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "y.fq"), "--stats", str(d / "y.tsv"),
                        "--devices", "0,0"], capture_output=True)
    assert r.returncode == 1 and b"--stats does not combine with --devices" in r.stderr
