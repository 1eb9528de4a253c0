"""`simmr-hip --depth FILE --depth-track FILE` on the GPU box: the FASTQ does not change, and the two TSVs are the Python
formatter's text (tests/_depth.py) of the numpy model applied to the ORACLE's columns of the same run."""
import subprocess

import numpy as np
import pytest

from simmr_amd import MinimalShortErrorProfile
from tests import _depth, _oracle
from tests.test_gpu_cli import EXE, workdir  # noqa: F401  (the two-genome FASTA fixture)

pytestmark = pytest.mark.gpu


def test_cli_depth_tsvs(workdir, oracle):
    d, genomes = workdir
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "3001", "--seed", "42", "--error-profile", "minimal-short"]
    plain, with_depth, all_opts = d / "plain_d.fq", d / "depth.fq", d / "depth_all.fq"
    subprocess.check_call([str(EXE), "--output", str(plain)] + argv)
    subprocess.check_call([str(EXE), "--output", str(with_depth), "--depth", str(d / "d.tsv"), "--depth-track", str(d / "t.tsv"),
                           "--depth-window", "777"] + argv)
    fq = plain.read_bytes()
    assert with_depth.read_bytes() == fq and len(fq) > 100_000
    # the run's columns from the oracle (tests/test_gpu_cli.py::test_cli_pe_fastq_bytes shows the FASTQ is theirs): 1501
    # reads of each genome with the run's seed, sequences of at most 450 bases dropped (main.rs:117-162)
    cols, lens, names = [], {}, {}
    for gi, (contigs, ids) in enumerate(genomes):
        keep = [i for i, c in enumerate(contigs) if c.size > 450]
        o = _oracle.simulate_pe(oracle, _oracle.HostGenome([contigs[i] for i in keep]), MinimalShortErrorProfile().pod(), 1501, 42, qual_offset=33).trimmed()
        cols.append(dict(o, genome=np.full(len(o["start"]), gi, dtype=np.uint32)))
        lens[gi] = [int(contigs[i].size) for i in keep]
        names[gi] = (f"genome{gi}", [ids[i] for i in keep])
    cols = {k: np.concatenate([c[k] for c in cols]) for k in ("start", "end", "contig", "genome")}
    want = _depth.depth(cols, lens)
    s = _depth.summary(want, lens, 777)
    assert (d / "d.tsv").read_text() == _depth.tsv(s, names)
    assert (d / "t.tsv").read_text() == _depth.track_tsv(s, names, 777)
    lines = fq.split(b"\n")
    assert int(s["depth_sum"].sum()) == sum(len(x) for x in lines[1::4]) and len(s["genome"]) == 3 and s["covered"].all()
    # several ranges, together with --truth and --stats, the default window: the same FASTQ and the same rows
    subprocess.check_call([str(EXE), "--output", str(all_opts), "--depth", str(d / "d2.tsv"), "--depth-track", str(d / "t2.tsv"),
                           "--truth", str(d / "d_truth.tsv"), "--stats", str(d / "d_stats.tsv"), "--device-chunk-reads", "334"] + argv)
    assert all_opts.read_bytes() == fq and (d / "d2.tsv").read_text() == _depth.tsv(s, names)
    assert (d / "t2.tsv").read_text() == _depth.track_tsv(_depth.summary(want, lens, 1000), names, 1000)
    assert len((d / "d_truth.tsv").read_text().splitlines()) == 3001 and (d / "d_stats.tsv").read_text().startswith("table\t")
    # --depth-track alone
    subprocess.check_call([str(EXE), "--output", str(d / "depth_t.fq"), "--depth-track", str(d / "t3.tsv"), "--depth-window", "777"] + argv)
    assert (d / "t3.tsv").read_text() == (d / "t.tsv").read_text()


def test_cli_depth_refuses_devices(workdir):
    d, _ = workdir
    r = subprocess.run([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "z.fq"), "--depth", str(d / "z.tsv"),
                        "--devices", "0,0"], capture_output=True)
    assert r.returncode == 1 and b"--depth does not combine with --devices" in r.stderr
