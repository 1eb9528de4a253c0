"""`simmr-hip --fit-model FILE [--fit-k K] [--fit-max-alt N]` on the GPU box: the FASTQ does not change, and the file is, byte for
byte, `model_bytes` of Engine.fit_model() over the same run made through the Python host — in one range and in several."""
import subprocess

import pytest

from simmr_amd import CustomShortErrorProfile, MinimalShortErrorProfile
from tests.test_gpu_cli import EXE, workdir  # noqa: F401  (the two-genome FASTA fixture)

pytestmark = pytest.mark.gpu


def test_cli_fit_model_is_the_engines(workdir):
    from simmr_amd.engine import Engine
    d, genomes = workdir
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "3001", "--seed", "42", "--error-profile", "minimal-short"]
    plain, with_fit, chunked = d / "plain_f.fq", d / "fit.fq", d / "fit_chunked.fq"
    subprocess.check_call([str(EXE), "--output", str(plain)] + argv)
    subprocess.check_call([str(EXE), "--output", str(with_fit), "--fit-model", str(d / "m.bin")] + argv)
    fq = plain.read_bytes()
    assert with_fit.read_bytes() == fq and len(fq) > 100_000
    # the same run through the Python host (tests/test_gpu_stats_cli.py): 1501 reads of each genome with the run's seed
    eng = Engine(0)
    try:
        def model(k, max_alt):
            eng.fit_reset(k, max_alt, 1 << 16)
            for gi, (contigs, _) in enumerate(genomes):
                eng.stage_genome(gi, [c for c in contigs if c.size > 450])
                eng.fit_add(eng.simulate_pe_reads_from_genome(gi, MinimalShortErrorProfile().pod(), 1501, 42, qual_offset=33), 2)
            return eng.fit_model()
        want, want5 = model(7, 20), model(5, 3)
    finally:
        eng.close()
    assert (d / "m.bin").read_bytes() == want["model_bytes"]
    assert want["n_reads"] == 3000 and want["n_pairs"] > want["n_ref_kmers"] > 1000 and want["n_insert_bins"] > 0
    CustomShortErrorProfile(want["model_bytes"]).pod()  # (the loader takes it)
    # several ranges (at least nine of them), together with --stats; and the two options
    subprocess.check_call([str(EXE), "--output", str(chunked), "--fit-model", str(d / "mc.bin"), "--stats", str(d / "mc.tsv"),
                           "--device-chunk-reads", "334"] + argv)
    assert chunked.read_bytes() == fq and (d / "mc.bin").read_bytes() == want["model_bytes"]
    subprocess.check_call([str(EXE), "--output", str(chunked), "--fit-model", str(d / "m5.bin"), "--fit-k", "5", "--fit-max-alt", "3",
                           "--device-chunk-reads", "1000"] + argv)
    assert (d / "m5.bin").read_bytes() == want5["model_bytes"] != want["model_bytes"]


def test_cli_fit_model_refusals(workdir):
    d, _ = workdir
    base = [str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "y.fq"), "--fit-model", str(d / "y.bin")]
    r = subprocess.run(base + ["--devices", "0,0"], capture_output=True)
    assert r.returncode == 1 and b"--fit-model does not combine with --devices" in r.stderr
    for k in ("2", "11"):
        r = subprocess.run(base + ["--fit-k", k], capture_output=True)
        assert r.returncode != 0 and b"--fit-k" in r.stderr
