"""`python3 bench.py --gpus N` must start itself: without a launcher in front of it the script
starts its N ranks as child processes, rank 0 prints ONE JSON line with the fields the contract asks for, and the exit
code is the children's.  Run here on CPU: gloo, and an oracle-backed stand-in for the engine (tests/bench_stub/)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _run(extra, timeout=420):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    env["PYTHONPATH"] = str(ROOT / "tests" / "bench_stub") + os.pathsep + env.get("PYTHONPATH", "")
    env["SIMMR_BENCH_STUB"] = "1"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--backend", "gloo", "--rehearse-device", "0", "--reads", "6000",
           "--genome-bases", "300000", "--steps", "2", "--warmup", "1", "--no-other-mode", "--layout", "compact"] + extra
    return subprocess.run(cmd, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=timeout)


def _line(p):
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(600)
def test_gpus_2_in_plain_form_starts_its_own_ranks():
    r = _line(_run(["--gpus", "2", "--full"]))
    assert r["n_gpus"] == 2 and r["steps"] == 2 and r["warmup"] == 1 and r["scaling"] == "weak"
    assert r["config"]["world_size_seen"] == 2 and r["config"]["backend"].startswith("gloo")
    assert r["config"]["reads_per_gpu"] == 6000
    # the whole job's reads: both ranks' shards went through the all-reduce of the counters
    assert abs(r["value"] * r["ms_per_step"] * 1e-3 - 12000) < 1e-6 * 12000
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(r["roofline"])
    assert r["roofline"]["alg_bytes_per_launch"] > 0 and r["roofline"]["kernel_ms"] > 0
    cb = r["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and "sample" in cb
    assert "reference_toolchain" in r


@pytest.mark.timeout(600)
def test_long_read_line_carries_cpu_baseline():
    """BASELINE config 3's line (and any N): cpu_baseline from the oracle's simulate_long_reads, with the
    faithful-cost figure (the reference's per-read genome clones, simulate.rs:362-375) beside it."""
    r = _line(_run(["--gpus", "1", "--full", "--profile", "minimal-long", "--reads", "400", "--cpu-sample-long-reads", "200"]))
    assert r["n_gpus"] == 1 and r["config"]["world_size_seen"] == 1
    cb = r["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["faithful_cost"]["value"] > 0
    assert "simulate.rs:362-375" in cb["faithful_cost"]["sample"] and cb["single_thread_value"] > 0


def test_a_failing_rank_is_the_exit_code():
    p = _run(["--gpus", "2", "--layout", "slot16"], timeout=300)  # the stand-in refuses the slot layout
    assert p.returncode != 0
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]


def test_plain_run_times_the_headline_only():
    """a plain run times exactly --steps steps and prints the headline figure; the CPU baseline, the side lines and
    the toolchain probe are --full's"""
    r = _line(_run(["--gpus", "1", "--steps", "3", "--warmup", "2"]))
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(r)
    assert r["steps"] == 3 and r["warmup"] == 2 and r["metric"] == "simulated_reads_per_sec" and r["unit"] == "reads/s"
    assert abs(r["value"] * r["ms_per_step"] * 1e-3 - 6000) < 1e-6 * 6000
    assert not {"cpu_baseline", "reference_toolchain", "other_rng_mode", "through_fastq"} & set(r)


def test_dump_outputs_are_the_last_step_and_repeat(tmp_path):
    """--dump-outputs: the same files with the same numbers from two runs, float32 / float64 only, and (6000 reads are
    below the sample size: the whole shard) the columns the oracle computes for the same run"""
    import numpy as np
    from simmr_amd import MinimalShortErrorProfile, _abi
    from tests import _oracle, _synth
    for d in ("a", "b"):
        _line(_run(["--gpus", "1", "--dump-outputs", str(tmp_path / d)]))
    names = sorted(f.name for f in (tmp_path / "a").iterdir())
    assert names == sorted(f.name for f in (tmp_path / "b").iterdir()) and "seq.npy" in names
    got = {}
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
        got[name[:-4]] = a
    assert sum((tmp_path / "a" / n).stat().st_size for n in names) < 64 << 20
    ora = _oracle.simulate_pe(_oracle.load(), _oracle.HostGenome(_synth.synthetic_contigs([300000], 2)),
                              MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod(), 6000, 42, qual_offset=33).trimmed()
    assert np.array_equal(got["read_index"], np.arange(6000))
    for col in ("start", "end", "contig", "genome", "flags"):
        assert np.array_equal(got["read_" + col], ora[col].astype(np.float64)), col
    assert np.array_equal(got["read_seq_off"], ora["seq_off"][:-1].astype(np.float64))
    assert np.array_equal(got["read_length"], np.diff(ora["seq_off"].astype(np.float64)))
    assert np.array_equal(got["read_id"], ora["read_id"].astype(np.float64))
    assert np.array_equal(got["seq"], ora["seq"].astype(np.float32)) and np.array_equal(got["qual"], ora["qual"].astype(np.float32))
    assert got["counters"][_abi.CNT_READS] == 6000 and got["counters"][_abi.CNT_BASES] == ora["seq"].size
