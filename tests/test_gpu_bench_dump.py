"""bench.py --dump-outputs on the device: a small run of the default command (full counter mode, 16-byte read slots, and
the compact layout) dumps the columns of every read of its last timed step and a sample of its bases, in the compact
form a caller receives, and that is the oracle's run."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["slot16", "compact"])
def test_bench_dump_is_the_oracle_run(tmp_path, oracle, layout):
    from simmr_amd import MinimalShortErrorProfile, _abi
    from tests import _oracle, _synth
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--reads", "20000", "--genome-bases", "300000",
                        "--steps", "2", "--warmup", "1", "--layout", layout, "--dump-outputs", str(tmp_path)],
                       cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    d = {f.stem: np.load(f) for f in tmp_path.iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    ora = _oracle.simulate_pe(oracle, _oracle.HostGenome(_synth.synthetic_contigs([300000], 2)),
                              MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod(), 20000, 42, qual_offset=33).trimmed()
    assert np.array_equal(d["read_index"], np.arange(20000))
    for col in ("start", "end", "contig", "genome", "read_id", "flags"):
        assert np.array_equal(d[col if col == "read_id" else "read_" + col], ora[col].astype(np.float64)), col
    assert np.array_equal(d["read_seq_off"], ora["seq_off"][:-1].astype(np.float64))
    # ~3 M bases: above the dump's 2 M positions, so a sample of them
    bi = d["base_index"].astype(np.int64)
    assert bi.size == 1 << 21 and np.all(np.diff(bi) > 0) and 0 <= bi[0] and bi[-1] < ora["seq"].size
    assert np.array_equal(d["seq"], ora["seq"][bi].astype(np.float32)) and np.array_equal(d["qual"], ora["qual"][bi].astype(np.float32))
    assert d["counters"][_abi.CNT_READS] == 20000 and d["counters"][_abi.CNT_BASES] == ora["seq"].size
