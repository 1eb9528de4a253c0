#!/usr/bin/env python3
"""Times the model-fitting pass (simmr_fit_add and simmr_fit_plan) next to the emit kernel of the same shard, in one process on
one device, for two shards: minimal-short 150 bp pairs (SIMMR_SLOT16, counter mode: the default bench workload) and
minimal-long reads (gamma 8000 / 6000).  The add is a HIP-event time (simmr_last_fit_ms), the plan a wall time around the call
(it synchronises), both the median of --steps repetitions after a warm-up.  Every step checks the model's identities against the
shard (observations, bases, windows).  Prints one JSON line; it gates nothing.

    python tools/fit_bench.py [--reads N] [--long-reads N] [--genome-bases N] [--k K] [--steps K] [--warmup W]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def time_shard(eng, reads, n_sets, k, capacity, steps, warmup):
    from simmr_amd import SimmrError
    add_ms, plan_ms, m, refused = [], [], None, None
    for step in range(warmup + steps):
        eng.fit_reset(k, 20, capacity)
        eng.fit_add(reads, n_sets)
        a = eng.last_fit_ms()
        t0 = time.perf_counter()
        try:
            m = eng.fit_model()  # plan + emit + the host's bincode image
        except SimmrError as err:  # (a quality above 93 in the shard: the add's time stands, there is no model to time)
            if step >= warmup:
                add_ms.append(a)
            refused = err.msg
            continue
        p = (time.perf_counter() - t0) * 1e3
        assert int(m["n_reads"]) == reads.n_reads == int(m["length_hist"].sum())
        assert int(m["qual_hist"].sum()) == int((m["length_hist"] * range(len(m["length_hist"]))).sum())
        if step >= warmup:
            add_ms.append(a); plan_ms.append(p)
    if m is None:
        return {"reads": reads.n_reads, "seq_bytes": reads.total_bases, "fit_add_ms": statistics.median(add_ms), "fit_add_ms_all": add_ms,
                "fit_model_refused": refused}
    return {"reads": reads.n_reads, "seq_bytes": reads.total_bases, "fit_add_ms": statistics.median(add_ms),
            "fit_model_wall_ms": statistics.median(plan_ms), "fit_add_ms_all": add_ms, "fit_model_wall_ms_all": plan_ms,
            "ref_kmers": int(m["n_ref_kmers"]), "pairs_kept": int(m["n_pairs"]), "positions": int(m["n_positions"]),
            "length_bins": int(m["n_length_bins"]), "insert_bins": int(m["n_insert_bins"]), "model_bytes": len(m["model_bytes"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--long-reads", type=int, default=200_000)
    ap.add_argument("--genome-bases", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=7)
    ap.add_argument("--pair-capacity", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()

    import torch
    from simmr_amd import MinimalLongErrorProfile, MinimalShortErrorProfile, _abi
    from simmr_amd.engine import Engine
    eng = Engine(0)
    eng.stage_synthetic(0, [args.genome_bases], 2)
    out = {"bench": "fit_pass", "k": args.k, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    eng.set_read_slots(16)
    reads = eng.simulate_pe_reads_from_genome(0, MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod(), args.reads, args.seed, qual_offset=33)
    out["short_pe_150"] = dict(time_shard(eng, reads, 2, args.k, args.pair_capacity, args.steps, args.warmup), emit_kernel_ms=eng.last_emit_kernel_ms())
    del reads
    lp = MinimalLongErrorProfile(gamma_mean=8000.0, gamma_std=6000.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    reads = eng.simulate_long_reads([0], [args.long_reads], lp, args.seed, qual_offset=33)
    out["long_gamma_8000_6000"] = dict(time_shard(eng, reads, 1, args.k, args.pair_capacity, args.steps, args.warmup), emit_kernel_ms=eng.last_emit_kernel_ms())
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
