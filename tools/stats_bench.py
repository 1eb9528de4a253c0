#!/usr/bin/env python3
"""Times the run-statistics pass (simmr_stats_add alone) next to the emit kernel and the count half of the ground-truth
pass (k_truth<false> + scan, simmr_truth_plan) of the same shard, in one process on one device: BASELINE config 2 by
default (100 M reads of minimal-short 150 bp pairs, SIMMR_SLOT16, counter mode).

k_truth<false> reads the same seq[] bytes, columns and planes as k_read_stats, without qual[] and without tables: it is the
yardstick the statistics pass is reported against.  All three are HIP-event times (simmr_last_stats_ms,
simmr_last_emit_kernel_ms, simmr_last_truth_ms after a plan without an emit), taken after a warm-up, as the median of
--steps repetitions.  Every step also checks the tables' identities against the emit's own counters.  Prints one JSON line.

    python tools/stats_bench.py [--reads N] [--genome-bases N] [--steps K] [--warmup W] [--layout slot16|compact]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK = 8.0e12  # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--genome-bases", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--layout", default="slot16", choices=["slot16", "compact"])
    args = ap.parse_args()

    import torch
    from simmr_amd import MinimalShortErrorProfile, _abi
    from simmr_amd.engine import Engine
    eng = Engine(0)
    eng.stage_synthetic(0, [args.genome_bases], 2)
    eng.set_read_slots(16 if args.layout == "slot16" else 0)
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
    emit_ms, stats_ms, count_ms = [], [], []
    reads = st = None
    for step in range(args.warmup + args.steps):
        eng.counters_reset()
        if reads is None:
            reads = eng.simulate_pe_reads_from_genome(0, prof, args.reads, args.seed, qual_offset=33)
        else:
            eng.pe_plan(0, prof, args.reads, args.seed)
            eng.pe_emit(0, reads)
        e_ms = eng.last_emit_kernel_ms()
        cnt = eng.counters()
        eng.stats_reset()
        eng.stats_add(reads, 2)
        s_ms = eng.last_stats_ms()
        st = eng.stats()
        m = eng.truth_plan(reads)
        c_ms = eng.last_truth_ms()  # (no emit after this plan: count + scan alone)
        n, subs = reads.n_reads, int(cnt[_abi.CNT_SUBSTITUTIONS])
        assert int(st["qual_mismatch"].sum()) == int(st["cycle_mismatch"].sum()) == m == subs, (int(st["qual_mismatch"].sum()), m, subs)
        assert int(st["reads"].sum()) == n and int(st["bases"].sum()) == int(st["qual_n"].sum()) == int(st["pair"].sum())
        assert int(st["qual_mismatch"].sum()) == int(st["pair"].sum()) - int(st["pair"].trace())
        assert int((st["qual_n"] * range(256)).sum()) == int(st["cycle_qsum"].sum())
        if step >= args.warmup:
            emit_ms.append(e_ms); stats_ms.append(s_ms); count_ms.append(c_ms)
    n, tb = reads.n_reads, reads.total_bases
    # bytes the statistics kernel moves: seq[] and qual[] once, the columns it reads (seq_off, start, end 8 B; contig,
    # genome 4 B; flags 1 B); the planes' traffic is cache-resident and the tables' is negligible
    moved = 2 * tb + n * (8 + 8 + 8 + 4 + 4 + 1)
    t = statistics.median(stats_ms)
    print(json.dumps({
        "bench": "stats_pass", "reads": n, "seq_bytes": tb, "layout": args.layout, "steps": args.steps, "warmup": args.warmup,
        "stats_ms": t, "emit_kernel_ms": statistics.median(emit_ms), "truth_count_scan_ms": statistics.median(count_ms),
        "stats_ms_all": stats_ms, "emit_kernel_ms_all": emit_ms, "truth_count_scan_ms_all": count_ms,
        "stats_over_truth_count": t / statistics.median(count_ms),
        "stats_bytes_moved": moved, "stats_fraction_of_8TBps": moved / (t * 1e-3) / HBM_PEAK,
        "bases": int(st["bases"].sum()), "counter_bases": int(cnt[_abi.CNT_BASES]), "qual_sum": int(st["cycle_qsum"].sum()),
        "counter_qual_sum": int(cnt[_abi.CNT_QUAL_SUM]),
        "edits": int(st["qual_mismatch"].sum()), "mean_phred": float((st["qual_n"] * range(256)).sum() / st["qual_n"].sum()),
        "device": torch.cuda.get_device_name(0)}))
    eng.close()


if __name__ == "__main__":
    main()
