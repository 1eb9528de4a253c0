#!/usr/bin/env python3
"""Times the ground-truth pass (simmr_truth_plan + simmr_truth_emit) next to the emit of the same shard, in one process
on one device: BASELINE config 2 by default (100 M reads of minimal-short 150 bp pairs, SIMMR_SLOT16, counter mode).

The yardstick is the emit kernel's time of the same run (simmr_last_emit_kernel_ms); the truth pass's is
simmr_last_truth_ms (count + scan + column copies + write, HIP events).  Both are taken after a warm-up, as the median
of --steps repetitions.  Prints one JSON line.

    python tools/truth_bench.py [--reads N] [--genome-bases N] [--steps K] [--warmup W] [--layout slot16|compact]
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
    emit_ms, truth_ms, plan_only_ms = [], [], []
    reads = truth = None
    for step in range(args.warmup + args.steps):
        del truth
        eng.counters_reset()
        if reads is None:
            reads = eng.simulate_pe_reads_from_genome(0, prof, args.reads, args.seed, qual_offset=33)
        else:
            eng.pe_plan(0, prof, args.reads, args.seed)
            eng.pe_emit(0, reads)
        e_ms = eng.last_emit_kernel_ms()
        subs = int(eng.counters()[_abi.CNT_SUBSTITUTIONS])
        m = eng.truth_plan(reads)
        p_ms = eng.last_truth_ms()  # (no emit after this plan yet: count + scan alone)
        truth = eng.truth(reads)
        t_ms = eng.last_truth_ms()
        assert truth.n_edits == m == subs, (truth.n_edits, m, subs)
        if step >= args.warmup:
            emit_ms.append(e_ms); truth_ms.append(t_ms); plan_only_ms.append(p_ms)
    n, tb, m = reads.n_reads, reads.total_bases, truth.n_edits
    # bytes the two truth kernels move: seq[] twice, the columns they read (seq_off, start, end 8 B; contig, genome 4 B;
    # flags 1 B) twice, nm written and copied, edit_off written, read and copied, the edit columns (4 + 1 + 1 + 1 B) and
    # the quality bytes of the edits; the planes' traffic is cache-resident and not counted
    cols = n * (8 + 8 + 8 + 4 + 4 + 1)
    moved = 2 * tb + 2 * cols + n * 4 * 3 + n * 8 * 4 + m * (7 + 1)
    t = statistics.median(truth_ms)
    print(json.dumps({
        "bench": "truth_pass", "reads": n, "seq_bytes": tb, "n_edits": m, "layout": args.layout, "steps": args.steps, "warmup": args.warmup,
        "emit_kernel_ms": statistics.median(emit_ms), "truth_ms": t, "truth_count_scan_ms": statistics.median(plan_only_ms),
        "emit_kernel_ms_all": emit_ms, "truth_ms_all": truth_ms,
        "truth_bytes_moved": moved, "truth_fraction_of_8TBps": moved / (t * 1e-3) / HBM_PEAK,
        "truth_below_emit": t < statistics.median(emit_ms),
        "device": torch.cuda.get_device_name(0)}))
    eng.close()


if __name__ == "__main__":
    main()
