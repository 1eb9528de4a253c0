#!/usr/bin/env python3
"""Times the SAM pass (simmr_sam_plan + simmr_sam_emit) next to the truth pass of the same shard, in one process on one
device: minimal-short 150 bp pairs (SIMMR_SLOT16, counter mode) by default, minimal-long reads with --long.

simmr_last_sam_ms is the size pass, the scan and the write (HIP events); simmr_last_truth_ms the truth pass that made its
edit lists.  Both are taken after a warm-up, as the median of --steps repetitions, with the spread (min, max).  The bytes
per second are the SAM text's bytes over the SAM pass's time: compare with profiles/microbench/write_bw_mi355x.txt.
With --sorted the coordinate-sorted pass (simmr_sam_sort_plan + simmr_sam_sort_emit, simmr_last_sam_sort_ms) is timed on the same
columns in the same step, beside the unsorted one, and its text is checked to have the unsorted text's size.
Prints one JSON line.  Needs an MI355X: there is no fallback.

    python tools/sam_bench.py [--reads N] [--long] [--sorted] [--genome-bases N] [--steps K] [--warmup W]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--sorted", action="store_true")
    ap.add_argument("--genome-bases", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()

    from simmr_amd import MinimalLongErrorProfile, MinimalShortErrorProfile, _abi
    from simmr_amd.engine import Engine
    eng = Engine(0)
    eng.stage_synthetic(0, [args.genome_bases], 2)
    eng.set_read_slots(16)
    sam_ms, truth_ms, sort_ms, text_bytes = [], [], [], 0
    for step in range(args.warmup + args.steps):
        if args.long:
            prof = MinimalLongErrorProfile(gamma_mean=8000.0, gamma_std=6000.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
            reads = eng.simulate_long_reads([0], [args.reads], prof, args.seed, qual_offset=33)
        else:
            prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
            reads = eng.simulate_pe_reads_from_genome(0, prof, args.reads, args.seed, qual_offset=33)
        truth = eng.truth(reads)
        t_ms = eng.last_truth_ms()
        text = eng.sam(reads, [(0, ["bench"])], not args.long, truth=truth)
        s_ms = eng.last_sam_ms()
        text_bytes = int(text.numel())
        del text
        if args.sorted:
            text = eng.sam_sorted(reads, [(0, ["bench"])], not args.long, truth=truth)
            o_ms = eng.last_sam_sort_ms()
            assert int(text.numel()) == text_bytes
            del text
            if step >= args.warmup:
                sort_ms.append(o_ms)
        del truth, reads
        if step >= args.warmup:
            sam_ms.append(s_ms)
            truth_ms.append(t_ms)
    med = statistics.median(sam_ms)
    extra = {}
    if args.sorted:
        smed = statistics.median(sort_ms)
        extra = {"sam_sorted_ms_median": smed, "sam_sorted_ms_min": min(sort_ms), "sam_sorted_ms_max": max(sort_ms), "sorted_over_unsorted": smed / med}
    print(json.dumps({**extra, "workload": "minimal-long" if args.long else "minimal-short 150 bp PE", "reads": args.reads, "steps": args.steps,
                      "sam_ms_median": med, "sam_ms_min": min(sam_ms), "sam_ms_max": max(sam_ms), "truth_ms_median": statistics.median(truth_ms),
                      "sam_bytes": text_bytes, "sam_bytes_per_s": text_bytes / (med * 1e-3)}))


if __name__ == "__main__":
    main()
