#!/usr/bin/env python3
"""Times the gold-standard-assembly pass — simmr_regions_plan and simmr_regions_emit, each alone — next to simmr_depth_emit
for the same depth[] array, in one process on one device: the 100 Mbp bench genome covered by minimal-short 150 bp pairs at
roughly 0.5x (many short regions) and 30x (one region), min_depth 1, min_len 1.

All are HIP-event times (simmr_last_regions_ms after the plan, and after the emit: the difference; simmr_last_depth_ms around
the depth emit), taken after a warm-up, as the median of --steps repetitions.  The plan's time runs from its first launch
to its last and so includes its two read-backs of counts.  Every step checks the regions against depth[] itself (torch on
the device: covered positions, depth sum).  Prints one JSON line.

    python tools/regions_bench.py [--genome-bases N] [--coverages 0.5,30] [--steps K] [--warmup W]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

COPY_CEILING = 6.29e12  # bytes per second, the measured copy rate (profiles/microbench/write_bw_mi355x.txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-bases", type=int, default=100_000_000)
    ap.add_argument("--coverages", default="0.5,30")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()

    import torch
    from simmr_amd import MinimalShortErrorProfile, _abi
    from simmr_amd.engine import Engine
    eng = Engine(0)
    eng.stage_synthetic(0, [args.genome_bases], 2)
    eng.set_read_slots(16)
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
    med = statistics.median
    cases = []
    for cov in (float(x) for x in args.coverages.split(",")):
        n_reads = max(int(cov * args.genome_bases / 150) // 2 * 2, 2)
        reads = eng.simulate_pe_reads_from_genome(0, prof, n_reads, args.seed, qual_offset=33)
        n_pos = eng.depth_reset()
        eng.depth_add(reads)
        add_ms = eng.last_depth_ms()
        plan_ms, emit_ms, depth_emit_ms = [], [], []
        r = None
        for step in range(args.warmup + args.steps):
            d = eng.depth()
            de_ms = eng.last_depth_ms() - add_ms
            n, nb = eng.regions_plan(d, 1, 1)
            p_ms = eng.last_regions_ms()
            del r
            r = eng.regions(1, 1, depth=d)      # (plans again, then emits every column and the bases)
            e_ms = eng.last_regions_ms() - p_ms  # (the second plan's time stands in for its own: same work)
            covered, total = int((d.view(torch.int32) != 0).sum()), int(d.view(torch.int32).to(torch.int64).sum())
            assert len(r["len"]) == n and int(r["len"].sum()) == nb == covered == r["seq"].numel(), (n, nb, covered)
            assert int(r["depth_sum"].sum()) == total
            del d
            if step >= args.warmup:
                plan_ms.append(p_ms); emit_ms.append(e_ms); depth_emit_ms.append(de_ms)
        depth_bytes_plan = 2 * n_pos * 4            # count and runs read depth[] once each
        emit_bytes = nb * 4 + nb // 4 + nb + n * 48  # depth[] over the regions again, planes, bases, columns
        cases.append({
            "coverage": cov, "reads": reads.n_reads, "positions": n_pos, "regions": n, "bases": nb,
            "plan_ms": med(plan_ms), "emit_ms": med(emit_ms), "depth_emit_ms": med(depth_emit_ms),
            "plan_ms_all": plan_ms, "emit_ms_all": emit_ms, "depth_emit_ms_all": depth_emit_ms,
            "plan_bytes": depth_bytes_plan, "emit_bytes": emit_bytes,
            "traffic_floor_ms": (depth_bytes_plan + emit_bytes) / COPY_CEILING * 1e3,
            "plan_fraction_of_copy_ceiling": depth_bytes_plan / (med(plan_ms) * 1e-3) / COPY_CEILING,
            "emit_fraction_of_copy_ceiling": emit_bytes / (med(emit_ms) * 1e-3) / COPY_CEILING})
        del reads, r
    print(json.dumps({"bench": "regions_pass", "min_depth": 1, "min_len": 1, "steps": args.steps, "warmup": args.warmup,
                      "form": "count / scan / runs per 4 096-position tile; flag / scan / compact per 256 runs; one lane per 16-base chunk",
                      "cases": cases, "device": torch.cuda.get_device_name(0)}))
    eng.close()


if __name__ == "__main__":
    main()
