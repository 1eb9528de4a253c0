#!/usr/bin/env python3
"""Times the coverage-depth pass — simmr_depth_add, simmr_depth_emit and simmr_depth_summarize, each alone — next to the
emit kernel of the same shard, in one process on one device: BASELINE config 2 by default (100 M reads of minimal-short
150 bp pairs on 100 Mbp, SIMMR_SLOT16, counter mode).

All are HIP-event times (simmr_last_depth_ms after the add, after the emit and after the summarize: the differences;
simmr_last_emit_kernel_ms), taken after a warm-up, as the median of --steps repetitions.  The add is two scattered 4-byte
atomics per read: the implied atomics per second are reported beside the bytes the three steps move.  Every step also checks
the sums against the emit's own counters.  The statistics and truth passes' committed times (profiles/r6/) are quoted for
scale.  Prints one JSON line.

    python tools/depth_bench.py [--reads N] [--genome-bases N] [--steps K] [--warmup W] [--window W]
"""
import argparse
import json
import re
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

COPY_CEILING = 6.29e12  # bytes per second, the measured copy rate (profiles/microbench/write_bw_mi355x.txt)


def committed(name, key):
    m = re.search(rf'"{key}": ([0-9.]+)', (ROOT / "profiles" / "r6" / name).read_text())
    return float(m.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--genome-bases", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--window", type=int, default=1000)
    args = ap.parse_args()

    import torch
    from simmr_amd import MinimalShortErrorProfile, _abi
    from simmr_amd.engine import Engine
    eng = Engine(0)
    eng.stage_synthetic(0, [args.genome_bases], 2)
    eng.set_read_slots(16)
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
    emit_ms, add_ms, scan_ms, sum_ms = [], [], [], []
    reads = s = None
    for step in range(args.warmup + args.steps):
        eng.counters_reset()
        if reads is None:
            reads = eng.simulate_pe_reads_from_genome(0, prof, args.reads, args.seed, qual_offset=33)
        else:
            eng.pe_plan(0, prof, args.reads, args.seed)
            eng.pe_emit(0, reads)
        e_ms = eng.last_emit_kernel_ms()
        cnt = eng.counters()
        n_pos = eng.depth_reset()
        eng.depth_add(reads)
        a_ms = eng.last_depth_ms()
        d = eng.depth()
        b_ms = eng.last_depth_ms() - a_ms
        s = eng.depth_summary(args.window, d)
        c_ms = eng.last_depth_ms() - a_ms - b_ms
        assert int(s["depth_sum"].sum()) == int(s["win_sum"].sum()) == int(cnt[_abi.CNT_BASES]), (int(s["depth_sum"].sum()), int(cnt[_abi.CNT_BASES]))
        assert int(s["hist"].sum()) == n_pos == args.genome_bases and int(s["covered"].sum()) == n_pos - int(s["hist"][0])
        del d
        if step >= args.warmup:
            emit_ms.append(e_ms); add_ms.append(a_ms); scan_ms.append(b_ms); sum_ms.append(c_ms)
    n = reads.n_reads
    med = statistics.median
    n_win = len(s["win_sum"])
    add_bytes = n * 24                              # start, end 8 B; contig, genome 4 B
    scan_bytes = (2 * (n_pos + 1) + n_pos) * 4      # the difference array read twice, depth[] written once
    sum_bytes = n_pos * 4 + n_win * 16
    print(json.dumps({
        "bench": "depth_pass", "reads": n, "positions": n_pos, "window": args.window, "windows": n_win, "steps": args.steps, "warmup": args.warmup,
        "form": "one lane per read, two no-return agent-scope atomics; tile reduce / scan / apply; one wave per window",
        "depth_add_ms": med(add_ms), "depth_emit_ms": med(scan_ms), "depth_summarize_ms": med(sum_ms), "emit_kernel_ms": med(emit_ms),
        "depth_add_ms_all": add_ms, "depth_emit_ms_all": scan_ms, "depth_summarize_ms_all": sum_ms, "emit_kernel_ms_all": emit_ms,
        "add_over_emit_kernel": med(add_ms) / med(emit_ms),
        "atomics_per_second": 2 * n / (med(add_ms) * 1e-3),
        "add_bytes": add_bytes, "emit_bytes": scan_bytes, "summarize_bytes": sum_bytes,
        "traffic_floor_ms": (add_bytes + scan_bytes + sum_bytes) / COPY_CEILING * 1e3,
        "emit_fraction_of_copy_ceiling": scan_bytes / (med(scan_ms) * 1e-3) / COPY_CEILING,
        "committed_stats_ms": committed("stats_pass_mi355x.txt", "stats_ms"), "committed_truth_ms": committed("truth_pass_mi355x.txt", "truth_ms"),
        "depth_max": int(s["depth_max"].max()), "mean_depth": float(s["depth_sum"].sum()) / n_pos,
        "device": torch.cuda.get_device_name(0)}))
    eng.close()


if __name__ == "__main__":
    main()
