#!/usr/bin/env python3
"""Times the strain-divergence pass — simmr_strain_plan (count + scan) and simmr_strain_apply, HIP events through
simmr_last_strain_ms — on the synthetic bench genome, in one process on one device: 100 Mbp at identity 0.99 by default.
Every repetition stages the genome again (an apply diverges it).  Prints one JSON line.

    python tools/strain_bench.py [--genome-bases N] [--identity F] [--steps K] [--warmup W]
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
    ap.add_argument("--genome-bases", type=int, default=100_000_000)
    ap.add_argument("--identity", type=float, default=0.99)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()

    import ctypes as C

    import torch
    from simmr_amd import _abi
    from simmr_amd.engine import Engine
    eng = Engine(0)
    plan_ms, apply_ms, n = [], [], 0
    for step in range(args.warmup + args.steps):
        eng.stage_synthetic(0, [args.genome_bases], 2)
        n = eng.strain_plan(0, args.identity, args.seed)
        p_ms = eng.last_strain_ms()
        cols = {k: torch.empty(max(n, 1), dtype=dt, device=eng.device)
                for k, dt in (("contig", torch.int32), ("pos", torch.int64), ("ref", torch.uint8), ("alt", torch.uint8))}
        out = _abi.StrainOut(cols["contig"].data_ptr(), cols["pos"].data_ptr(), cols["ref"].data_ptr(), cols["alt"].data_ptr(), n)
        eng._check(eng.lib.simmr_strain_apply(eng._h, 0, C.byref(out)))
        a_ms = eng.last_strain_ms() - p_ms
        assert int(cols["pos"][-1]) < args.genome_bases and bool((cols["ref"] != cols["alt"]).all())
        if step >= args.warmup:
            plan_ms.append(p_ms); apply_ms.append(a_ms)
    med = statistics.median
    print(json.dumps({
        "bench": "strain_pass", "genome_bases": args.genome_bases, "identity": args.identity, "sites": n,
        "site_rate": n / args.genome_bases, "steps": args.steps, "warmup": args.warmup,
        "form": "one lane per 16-base plane word, four Philox blocks; count, tile scan, apply in place",
        "strain_plan_ms": med(plan_ms), "strain_apply_ms": med(apply_ms), "strain_ms": med(plan_ms) + med(apply_ms),
        "strain_plan_ms_all": plan_ms, "strain_apply_ms_all": apply_ms,
        "philox_blocks_per_second": 2 * (args.genome_bases / 4) / ((med(plan_ms) + med(apply_ms)) * 1e-3),
        "device": torch.cuda.get_device_name(0)}))
    eng.close()


if __name__ == "__main__":
    main()
