#!/usr/bin/env python3
"""Times the allele-count pass (simmr_pileup_add alone) next to the emit kernel of the same shard, in one process on one
device, on the 100 Mbp bench genome diverged to a strain whose sites are the site list:

    short: 100 M reads of minimal-short 150 bp pairs (SIMMR_SLOT16, counter mode) at identity 0.99 — 1.5 sites per read;
    long:  1 M minimal-long reads at gamma 8000 / 6000 (per-read lengths, counter mode) at the same identity — 80 per read.

Both are HIP-event times (simmr_last_pileup_ms, simmr_last_emit_kernel_ms), taken after a warm-up, as the median of --steps
repetitions; every step resets the table, adds the shard and checks that the counts sum to the number of (read, site) pairs
the depth pass gives for the same reads (the header's invariant).  Prints one JSON line.

    python tools/pileup_bench.py [--short-reads N] [--long-reads N] [--genome-bases N] [--identity X] [--steps K] [--warmup W]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# per 100 M reads of the short workload, from the committed profiles: the count half of the truth pass and the statistics pass
TRUTH_COUNT_MS, STATS_MS = 14.6, 56.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--short-reads", type=int, default=100_000_000)
    ap.add_argument("--long-reads", type=int, default=1_000_000)
    ap.add_argument("--genome-bases", type=int, default=100_000_000)
    ap.add_argument("--identity", type=float, default=0.99)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()

    import numpy as np
    import torch
    from simmr_amd import MinimalLongErrorProfile, MinimalShortErrorProfile, _abi
    from simmr_amd.engine import Engine
    eng = Engine(0)
    eng.stage_synthetic(0, [args.genome_bases], 2)
    s = eng.strain(0, args.identity, args.seed)
    n_sites = int(s["pos"].size)
    pos = torch.from_numpy(s["pos"].view(np.int64)).to(eng.device)
    genome, contig = torch.zeros(n_sites, dtype=torch.int32, device=eng.device), torch.zeros(n_sites, dtype=torch.int32, device=eng.device)
    eng.set_read_slots(16)
    med = statistics.median
    cases = []
    for name, n_reads in (("short", args.short_reads), ("long", args.long_reads)):
        if n_reads <= 0:
            continue
        if name == "short":
            prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
            reads = eng.simulate_pe_reads_from_genome(0, prof, n_reads, args.seed, qual_offset=33)
        else:
            prof = MinimalLongErrorProfile(gamma_mean=8000.0, gamma_std=6000.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX,
                                           uniform_start=True).pod()
            reads = eng.simulate_long_reads([0], [n_reads], prof, args.seed, qual_offset=33)
        emit_ms = eng.last_emit_kernel_ms()
        # the pairs of the shard, from the depth pass: depth[] summed over the sites
        eng.depth_reset()
        eng.depth_add(reads)
        pairs = int(eng.depth().view(torch.int32)[pos].to(torch.int64).sum())
        add_ms = []
        for step in range(args.warmup + args.steps):
            eng.pileup_reset(genome, contig, pos)
            eng.pileup_add(reads)
            ms = eng.last_pileup_ms()
            counts = eng.pileup()
            assert int(counts.sum(dtype=np.uint64)) == pairs, (int(counts.sum(dtype=np.uint64)), pairs)
            if step >= args.warmup:
                add_ms.append(ms)
        t = med(add_ms)
        per_100m = t * 1e8 / reads.n_reads
        cases.append({"workload": name, "reads": reads.n_reads, "seq_bytes": reads.total_bases, "pairs": pairs, "pairs_per_read": pairs / reads.n_reads,
                      "pileup_add_ms": t, "pileup_add_ms_all": add_ms, "emit_kernel_ms": emit_ms, "add_over_emit": t / emit_ms,
                      "pairs_per_second": pairs / (t * 1e-3), "add_ms_per_100M_reads": per_100m,
                      "over_truth_count_14.6ms": per_100m / TRUTH_COUNT_MS if name == "short" else None,
                      "over_stats_56.2ms": per_100m / STATS_MS if name == "short" else None})
        del reads, counts
    print(json.dumps({"bench": "pileup_pass", "genome_bases": args.genome_bases, "identity": args.identity, "sites": n_sites,
                      "steps": args.steps, "warmup": args.warmup,
                      "form": "64 reads per wave: two bisections per lane, DPP scan, pairs 64 at a time through ds_bpermute, one atomic per pair",
                      "cases": cases, "device": torch.cuda.get_device_name(0)}))
    eng.close()


if __name__ == "__main__":
    main()
