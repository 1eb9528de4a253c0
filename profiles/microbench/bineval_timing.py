"""Timing of the scoring of a binner's bins (simmr_bineval_truth_add + simmr_bineval_truth_plan + simmr_bineval_add +
simmr_bineval_read): a synthetic truth of `contigs` contigs (default 2 000 000, names of about 25 bytes, 500 genomes and a few
contigs of none) as --eval-assembly-contigs writes it, and an assignment of every contig to one of 2 000 bins, nine in ten to a bin
of their genome:
    python profiles/microbench/bineval_timing.py [contigs]
One warm-up pass at a hundredth of the size, then ONE timed pass; prints the HIP-event time of each call (simmr_last_bineval_ms), the
sort's share of the plan, contigs and records per second.  On a shared machine run it under a time limit of its own:
    timeout -k 10 500 python profiles/microbench/bineval_timing.py"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from simmr_amd import Engine  # noqa: E402
from tests._synth import splitmix64_words  # noqa: E402

N_GENOMES, N_BINS = 500, 2000
GENOMES = [f"genome_{g:03d}" for g in range(N_GENOMES)]


def texts(n: int, seed=7):
    w = splitmix64_words(seed, 3 * n)
    genome = (w[:n] % np.uint64(N_GENOMES + 1)).astype(np.int64)                  # N_GENOMES: none
    length = (w[n:2 * n] % np.uint64(200_000) + np.uint64(500)).astype(np.int64)
    pick = w[2 * n:]
    own = (pick % np.uint64(10)) != 0
    bins = np.where(own, genome * (N_BINS // (N_GENOMES + 1)) + ((pick >> np.uint64(8)) % np.uint64(3)).astype(np.int64),
                    ((pick >> np.uint64(16)) % np.uint64(N_BINS)).astype(np.int64))
    names = [f"NODE_{i:08d}_length_{l:06d}" for i, l in enumerate(length.tolist())]   # 27 bytes
    gn = GENOMES + ["."]
    truth = "".join(f"{nm}\t{l}\t{l - 30}\t{l - 40}\t0\t1\t{l - 40}\t{gn[g]}\n" for nm, l, g in zip(names, length.tolist(), genome.tolist()))
    cand = "".join(f"{nm}\tbin.{b:04d}\n" for nm, b in zip(names, bins.tolist()))
    return np.frombuffer(truth.encode(), dtype=np.uint8), np.frombuffer(cand.encode(), dtype=np.uint8)


def one_pass(eng, n, report):
    import torch
    truth, cand = texts(n)
    d_truth, d_cand = torch.from_numpy(truth.copy()).to(eng.device), torch.from_numpy(cand.copy()).to(eng.device)
    ev = eng.binning_eval_open(GENOMES, 64)
    try:
        ev.truth_add(d_truth)
        t_add = ev.ms()[0]
        contigs = ev.truth_plan()
        total, t_sort = ev.ms()
        t_plan = total - t_add
        ev.add(d_cand)
        after_add = ev.ms()[0]
        t_cand = after_add - total
        c = ev.read()[0]
        t_read = ev.ms()[0] - after_add
    finally:
        ev.close()
    if report:
        print(f"truth {contigs} contigs ({len(truth)} bytes, {c['truth_bases']} bases, {c['truth_none']} of none), {c['records']} records ({len(cand)} bytes), "
              f"{c['assigned']} assigned, {c['bins']} bins, {c['cells']} cells; purity {c['sum_top_bases'] / max(c['assigned_bases'], 1):.4f}")
        print(f"  truth_add {t_add:.2f} ms ({contigs / t_add / 1e3:.1f} M contigs/s), truth_plan {t_plan:.2f} ms of which the sort {t_sort:.2f} ms, "
              f"add {t_cand:.2f} ms ({c['records'] / t_cand / 1e3:.1f} M lookups/s), read {t_read:.2f} ms, together {t_add + t_plan + t_cand + t_read:.2f} ms; "
              f"one run, untuned", flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    eng = Engine(0)
    one_pass(eng, max(n // 100, 1), False)   # warm-up
    one_pass(eng, n, True)
    eng.close()


if __name__ == "__main__":
    main()
