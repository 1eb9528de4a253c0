"""Timing of the scoring of an assembler's contigs (simmr_asmeval_truth_add + simmr_asmeval_truth_plan + simmr_asmeval_add): a
synthetic truth of `mbases` Mbase in four genomes, as --gold-assembly writes it (records of 50 kbase, lines of 80), and a candidate
of the same size cut from it in contigs of 20 kbase with a substitution every 1000 bases, at k = 31:
    python profiles/microbench/asmeval_timing.py [mbases] [plain]
One warm-up pass at a hundredth of the size, then ONE timed pass (with `plain`: the lookups by a binary search over all entries
instead of the prefix table); prints the HIP-event time of each call (simmr_last_asmeval_ms), the sort's share of the plan, bases
per second and lookups per second.  On a shared machine run each pass under a time limit of its own and chain them:
    timeout -k 10 500 python profiles/microbench/asmeval_timing.py 100 && timeout -k 10 500 python profiles/microbench/asmeval_timing.py 100 plain"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from simmr_amd import Engine  # noqa: E402
from tests._synth import synthetic_contigs_chunked  # noqa: E402

GENOMES = ["g0", "g1", "g2", "g3"]


def wrap(seq: np.ndarray, width=80) -> np.ndarray:
    """the sequence in lines of `width` bases, each with its newline"""
    n = len(seq) // width * width
    body = np.concatenate([seq[:n].reshape(-1, width), np.full((n // width, 1), 10, dtype=np.uint8)], axis=1).reshape(-1)
    return np.concatenate([body, seq[n:], np.array([10], dtype=np.uint8)]) if n < len(seq) else body


def texts(mbases: int, seed=7):
    per = mbases * 1_000_000 // 4
    truth, cand = [], []
    for g, seq in enumerate(synthetic_contigs_chunked([per] * 4, seed)):
        for a in range(0, per, 50_000):
            truth += [np.frombuffer(f">g{g}|s0:{a}-{min(a + 50_000, per)} depth_sum=1\n".encode(), dtype=np.uint8), wrap(seq[a:a + 50_000])]
        mut = seq.copy()
        at = np.arange(500, per, 1000)
        mut[at] = np.where(mut[at] == ord("A"), ord("C"), ord("A")).astype(np.uint8)
        for a in range(0, per, 20_000):
            cand += [np.frombuffer(f">contig_{g}_{a}\n".encode(), dtype=np.uint8), wrap(mut[a:a + 20_000])]
    return np.concatenate(truth), np.concatenate(cand)


def one_pass(eng, mbases, plain, report):
    import torch
    truth, cand = texts(mbases)
    d_truth, d_cand = torch.from_numpy(truth).to(eng.device), torch.from_numpy(cand).to(eng.device)
    ev = eng.assembly_eval_open(GENOMES, 31, plain)
    try:
        ev.truth_add(d_truth)
        t_add = ev.ms()[0]
        entries = ev.truth_plan()
        total, t_sort = ev.ms()
        t_plan = total - t_add
        ev.add(d_cand)
        t_cand = ev.ms()[0] - total
        c = ev.read()[0]
    finally:
        ev.close()
    if report:
        print(f"{'plain search' if plain else 'prefix table'}: truth {c['truth_bases']} bases ({len(truth)} bytes), {c['truth_kmers']} occurrences, {entries} entries; "
              f"candidate {c['bases']} bases, {c['kmers']} k-mers, {c['found']} found, {c['novel']} novel, {c['records']} contigs ({c['contigs_pure']} pure)")
        print(f"  truth_add {t_add:.2f} ms ({c['truth_bases'] / t_add / 1e6:.2f} Gbase/s), truth_plan {t_plan:.2f} ms of which the sort {t_sort:.2f} ms, "
              f"add {t_cand:.2f} ms ({c['bases'] / t_cand / 1e6:.2f} Gbase/s, {c['kmers'] / t_cand / 1e6:.3f} G lookups/s), together {t_add + t_plan + t_cand:.2f} ms; "
              f"one run, untuned", flush=True)


def main():
    mbases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    plain = len(sys.argv) > 2 and sys.argv[2] == "plain"
    eng = Engine(0)
    one_pass(eng, max(mbases // 100, 1), plain, False)   # warm-up
    one_pass(eng, mbases, plain, True)
    eng.close()


if __name__ == "__main__":
    main()
