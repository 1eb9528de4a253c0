"""Timing of the placement of an assembler's contigs (simmr_asmmap_truth_add + simmr_asmmap_truth_plan + simmr_asmmap_add): the
synthetic truth of asmeval_timing.py (`mbases` Mbase in four genomes, records of 50 kbase, lines of 80) and a candidate of the same
size cut from it in contigs of 20 kbase with a substitution every 1000 bases, of which one contig in ten is a chimera of two genomes
(its second half comes from the next genome), at k = 31 and the default thresholds:
    python profiles/microbench/asmmap_timing.py [mbases]
One warm-up pass at a hundredth of the size, then ONE timed pass; prints the HIP-event time of each call (simmr_last_asmmap_ms) and
bases per second.  On a shared machine run it under a time limit of its own:
    timeout -k 10 500 python profiles/microbench/asmmap_timing.py 100"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from simmr_amd import Engine  # noqa: E402
from tests._synth import synthetic_contigs_chunked  # noqa: E402

sys.path.insert(0, str(HERE))
from asmeval_timing import GENOMES, wrap  # noqa: E402


def texts(mbases: int, seed=7):
    per = mbases * 1_000_000 // 4
    truth, cand, muts = [], [], []
    for g, seq in enumerate(synthetic_contigs_chunked([per] * 4, seed)):
        for a in range(0, per, 50_000):
            truth += [np.frombuffer(f">g{g}|s0:{a}-{min(a + 50_000, per)} depth_sum=1\n".encode(), dtype=np.uint8), wrap(seq[a:a + 50_000])]
        mut = seq.copy()
        at = np.arange(500, per, 1000)
        mut[at] = np.where(mut[at] == ord("A"), ord("C"), ord("A")).astype(np.uint8)
        muts.append(mut)
    for g in range(4):
        for i, a in enumerate(range(0, per, 20_000)):
            piece = muts[g][a:a + 20_000]
            if i % 10 == 9:  # a chimera: the second half from the next genome
                piece = np.concatenate([piece[:10_000], muts[(g + 1) % 4][a + 10_000:a + 20_000]])
            cand += [np.frombuffer(f">contig_{g}_{a}\n".encode(), dtype=np.uint8), wrap(piece)]
    return np.concatenate(truth), np.concatenate(cand)


def one_pass(eng, mbases, report):
    import torch
    truth, cand = texts(mbases)
    d_truth, d_cand = torch.from_numpy(truth).to(eng.device), torch.from_numpy(cand).to(eng.device)
    ev = eng.assembly_map_open(GENOMES, 31)
    try:
        ev.truth_add(d_truth)
        t_add = ev.ms()
        anchors = ev.truth_plan()
        total = ev.ms()
        t_plan = total - t_add
        ev.add(d_cand)
        t_cand = ev.ms() - total
        c = ev.read()[0]
    finally:
        ev.close()
    if report:
        print(f"truth {c['truth_bases']} bases ({len(truth)} bytes), {c['truth_kmers']} occurrences, {anchors} anchors, {c['truth_repeats']} repeats; "
              f"candidate {c['bases']} bases, {c['kmers']} k-mers, {c['hits']} hits, {c['runs']} runs ({c['runs_dropped']} dropped), {c['blocks']} blocks, "
              f"{c['records']} contigs ({c['contigs_misassembled']} misassembled, {c['breaks_inter_genome']} inter-genome breaks)")
        print(f"  truth_add {t_add:.2f} ms ({c['truth_bases'] / t_add / 1e6:.2f} Gbase/s), truth_plan {t_plan:.2f} ms, "
              f"add {t_cand:.2f} ms ({c['bases'] / t_cand / 1e6:.2f} Gbase/s), together {t_add + t_plan + t_cand:.2f} ms; one run, untuned", flush=True)


def main():
    mbases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    eng = Engine(0)
    one_pass(eng, max(mbases // 100, 1), False)   # warm-up
    one_pass(eng, mbases, True)
    eng.close()


if __name__ == "__main__":
    main()
