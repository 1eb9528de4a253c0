"""Timing of the scoring of an aligner's SAM (simmr_mapeval_truth_add + simmr_mapeval_truth_plan + simmr_mapeval_add) on the text
fit_sam_timing.py times through simmr_fit_add_sam: 1 M minimal-short pairs of one 100 Mbase synthetic slot, their SAM text made by
Engine.sam, given as the truth and as the aligner's output:
    python profiles/microbench/mapeval_timing.py [pairs]
Prints the HIP-event time of the three calls together (simmr_last_mapeval_ms) and of each, the text's bytes per second as a share
of the HBM peak figure bench.py uses, and checks that every read came out correct.  On a shared machine run it under a time limit:
    timeout -k 10 300 python profiles/microbench/mapeval_timing.py"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from simmr_amd import Engine, MinimalShortErrorProfile, _abi  # noqa: E402

HBM_PEAK_GBS = 8000.0  # bench.py's roofline peak


def main():
    pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    eng = Engine(0)
    eng.stage_synthetic(0, [100_000_000], 2)
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX, mean_phred_score=20).pod()
    reads = eng.simulate_pe_reads_from_genome(0, prof, 2 * pairs, 42, qual_offset=33)
    text = eng.sam(reads, [(0, ["c0"])], True)
    n_bytes = int(text.numel())
    ev = eng.mapeval(["c0"])
    for it in range(3):
        ev.reset(["c0"])
        ev.truth_add(text)
        t_add = ev.last_ms()
        n = ev.truth_plan()
        t_plan = ev.last_ms() - t_add
        ev.add(text)
        total = ev.last_ms()
        t_rec = total - t_add - t_plan
        counts, by = ev.read()
        rate = 2 * n_bytes / (total * 1e-3) / 1e9
        print(f"iter {it}: {n} truth entries, {n_bytes} bytes of SAM text on either side: truth_add {t_add:.3f} ms, truth_plan {t_plan:.3f} ms, "
              f"add {t_rec:.3f} ms, together {total:.3f} ms; {rate:.1f} GB/s of text = {100.0 * rate / HBM_PEAK_GBS:.2f} % of the "
              f"{HBM_PEAK_GBS:.0f} GB/s HBM peak; every read correct at MAPQ 255: {counts['reads_correct'] == n == int(by[255, 0])}", flush=True)
    ev.close()
    eng.close()


if __name__ == "__main__":
    main()
