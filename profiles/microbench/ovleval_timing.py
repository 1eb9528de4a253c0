"""Timing of the scoring of an overlapper's PAF (simmr_ovleval_truth_add + simmr_ovleval_truth_plan + simmr_ovleval_add) on
the true overlaps of a run: 350 000 minimal-long reads at gamma(8000, 6000) with uniform starts on one
100 Mbase synthetic slot, min_overlap 1000 — about 10^7 pairs — their PAF text made by Engine.overlaps, given as the truth and as
the candidate:
    python profiles/microbench/ovleval_timing.py [reads] [min_overlap]
Prints the HIP-event time of the calls together (simmr_last_ovleval_ms) and of each, the text's bytes per second as a share of the
HBM peak figure bench.py uses, and checks that every pair came out found once.  On a shared machine run it under a time limit:
    timeout -k 10 300 python profiles/microbench/ovleval_timing.py"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from simmr_amd import Engine, MinimalLongErrorProfile, _abi  # noqa: E402

HBM_PEAK_GBS = 8000.0  # bench.py's roofline peak


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 350_000
    min_overlap = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    eng = Engine(0)
    eng.stage_synthetic(0, [100_000_000], 2)
    prof = MinimalLongErrorProfile(gamma_mean=8000.0, gamma_std=6000.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    prof.long_start_mode = _abi.START_UNIFORM
    eng.overlap_reset(False)
    step = 50_000
    for first in range(0, reads, step):  # the overlap pass keeps 20 bytes a read; the reads themselves are dropped
        out = eng.simulate_long_reads([0], [reads], prof, 42, first=first, count=min(step, reads - first), qual_offset=33)
        eng.overlap_add(out)
        del out
    text = eng.overlaps(min_overlap, text=True)
    n_bytes = int(text.numel())
    ev = eng.overlap_eval()
    for it in range(3):
        ev.reset()
        ev.truth_add(text)
        t_add = ev.last_ms()
        n, n_reads = ev.truth_plan()
        t_plan = ev.last_ms() - t_add
        ev.add(text)
        t_rec = ev.last_ms() - t_add - t_plan
        total = t_add + t_plan + t_rec
        counts, by = ev.read()   # (the reduction over the entries is outside the spans)
        rate = 2 * n_bytes / (total * 1e-3) / 1e9
        ok = counts["pairs_found"] == counts["correct"] == n == int(by[:, 0].sum()) and counts["wrong"] == counts["pairs_multiple"] == 0
        print(f"iter {it}: {n} true pairs of {n_reads} reads, {n_bytes} bytes of PAF text on either side: truth_add {t_add:.3f} ms, "
              f"truth_plan {t_plan:.3f} ms, add {t_rec:.3f} ms, together {total:.3f} ms; {rate:.1f} GB/s of text = "
              f"{100.0 * rate / HBM_PEAK_GBS:.2f} % of the {HBM_PEAK_GBS:.0f} GB/s HBM peak; every pair found once: {ok}", flush=True)
    ev.close()
    eng.close()


if __name__ == "__main__":
    main()
