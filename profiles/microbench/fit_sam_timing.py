"""Timing of the model fit's SAM route (simmr_fit_add_sam) against the columns route (simmr_fit_add) on the same reads: 1 M
minimal-short pairs of one 100 Mbase synthetic slot, their SAM text made by Engine.sam:
    python profiles/microbench/fit_sam_timing.py [pairs]
Prints both HIP-event times (simmr_last_fit_ms), the text's bytes per second as a share of the HBM peak figure bench.py uses, and
checks that the two models are the same bytes.  The per-kernel split is a kernel trace of the same command:
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/microbench/fit_sam_timing.py
On a shared machine run each GPU step under its own time limit and chain them:
    timeout -k 10 300 python profiles/microbench/fit_sam_timing.py && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -- python ..."""
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
    models = {}
    for it in range(3):
        eng.fit_reset(7, 20, 1 << 24)
        eng.fit_add(reads, 2)
        cols_ms = eng.last_fit_ms()
        models["columns"] = eng.fit_model()["model_bytes"]
        eng.fit_reset(7, 20, 1 << 24)
        eng.fit_add_sam(text, 2)
        sam_ms = eng.last_fit_ms()
        models["sam"] = eng.fit_model()["model_bytes"]
        rate = n_bytes / (sam_ms * 1e-3) / 1e9
        print(f"iter {it}: {reads.n_reads} reads, {n_bytes} bytes of SAM text: fit_add {cols_ms:.3f} ms, fit_add_sam {sam_ms:.3f} ms "
              f"({sam_ms / cols_ms:.1f} x), {rate:.1f} GB/s of text = {100.0 * rate / HBM_PEAK_GBS:.2f} % of the {HBM_PEAK_GBS:.0f} GB/s HBM peak; "
              f"models identical: {models['sam'] == models['columns']}", flush=True)
    c = eng.fit_sam_counts()
    print("counts:", {k: v for k, v in c.items() if v}, flush=True)
    eng.close()


if __name__ == "__main__":
    main()
