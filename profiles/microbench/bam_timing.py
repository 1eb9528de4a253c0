"""Timing of the BAM record pass (simmr_bam_plan + simmr_bam_emit) against the SAM text pass (simmr_sam_plan + simmr_sam_emit) on
the same columns, and of BGZF framing (simmr_bgzf_frame) against a device-to-device copy of the same bytes: 10 M minimal-short
150 bp reads (5 M pairs) of one 100 Mbase synthetic slot, in ONE process, the runs alternating, after a warm-up:
    python profiles/microbench/bam_timing.py [reads]
The record and text passes are HIP-event times (simmr_last_bam_ms, simmr_last_sam_ms); simmr_bgzf_frame synchronises, so it and
the copy are timed by the host's clock around a synchronised call.  The per-kernel split is a kernel trace of the same command:
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/microbench/bam_timing.py
On a shared machine run each GPU step under its own time limit and chain them."""
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from simmr_amd import Engine, MinimalShortErrorProfile, _abi  # noqa: E402

HBM_PEAK_GBS = 8000.0  # bench.py's roofline peak
ROUNDS = 5


def main():
    import torch
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    eng = Engine(0)
    eng.stage_synthetic(0, [100_000_000], 2)
    eng.set_read_slots(16)
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
    reads = eng.simulate_pe_reads_from_genome(0, prof, n_reads, 42, qual_offset=33)
    truth = eng.truth(reads)
    rn = [(0, ["c0"])]
    bam_ms, sam_ms, frame_ms, copy_ms = [], [], [], []
    for it in range(ROUNDS + 1):  # the first round warms up
        rec = eng.bam(reads, rn, True, truth, framed=False)
        b = eng.last_bam_ms()
        text = eng.sam(reads, rn, True, truth)
        s = eng.last_sam_ms()
        n_rec, n_text = int(rec.numel()), int(text.numel())
        del text
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        blocks = eng.bgzf(rec)
        f = (time.perf_counter() - t0) * 1e3
        n_blocks = int(blocks.numel())
        del blocks
        dst = torch.empty_like(rec)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(rec)
        torch.cuda.synchronize()
        c = (time.perf_counter() - t0) * 1e3
        del dst, rec
        if it:
            bam_ms.append(b); sam_ms.append(s); frame_ms.append(f); copy_ms.append(c)
        print(f"round {it}: bam {b:.3f} ms, sam {s:.3f} ms, bgzf_frame {f:.3f} ms (allocation of dst included), copy {c:.3f} ms", flush=True)
    med = statistics.median
    print(f"{reads.n_reads} reads: {n_rec} bytes of records = {n_rec / reads.n_reads:.1f} a read, {n_text} bytes of SAM text = {n_text / reads.n_reads:.1f} a read, "
          f"{n_blocks} bytes of blocks")
    print(f"medians of {ROUNDS}: records {med(bam_ms):.3f} ms ({n_rec / med(bam_ms) / 1e6:.0f} GB/s written, {100 * n_rec / med(bam_ms) / 1e6 / HBM_PEAK_GBS:.1f} % of "
          f"the {HBM_PEAK_GBS:.0f} GB/s peak), text {med(sam_ms):.3f} ms: records / text = {med(bam_ms) / med(sam_ms):.2f}")
    print(f"medians of {ROUNDS}: bgzf_frame {med(frame_ms):.3f} ms ({n_rec / med(frame_ms) / 1e6:.0f} GB/s of source), copy {med(copy_ms):.3f} ms: "
          f"frame / copy = {med(frame_ms) / med(copy_ms):.1f}")
    eng.close()


if __name__ == "__main__":
    main()
