"""Timing of the overlap pass (simmr_overlap_plan / simmr_overlap_emit): 200 000 minimal-long reads at the bench's
gamma(8000, 6000) on one 100 Mbase synthetic slot, min_overlap 1000:
    python profiles/microbench/overlap_timing.py [reads] [min_overlap] [reference|uniform]
Prints n_pairs, total_bytes, the plan's and the emit's HIP-event time (simmr_last_overlap_ms) and the emit's bytes per second as
a share of the linear store figure of profiles/microbench/write_bw_mi355x.txt.  `reference` (the bench's start mode: every long
read starts within the first read_length bases of its sequence, so the run is ONE pile and nearly every pair overlaps) drains the
first windows of the text only, EMIT_CAP bytes of it, through a 2 GiB buffer; `uniform` (--uniform-start) emits the whole text."""
import re
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

import torch  # noqa: E402

from simmr_amd import Engine, MinimalLongErrorProfile, _abi  # noqa: E402


EMIT_CAP = 8 << 30   # text drained at most (the reference start mode's text is hundreds of GiB)
WINDOW = 2 << 30


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    min_overlap = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    mode = sys.argv[3] if len(sys.argv) > 3 else "reference"
    store_tbs = float(re.search(r"linear aligned fill.*?([\d.]+) TB/s", (HERE / "write_bw_mi355x.txt").read_text()).group(1))
    eng = Engine(0)
    eng.stage_synthetic(0, [100_000_000], 2)
    prof = MinimalLongErrorProfile(gamma_mean=8000.0, gamma_std=6000.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    if mode == "uniform":
        prof.long_start_mode = _abi.START_UNIFORM
    # the columns of the run, range by range: the overlap pass keeps 20 bytes a read, the reads themselves are dropped
    eng.overlap_reset(False)
    step = 50_000
    for first in range(0, reads, step):
        out = eng.simulate_long_reads([0], [reads], prof, 42, first=first, count=min(step, reads - first), qual_offset=33)
        eng.overlap_add(out)
        del out
    text = None
    for it in range(3):
        n, pairs, total = eng.overlap_plan(min_overlap)
        plan_ms = eng.last_overlap_ms()
        if text is None:
            text = torch.empty(max(min(total, WINDOW), 1), dtype=torch.uint8, device=eng.device)
        place, done, windows = 0, 0, 0
        while place < n and done < min(total, EMIT_CAP):
            n_places, _, nbytes = eng.overlap_window(place, text.numel())
            eng._check(eng.lib.simmr_overlap_emit(eng._h, place, n_places, None, text.data_ptr(), text.numel()))
            place, done, windows = place + n_places, done + nbytes, windows + 1
        emit_ms = eng.last_overlap_ms() - plan_ms
        rate = done / (emit_ms * 1e-3) if emit_ms > 0 else 0.0
        print(f"iter {it}: {n} reads, {mode} starts, min_overlap {min_overlap}: n_pairs {pairs}, total_bytes {total}, plan {plan_ms:.3f} ms, "
              f"emit {emit_ms:.3f} ms for {done} bytes in {windows} window(s), {rate / 1e9:.1f} GB/s = "
              f"{100.0 * rate / (store_tbs * 1e12):.2f} % of the {store_tbs} TB/s store figure", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
