"""Closing an engine gives back everything it allocated.  The route taken is the one whose buffers no list named: a paired plan
in the reference RNG mode, whose emit kernel does not write text, so simmr_emit_fastq builds the columns in buffers of the
engine first (fd_seq and fd_qual of plan.total_bases bytes each, seven smaller ones, fq_hlen and fq_tpl_dev) and frames them.
Each cycle also takes the ground truth and the run statistics of a small shard, so the states of those two units, which live in
slots of the engine, are part of what a close has to give back."""
import pytest

from simmr_amd import MinimalShortErrorProfile, _abi
from tests.test_gpu_cli import FMT

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def test_closed_engines_leave_no_device_memory_behind():
    """Six engines, each made, used and closed: the device's free memory after the sixth close against after the first.  One
    cycle's columns are at least 128 MiB (asserted from the plan), so an engine that kept them would cost five times that;
    the bound is one cycle's worth.  Measured on the MI355X: 0.0 MiB with the owning buffers (twice), 910.0 MiB at the parent commit (LAB.md)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from simmr_amd.engine import Engine
    prof = MinimalShortErrorProfile(read_length=250, insert_size=400).pod()
    assert prof.rng_mode == _abi.RNG_REFERENCE
    names = [(0, "g0", ["c0", "c1"])]

    def cycle():
        eng = Engine(0)
        try:
            eng.stage_synthetic(0, [200_000, 50_000], 1)
            info = eng.pe_plan(0, prof, 300_000, 42)
            assert info.total_bases >= 64 * MIB, info.total_bases
            text = eng.fastq_direct(FMT, names)
            assert text.numel() > 2 * info.total_bases
            del text
            # the states the units keep in the engine's slots: truth.hip's and stats.hip's buffers and events go with the engine too
            reads = eng.simulate_pe_reads_from_genome(0, prof, 2000, 42, qual_offset=33)
            assert eng.truth(reads).n_edits > 0 and eng.last_truth_ms() > 0
            eng.stats_reset()
            eng.stats_add(reads, 2)
            assert eng.stats()["reads"].sum() == reads.n_reads and eng.last_stats_ms() > 0
            del reads
        finally:
            eng.close()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info(0)[0]

    free = [cycle() for _ in range(6)]
    fall = free[0] - free[5]
    print(f"free MiB after each close: {[f // MIB for f in free]}; fall from the first to the sixth: {fall / MIB:.1f} MiB")
    assert fall < 128 * MIB, f"{fall / MIB:.1f} MiB"
