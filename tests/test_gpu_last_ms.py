"""Every Engine.last_*_ms through its states: refused before the first timed call (ESTATE, the library's own words), a finite
time above zero behind the first phase, no less behind each later phase, and back to the first phase's span alone behind the
call that makes the later phases stale.  Two synthetic contigs of 1 kb, 64 minimal-short pairs, one engine per test.

The messages are those of the sources before the timing went through host_support.hpp's Spans (depth.hip, strain.hip,
regions.hip, pileup.hip, fit.hip, overlap.hip, record_stream_host.hpp with each writer's F::PLAN, and the truth and statistics
sections engine.hip had then).  That a time is above zero behind a unit's first use is also asserted, each in its own run, by
test_gpu_stats.py, test_gpu_depth.py, test_gpu_fit.py, test_gpu_sam.py, test_gpu_bam.py, test_gpu_bam_sorted.py,
test_gpu_regions.py, test_gpu_strain.py, test_gpu_overlap.py and test_gpu_sam_sort.py; here that value is the one the later
states are compared with, so the row stays."""
import ctypes as C
import math

import numpy as np
import pytest

from simmr_amd import MinimalShortErrorProfile, _abi
from simmr_amd._abi import SimmrError
from simmr_amd.engine import Truth

pytestmark = pytest.mark.gpu

RNAMES = [(0, ["c0", "c1"])]


class Run:
    """an engine of its own with the reads staged and emitted, and the calls the phases are made of"""

    def __init__(self):
        import torch
        from simmr_amd.engine import Engine
        self.torch = torch
        self.eng = eng = Engine(0)
        eng.stage_synthetic(0, [1000, 1000], 1)
        self.reads = eng.simulate_pe_reads_from_genome(0, MinimalShortErrorProfile().pod(), 64, 42, qual_offset=33)
        assert self.reads.n_reads > 0
        self.lib, self.h = eng.lib, eng._h

    def close(self):
        self.eng.close()

    def empty(self, n, dtype):
        return self.torch.empty(max(int(n), 1), dtype=dtype, device=self.eng.device)

    def truth_columns(self, n_edits):
        t, n = self.torch, self.reads.n_reads
        return Truth(nm=self.empty(n, t.int32), edit_off=self.empty(n + 1, t.int64), edit_pos=self.empty(n_edits, t.int32),
                     edit_ref=self.empty(n_edits, t.uint8), edit_alt=self.empty(n_edits, t.uint8), edit_qual=self.empty(n_edits, t.uint8),
                     n_reads=n, n_edits=n_edits)

    def truth_emit(self, tr, reads_capacity=None):
        out, pod = tr.pod(), self.reads.pod()
        if reads_capacity is not None:
            out.reads_capacity = reads_capacity
        self.eng._check(self.lib.simmr_truth_emit(self.h, C.byref(pod), C.byref(out)))


@pytest.fixture()
def run():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = Run()
    yield r
    r.close()


def refused(call, message):
    with pytest.raises(SimmrError) as ei:
        call()
    assert ei.value.code == _abi.ESTATE and ei.value.msg == message, (ei.value.code, ei.value.msg)


def first(call):
    v = call()
    assert math.isfinite(v) and v > 0, v
    return v


def no_less(call, before):
    v = call()
    assert math.isfinite(v) and v >= before, (v, before)
    return v


def fallen_back(call):
    """the first phase's span alone: one pair of events, so the same number however often it is read"""
    v = first(call)
    assert call() == v
    return v


def test_truth(run):
    eng = run.eng
    refused(eng.last_truth_ms, "no truth plan yet")
    n_edits = eng.truth_plan(run.reads)
    plan = first(eng.last_truth_ms)
    tr = run.truth_columns(n_edits)
    run.truth_emit(tr)
    both = no_less(eng.last_truth_ms, plan)
    assert eng.last_truth_ms() == both
    with pytest.raises(SimmrError) as ei:  # an emit that fails adds nothing: the plan's span, which no call has recorded anew
        run.truth_emit(tr, reads_capacity=run.reads.n_reads - 1)
    assert ei.value.code == _abi.ERANGE
    assert fallen_back(eng.last_truth_ms) == plan
    run.truth_emit(tr)
    no_less(eng.last_truth_ms, plan)


def test_truth_plan_does_not_outlive_a_staging(run):
    eng = run.eng
    n_edits = eng.truth_plan(run.reads)
    first(eng.last_truth_ms)
    eng.stage_synthetic(1, [500], 3)  # any slot: the staging epoch counts on
    refused(lambda: run.truth_emit(run.truth_columns(n_edits)), "simmr_truth_emit called without a simmr_truth_plan for these columns")
    refused(eng.last_truth_ms, "no truth plan yet")
    eng.truth_plan(run.reads)  # and a new plan is in force again
    first(eng.last_truth_ms)


def test_stats(run):
    eng = run.eng
    refused(eng.last_stats_ms, "no simmr_stats_add yet")
    eng.stats_reset()
    refused(eng.last_stats_ms, "no simmr_stats_add yet")
    eng.stats_add(run.reads, 2)
    fallen_back(eng.last_stats_ms)
    assert eng.stats()["reads"].sum() == run.reads.n_reads
    eng.stats_reset()  # the add's span went with the tables
    refused(eng.last_stats_ms, "no simmr_stats_add yet")


def test_depth(run):
    eng = run.eng
    refused(eng.last_depth_ms, "no simmr_depth_add yet")
    eng.depth_reset()
    refused(eng.last_depth_ms, "no simmr_depth_add yet")
    eng.depth_add(run.reads)
    add = first(eng.last_depth_ms)
    d = eng.depth()
    emitted = no_less(eng.last_depth_ms, add)
    eng.depth_summary(window=100, depth=d)
    no_less(eng.last_depth_ms, emitted)
    eng.depth_add(run.reads)  # the scan and the summary are of fewer reads than were added
    fallen_back(eng.last_depth_ms)
    eng.depth_reset()
    refused(eng.last_depth_ms, "no simmr_depth_add yet")


def regions_out(run, n, nb):
    t = run.torch
    dt = {np.uint32: t.int32, np.uint64: t.int64}
    cols = {name: run.empty(n + 1, dt[ty]) for name, ty in run.eng.REGION_COLUMNS}
    bases = run.empty((nb + 15) // 16 * 16 + 16, t.uint8)
    out = _abi.RegionsOut(*[cols[name].data_ptr() for name, _ in run.eng.REGION_COLUMNS], n, bases.data_ptr(), bases.numel())
    out._keep = (cols, bases)
    return out


def test_regions(run):
    eng = run.eng
    refused(eng.last_regions_ms, "no simmr_regions_plan yet")
    eng.depth_reset()
    eng.depth_add(run.reads)
    d = eng.depth()
    refused(eng.last_regions_ms, "no simmr_regions_plan yet")
    n, nb = eng.regions_plan(d, 1, 1)
    assert n > 0
    plan = first(eng.last_regions_ms)
    eng.regions_emit(d, regions_out(run, n, nb))
    no_less(eng.last_regions_ms, plan)
    eng.regions_plan(d, 2, 1)  # another plan: the emit behind the last one is not of it
    fallen_back(eng.last_regions_ms)


def test_strain(run):
    eng = run.eng
    refused(eng.last_strain_ms, "no simmr_strain_plan yet")
    assert eng.strain_plan(0, 0.9, 7) > 0
    plan = first(eng.last_strain_ms)
    eng._check(eng.lib.simmr_strain_apply(eng._h, 0, None))
    no_less(eng.last_strain_ms, plan)
    eng.strain_plan(0, 0.95, 8)  # another plan: nothing of it has been applied
    fallen_back(eng.last_strain_ms)


def test_pileup(run):
    eng = run.eng
    refused(eng.last_pileup_ms, "no simmr_pileup_add yet")
    eng.pileup_reset(np.zeros(3, np.uint32), np.array([0, 0, 1], np.uint32), np.array([10, 500, 20], np.uint64))
    refused(eng.last_pileup_ms, "no simmr_pileup_add yet")
    eng.pileup_add(run.reads)
    fallen_back(eng.last_pileup_ms)
    eng.pileup_reset(np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.array([10], np.uint64))
    refused(eng.last_pileup_ms, "no simmr_pileup_add yet")


def test_fit(run):
    eng = run.eng
    refused(eng.last_fit_ms, "no simmr_fit_add yet")
    eng.fit_reset(k=5, pair_capacity=1 << 12)
    refused(eng.last_fit_ms, "no simmr_fit_add yet")
    eng.fit_add(run.reads, 2)
    fallen_back(eng.last_fit_ms)
    eng.fit_reset(k=5, pair_capacity=1 << 12)
    refused(eng.last_fit_ms, "no simmr_fit_add yet")


def test_overlap(run):
    eng = run.eng
    refused(eng.last_overlap_ms, "no simmr_overlap_plan yet")
    eng.overlap_reset(True)
    eng.overlap_add(run.reads)
    refused(eng.last_overlap_ms, "no simmr_overlap_plan yet")
    n, pairs, total = eng.overlap_plan(25)
    assert n == run.reads.n_reads and total > 0
    plan = fallen_back(eng.last_overlap_ms)
    text = run.empty(total, run.torch.uint8)
    eng._check(eng.lib.simmr_overlap_emit(eng._h, 0, n, None, C.c_void_p(text.data_ptr()), total))
    both = no_less(eng.last_overlap_ms, plan)
    assert eng.last_overlap_ms() == both
    eng.overlap_plan(25)  # a plan starts the sum of its emits anew
    fallen_back(eng.last_overlap_ms)


WRITERS = {
    "sam": ("simmr_sam_plan", "simmr_sam_emit", "last_sam_ms", 0),
    "sam_sorted": ("simmr_sam_sort_plan", "simmr_sam_sort_emit", "last_sam_sort_ms", 2),
    "bam": ("simmr_bam_plan", "simmr_bam_emit", "last_bam_ms", 0),
    "bam_sorted": ("simmr_bam_sort_plan", "simmr_bam_sort_emit", "last_bam_sort_ms", 3),
}


@pytest.mark.parametrize("writer", sorted(WRITERS))
def test_record_writers(run, writer):
    eng = run.eng
    plan_name, emit_name, ms_name, n_extra = WRITERS[writer]
    last_ms = getattr(eng, ms_name)
    refused(last_ms, f"no {plan_name} yet")
    handle = eng._h
    if writer == "bam_sorted":  # the handle is made on first use: without it the wrapper refuses, with it the library does
        handle = eng._bam_sort_handle()
        refused(last_ms, f"no {plan_name} yet")
    tr = eng.truth(run.reads)
    out, pod, sn, total = tr.pod(), run.reads.pod(), eng._sam_names(RNAMES), C.c_uint64(0)

    def plan():
        eng._check(getattr(eng.lib, plan_name)(handle, C.byref(sn), C.byref(pod), C.byref(out), run.reads.n_reads, 1, C.byref(total)))
    plan()
    assert total.value > 0
    planned = fallen_back(last_ms)
    dst = run.empty(total.value, run.torch.uint8)
    eng._check(getattr(eng.lib, emit_name)(handle, C.byref(pod), C.byref(out), C.c_void_p(dst.data_ptr()), total.value, *([None] * n_extra)))
    both = no_less(last_ms, planned)
    assert last_ms() == both
    plan()  # another plan: the emit behind the last one is not of it
    fallen_back(last_ms)
