"""The truth pass (simmr_truth_plan / simmr_truth_emit; k_truth<false> and k_truth<true> of truth_kernels.hip, the walker of
read_walk.hpp, the engine's scan) at its seams: windows and rounds full of edits, the last window's overlapped bytes, reads past
65 535 bases, the grid cap with a partial last batch and the scan's second trip, seq[] changed between plan and emit, each refusal of
the bounds check, and subsets of the output columns.  The columns are hand-built (tests/_truth_cases.py: bytes copied from the host
genome with chosen bytes altered; no simulator), what is expected is tests/_truth.model — the header's definition in numpy — over host
copies of the same columns, and every comparison is exact (tests/_truth.assert_truth).  tests/test_truth_host.py holds the builders to
the model without a GPU.  The engine is the module's own, with its own genomes in its own slots.

Which path each test is the first to enter:
  test_every_base_an_edit
      x.diff == 0xffff in every lane, a round that adds 256 to the cursor, 256 such rounds in a row (65 535 bases), next to reads
      with no edit and with one at offset 0, whose ranges an overrunning cursor would land in;
  test_edits_in_the_last_windows_overlap
      the overlapped bytes of the last window all edits: `keep` drops them there, the window before has them;
  test_reads_longer_than_65535_bases
      edit_pos above 65 535, 300 edits in a row over offset 65 535 and the start of a round;
  test_tiny_reads_past_the_grid_cap_and_the_scans_first_trip
      workgroups of k_truth in their third trip, five reads in the last batch (and a whole one), k_scan_tops' second trip with
      more than one tile: every read's offset and every edit compared;
  test_seq_changed_between_plan_and_emit
      the `o < limit` of the store loop;
  test_each_refusal_of_the_bounds_check
      so > so1, so1 > seq_capacity, len > so1 - so, lo > C.len, len > C.len - lo and a slot that is not staged, one read each;
  test_column_subsets
      one edit column alone, several without nm, nm alone."""
import ctypes as C
import time

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _truth
from tests import _stats_cases as sc
from tests import _truth_cases as tc

pytestmark = pytest.mark.gpu

COLS = ("nm", "edit_off", "edit_pos", "edit_ref", "edit_alt", "edit_qual")
EDIT_COLS = COLS[2:]
FILL = {"nm": -3, "edit_off": -5, "edit_pos": -7, "edit_ref": 0xA5, "edit_alt": 0xA6, "edit_qual": 0xA7}
CAN = 64  # canary entries on either side of every buffer


@pytest.fixture(scope="module")
def genomes():
    return tc.host_genomes()


@pytest.fixture(scope="module")
def own(genomes):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from simmr_amd.engine import Engine
    e = Engine(0)
    try:
        tc.stage(e, genomes)
        yield e
    finally:
        e.close()


@pytest.fixture(params=[0, 16], ids=["compact", "slot16"])
def layout(request):
    return request.param


def check(eng, oracle, genomes, host, dev, what):
    """the device truth of `dev` is the model of the host copy of the same columns"""
    want = _truth.model(oracle, host, genomes)
    got = eng.truth(dev).to_host()
    _truth.assert_truth(got, want, what)
    assert np.array_equal(got["nm"], np.diff(got["edit_off"].astype(np.int64)).astype(np.uint32)), what
    return got


class Canaried:
    """the six output columns for n reads and m edits, each filled with its own value and with CAN entries on either side"""

    def __init__(self, eng, n, m):
        import torch
        dtypes = {"nm": torch.int32, "edit_off": torch.int64, "edit_pos": torch.int32, "edit_ref": torch.uint8, "edit_alt": torch.uint8,
                  "edit_qual": torch.uint8}
        self.n, self.m = n, m
        self.count = {"nm": n, "edit_off": n + 1, "edit_pos": m, "edit_ref": m, "edit_alt": m, "edit_qual": m}
        self.bufs = {k: torch.full((CAN + self.count[k] + CAN,), FILL[k], dtype=dtypes[k], device=eng.device) for k in COLS}
        self.before = {k: v.clone() for k, v in self.bufs.items()}

    def out(self, given=COLS):
        ptr = lambda k: self.bufs[k].data_ptr() + CAN * self.bufs[k].element_size() if k in given else None
        return _abi.TruthOut(*[ptr(k) for k in COLS], self.n, self.m)

    def untouched(self, k):
        import torch
        return torch.equal(self.bufs[k], self.before[k])

    def inside(self, k):
        """column k without its canaries, after asserting that they are whole"""
        import torch
        t, cnt = self.bufs[k], self.count[k]
        assert torch.equal(t[:CAN], self.before[k][:CAN]) and torch.equal(t[CAN + cnt:], self.before[k][CAN + cnt:]), f"{k}: canary"
        return t[CAN:CAN + cnt].cpu().numpy()


def same(got, want):
    """a column as the device holds it (int32 / int64 for the unsigned ones) against the model's"""
    return np.array_equal(got.astype(want.dtype), want)


# ---- 1. every base an edit -----------------------------------------------------------------------------------------------------
def test_every_base_an_edit(own, oracle, genomes, layout):
    case = tc.dense_reads(oracle)
    L = case.L
    dense = np.array([k == "dense" for k in case.kinds])
    assert L[dense].max() == 65535 == 256 * tc.ROUND - 1 and (L[dense] == 65535).sum() == 4   # 256 rounds of a row
    assert {tc.ROUND - 1, tc.ROUND, tc.ROUND + 1} <= set(L[dense].tolist())                                          # one round, and one group more
    got = check(own, oracle, genomes, case.host, sc.device_reads(case.host, layout, own.device), "every base an edit")
    off = got["edit_off"].astype(np.int64)
    for r in np.flatnonzero(dense):
        assert got["nm"][r] == L[r] and np.array_equal(got["edit_pos"][off[r]:off[r + 1]], np.arange(L[r], dtype=np.uint32)), f"read {r}"
    assert got["nm"][~dense].tolist() == [0 if k == "clean" else 1 for k in case.kinds if k != "dense"]


# ---- 2. the last window's overlapped bytes -------------------------------------------------------------------------------------
def test_edits_in_the_last_windows_overlap(own, oracle, genomes, layout):
    case = tc.overlap_reads(oracle)
    got = check(own, oracle, genomes, case.host, sc.device_reads(case.host, layout, own.device), "the last window's overlap")
    off = got["edit_off"].astype(np.int64)
    for r, at in enumerate(case.at):  # exactly those offsets, once, ascending
        assert got["edit_pos"][off[r]:off[r + 1]].tolist() == at.tolist(), f"read {r}"


# ---- 3. reads longer than 65 535 bases -----------------------------------------------------------------------------------------
def test_reads_longer_than_65535_bases(own, oracle, genomes, layout):
    case = tc.long_reads(oracle)
    L = np.diff(case.host["seq_off"].astype(np.int64))
    assert L.min() > 65535 and L.max() == 70000 == genomes[tc.RANDOM].contigs[tc.LONG_CONTIG].size
    got = check(own, oracle, genomes, case.host, sc.device_reads(case.host, layout, own.device), "reads past 65 535 bases")
    assert int(got["edit_pos"].max()) == 69999 and (got["edit_pos"] > 65535).sum() > 300


# ---- 4. past the grid cap, a partial last batch, the scan's second trip --------------------------------------------------------
@pytest.mark.parametrize("last", ["partial", "whole"])
def test_tiny_reads_past_the_grid_cap_and_the_scans_first_trip(own, oracle, genomes, last):
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    n = tc.tiny_n(cus) - (0 if last == "partial" else 5)
    s = tc.tiny_shape(n, cus)
    assert s.grid == cus * tc.WGS_PER_CU < s.batches, "resize: the grid must be capped"
    assert s.trips >= 3 and s.batches - 1 >= 2 * s.grid, "resize: the last batch must be of a third trip"
    assert s.last == (5 if last == "partial" else tc.WG_READS)
    assert s.scan_tiles > tc.SCAN_THREADS + 1, "resize: the second trip of k_scan_tops must hold more than one tile"
    units = tc.tiny_units(oracle)
    models = [_truth.model(oracle, u, genomes) for u in units]   # the per-read loop runs over the units alone
    order = tc.unit_order(s.batches, len(units))
    for shift in (1, s.grid, 2 * s.grid):  # a batch, or a trip, later is another unit more often than not
        assert (order[shift:] != order[:-shift]).mean() > 0.5
    t0 = time.perf_counter()
    dev = tc.device_sequenced(units, order, n, own.device)
    host = tc.host_sequenced(units, order, n)
    raw = dev.raw_to_host()
    for name in sc.SMALL + ("seq_off",):
        assert np.array_equal(raw[name], host[name]), name
    total = int(host["seq_off"][n])
    assert np.array_equal(raw["seq"][:total], host["seq"]) and np.array_equal(raw["qual"][:total], host["qual"])
    want = tc.assembled(models, order, n)
    got = own.truth(dev).to_host()
    _truth.assert_truth(got, want, f"{n} tiny reads")
    assert np.array_equal(got["nm"], np.diff(got["edit_off"].astype(np.int64)).astype(np.uint32))
    print(f"{n} tiny reads, {s.batches} batches on {s.grid} workgroups, {s.scan_tiles} scan tiles, {want['edit_pos'].size} edits: "
          f"{time.perf_counter() - t0:.2f} s")


# ---- 5. seq[] changed between plan and emit ------------------------------------------------------------------------------------
def within_the_plan(planned, now):
    """What an emit leaves when seq[] is no longer what the plan counted: nm and edit_off are the plan's, and a read's range
    holds the first `planned` of its edits now, in ascending order; entries past those it has now keep their fill value."""
    a, b = planned["edit_off"].astype(np.int64), now["edit_off"].astype(np.int64)
    m = int(a[-1])
    out = {k: np.full(m, FILL[k] & 0xFFFFFFFF if k == "edit_pos" else FILL[k], dtype=planned[k].dtype) for k in EDIT_COLS}
    for r in range(len(planned["nm"])):
        k = int(min(a[r + 1] - a[r], b[r + 1] - b[r]))
        for col in EDIT_COLS:
            out[col][a[r]:a[r] + k] = now[col][b[r]:b[r] + k]
    return out


def test_seq_changed_between_plan_and_emit(own, oracle, genomes, layout):
    import torch
    case = tc.small_reads(oracle)
    host = case.host
    dev = sc.device_reads(host, layout, own.device)
    n = dev.n_reads
    planned = _truth.model(oracle, host, genomes)
    m = own.truth_plan(dev)
    assert m == int(planned["nm"].sum()) == sum(case.planned)
    off = host["seq_off"].astype(np.int64)
    first = dev.seq_off[:n].cpu().numpy()   # a read's first base, in either layout
    lib, h, pod = own.lib, own._h, dev.pod()

    def emitted(now_host, what):
        now = _truth.model(oracle, now_host, genomes)
        c = Canaried(own, n, m)
        out = c.out()
        assert lib.simmr_truth_emit(h, C.byref(pod), C.byref(out)) == _abi.OK, what
        torch.cuda.synchronize()
        assert same(c.inside("nm"), planned["nm"]) and same(c.inside("edit_off"), planned["edit_off"]), what
        want = within_the_plan(planned, now)
        for col in EDIT_COLS:   # nothing outside a read's range: the canaries, and every other read's range exact
            got = c.inside(col).astype(want[col].dtype)
            assert np.array_equal(got, want[col]), f"{what}: {col} differs first at {int(np.flatnonzero(got != want[col])[0])}"
        return now

    # more edits than planned: a read that planned none, one with several, the last read
    more = {0: [2, 20, 39], 5: [0, 6], 8: [0, 10, 49]}
    assert case.planned[0] == 0 and case.planned[5] > 1 and max(more) == n - 1
    changed = dict(host, seq=host["seq"].copy())
    for r, at in more.items():
        for j in at:
            changed["seq"][off[r] + j] = sc.stepped(host["seq"][off[r] + j], 1 + j % 3)
            dev.seq[int(first[r]) + j] = int(changed["seq"][off[r] + j])
    now = emitted(changed, "more edits than planned")
    assert [int(now["nm"][r]) - case.planned[r] for r in more] == [len(at) for at in more.values()]
    assert sum(len(at) for at in more.values()) < CAN   # (a store past the last read's range would still land in the canary)
    # the bytes put back, and one edit of read 2 taken away: its last entry keeps the fill value
    r, j = 2, 16
    fewer = dict(host, seq=host["seq"].copy())
    fewer["seq"][off[r] + j] = sc.expected(oracle, genomes, tc.RANDOM, 0, int(host["start"][r]), 64, 0)[j]
    assert fewer["seq"][off[r] + j] != host["seq"][off[r] + j]
    for rr, at in more.items():
        for jj in at:
            dev.seq[int(first[rr]) + jj] = int(host["seq"][off[rr] + jj])
    dev.seq[int(first[r]) + j] = int(fewer["seq"][off[r] + j])
    now = emitted(fewer, "an edit fewer than planned")
    assert int(now["nm"][r]) == case.planned[r] - 1
    # as planned again
    dev.seq[int(first[r]) + j] = int(host["seq"][off[r] + j])
    emitted(host, "the planned bytes")


# ---- 6. the bounds check, branch by branch -------------------------------------------------------------------------------------
def test_each_refusal_of_the_bounds_check(own, oracle, genomes, layout):
    import torch
    case = tc.small_reads(oracle)
    host, clen = case.host, case.clen
    dev = sc.device_reads(host, layout, own.device)
    n = dev.n_reads
    L = np.diff(host["seq_off"].astype(np.int64))
    # (taken: read 3 and read 6 end exactly at their contig's end, read 4 has no base at lo == the contig's length)
    check(own, oracle, genomes, host, dev, "before")
    m = own.truth_plan(dev)
    assert m == sum(case.planned) > 0
    lib, h = own.lib, own._h
    so = dev.seq_off.cpu().numpy().astype(np.int64)
    canaried = Canaried(own, n, m)

    def refused(what, pod=None):
        pod = dev.pod() if pod is None else pod
        total = C.c_uint64(0)
        assert lib.simmr_truth_plan(h, C.byref(pod), n, C.byref(total)) == _abi.EINVAL, what
        assert b"not staged" in lib.simmr_last_error(h), what   # the device's bounds check answered, through the error word
        out = canaried.out()
        assert lib.simmr_truth_emit(h, C.byref(pod), C.byref(out)) == _abi.ESTATE, what
        torch.cuda.synchronize()
        assert all(canaried.untouched(k) for k in COLS), what

    def altered(entries, what):
        """the entries (column, read, value) written, the plan refused, the entries put back, the plan as before"""
        keep = [int(column[r]) for column, r, _ in entries]
        for column, r, value in entries:
            column[r] = int(value)
        try:
            refused(what)
        finally:
            for (column, r, _), was in zip(entries, keep):
                column[r] = was
        assert own.truth_plan(dev) == m, f"after {what}"

    r = 2  # a forward read in the middle, with reads of more bases behind it
    assert 0 < r < n - 1 and L[r] == 64
    altered([(dev.seq_off, r + 1, so[r] + L[r] - 1)], "len > so1 - so")
    assert so[r + 1] + 1 + L[r] <= dev.seq.numel()   # (read without the check, the bytes would still be the tensor's)
    altered([(dev.seq_off, r, so[r + 1] + 1)], "so > so1")
    # so1 > seq_capacity: the capacity in the pod one less than seq_off[n], the tensors as they are.  No host check looks at it
    # (check_read_columns asks for the pointers alone): the device's check answers
    pod = dev.pod()
    assert pod.seq_capacity == so[n] == dev.seq.numel()
    pod.seq_capacity = int(so[n]) - 1
    refused("so1 > seq_capacity", pod)
    assert own.truth_plan(dev) == m
    # len > C.len - lo: lo = C.len - L + 1, forward and reverse (the contig is not its genome's last: the base past its end is staged)
    assert int(host["end"][3]) == clen and L[3] == 150 and host["flags"][3] == 0
    altered([(dev.start, 3, clen - L[3] + 1), (dev.end, 3, clen + 1)], "len > C.len - lo, forward")
    assert int(host["start"][6]) == clen and L[6] == 33 and host["flags"][6] == 1
    altered([(dev.end, 6, clen - L[6] + 1), (dev.start, 6, clen + 1)], "len > C.len - lo, reverse")
    # lo > C.len, with no base
    assert L[4] == 0 and int(host["start"][4]) == int(host["end"][4]) == clen
    altered([(dev.start, 4, clen + 1), (dev.end, 4, clen + 1)], "lo > C.len")
    # a slot below n_genomes that was never staged (a slot above it is)
    assert tc.UNSTAGED < tc.HOMOPOLYMER and tc.UNSTAGED not in genomes
    altered([(dev.genome, 1, tc.UNSTAGED)], "a slot that is not staged")
    check(own, oracle, genomes, host, dev, "after")


# ---- 7. column subsets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [("edit_off", "edit_pos"), ("edit_off", "edit_qual"), ("edit_off", "edit_ref", "edit_alt"), ("nm",)],
                         ids=lambda g: "+".join(g))
def test_column_subsets(own, oracle, genomes, layout, given):
    import torch
    case = tc.small_reads(oracle)
    dev = sc.device_reads(case.host, layout, own.device)
    full = check(own, oracle, genomes, case.host, dev, "all columns")
    n, m = dev.n_reads, own.truth_plan(dev)
    assert m == full["edit_pos"].size > 0
    c = Canaried(own, n, m)
    out, pod = c.out(given), dev.pod()
    assert own.lib.simmr_truth_emit(own._h, C.byref(pod), C.byref(out)) == _abi.OK
    torch.cuda.synchronize()
    for k in COLS:
        if k in given:
            assert same(c.inside(k), full[k]), k
        else:
            assert c.untouched(k), f"{k} was not passed and was written"
