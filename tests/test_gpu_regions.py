"""The gold-standard assembly on the device (simmr_regions_plan / simmr_regions_emit, include/simmr_hip.h) against the numpy
restatement of the header's definition (tests/_regions.py).  depth[] is hand-built or random and handed straight to the pass;
the expected columns come from the model and the expected bases from the host copies of the staged contigs, so nothing
expected here comes from the pass under test.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import SimmrError, _abi
from simmr_amd.engine import Engine
from tests import _regions, _synth

pytestmark = pytest.mark.gpu
TILE, TOPS, RUN_TILE = _regions.constants()
LENS1 = [1, 15, 16, 17, 4095, 4096, 4097, 30_017, 123_457]  # region starts at every 2-bit offset and word phase
LEN0 = 70_000


def to_dev(eng, d):
    import torch
    return torch.from_numpy(np.ascontiguousarray(d, dtype=np.uint32).view(np.int32)).to(eng.device)


def new_engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine(0)


@pytest.fixture(scope="module")
def staged():
    """an engine of this module's own (depth[] covers every genome staged in an engine), three genomes, a reset"""
    eng = new_engine()
    rng = np.random.default_rng(21)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30000)].copy()  # (the contig of tests/test_gpu_depth.py)
    seq[rng.integers(0, 30000, 3000)] = ord("N")
    seq[rng.integers(0, 30000, 500)] = ord("-")
    seq[12_000:12_400] = ord("N")
    contigs = {0: _synth.synthetic_contigs([LEN0], 1), 1: _synth.synthetic_contigs(LENS1, 7), 3: [seq]}
    eng.stage_synthetic(0, [LEN0], 1)
    eng.stage_genome(1, contigs[1])
    eng.stage_genome(3, contigs[3])
    lens = {s: [int(c.size) for c in v] for s, v in contigs.items()}
    n = eng.depth_reset()
    assert n == sum(sum(v) for v in lens.values())
    yield eng, lens, contigs, n
    eng.close()


def check(eng, d, lens, contigs, min_depth=1, min_len=1, what=""):
    want = _regions.regions(d, lens, min_depth, min_len)
    got = eng.regions(min_depth, min_len, depth=to_dev(eng, d))
    _regions.assert_regions(got, want, what)
    seq = got["seq"].cpu().numpy()
    expect = _regions.bases(want, contigs)
    assert seq.dtype == np.uint8 and seq.shape == expect.shape and np.array_equal(seq, expect), (what, np.flatnonzero(seq != expect)[:8])
    return want


# ---- (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_len", [1, 2, 50])
@pytest.mark.parametrize("min_depth", [1, 3])
@pytest.mark.parametrize("p", [0.05, 0.5, 0.95])
def test_random_depth(staged, p, min_depth, min_len):
    eng, lens, contigs, n = staged
    rng = np.random.default_rng(int(p * 100) * 7 + min_depth * 3 + min_len)
    d = np.where(rng.random(n) < p, min_depth + rng.integers(0, 4, n), rng.integers(0, min_depth, n)).astype(np.uint32)
    want = check(eng, d, lens, contigs, min_depth, min_len, (p, min_depth, min_len))
    if min_len == 1:
        assert int(want["len"].sum()) == int((d >= min_depth).sum()) and want["len"].size > 1000


# ---- (b), (c) -----------------------------------------------------------------------------------------------------------
def test_nothing_covered(staged):
    eng, lens, contigs, n = staged
    got = eng.regions(depth=to_dev(eng, np.zeros(n, dtype=np.uint32)))
    assert all(got[k].size == 0 for k in ("genome", "contig", "start", "len", "depth_sum")) and got["seq_off"].tolist() == [0] and got["seq"].numel() == 0


def test_everything_covered_is_one_region_per_contig(staged):
    eng, lens, contigs, n = staged
    want = check(eng, np.full(n, 2, dtype=np.uint32), lens, contigs, 2, 1, "all covered")
    assert want["len"].tolist() == [LEN0] + LENS1 + [30000] and want["start"].max() == 0  # adjacent covered contigs are not merged
    assert want["depth_sum"].tolist() == [2 * x for x in want["len"].tolist()]


# ---- (d) ----------------------------------------------------------------------------------------------------------------
def test_threshold_is_inclusive(staged):
    eng, lens, contigs, n = staged
    rng = np.random.default_rng(4)
    d = (4 + rng.integers(0, 2, n)).astype(np.uint32)  # 4 and 5 side by side
    want = check(eng, d, lens, contigs, 5, 1, "d and d - 1")
    assert int(want["len"].sum()) == int((d == 5).sum())
    check(eng, d, lens, contigs, 4, 1, "all at or above")
    assert eng.regions(6, 1, depth=to_dev(eng, d))["len"].size == 0


# ---- (e), (f), (g) --------------------------------------------------------------------------------------------------------
def test_single_positions_on_every_edge(staged):
    eng, lens, contigs, n = staged
    _, _, first = _regions.layout(lens)
    d = np.zeros(n, dtype=np.uint32)
    at = [0, n - 1, TILE - 1, TILE, 2 * TILE - 1, 5 * TILE]
    for f in first[1:-1]:
        at += [int(f) - 1, int(f)]  # both sides of every contig boundary (the 1-base contig is both at once)
    d[at] = 7
    want = check(eng, d, lens, contigs, 1, 1, "single positions")
    assert want["len"].max() <= 2 and int(want["len"].sum()) == len(set(at))
    # covered on both sides of a boundary: two regions
    k = np.flatnonzero((want["start"] == 0) & (want["genome"] == 3))
    assert k.size == 1 and int(want["len"][k[0]]) == 1 and int(want["len"][k[0] - 1]) == 1


def test_long_runs_and_the_length_threshold(staged):
    eng, lens, contigs, n = staged
    d = np.zeros(n, dtype=np.uint32)
    d[100:100 + 3 * TILE + 5] = 3            # one run over four tiles
    d[20_000:20_050] = 1                     # exactly min_len
    d[21_000:21_049] = 1                     # min_len - 1
    d[TILE * 6 - 25:TILE * 6 + 25] = 9       # min_len across a tile boundary
    want = check(eng, d, lens, contigs, 1, 50, "min_len")
    assert want["len"].tolist() == [3 * TILE + 5, 50, 50] and want["start"].tolist() == [100, 20_000, TILE * 6 - 25]
    assert check(eng, d, lens, contigs, 1, 1, "all runs")["len"].size == 4


def test_alternating_positions_give_the_most_runs(staged):
    eng, lens, contigs, n = staged
    d = np.zeros(n, dtype=np.uint32)
    d[0:2 * TILE:2] = 1                      # 1, 0, 1, 0 over two tiles: sixteen regions per chunk of the base stream
    d[3 * TILE + 1:4 * TILE:2] = 1           # ... and in the other phase
    want = check(eng, d, lens, contigs, 1, 1, "alternating")
    assert want["len"].size == TILE + TILE // 2 and want["len"].max() == 1


# ---- (h) ----------------------------------------------------------------------------------------------------------------
def test_more_tiles_than_one_scan_iteration():
    n = TOPS * TILE + TILE + 77
    eng = new_engine()
    try:
        import torch
        try:
            eng.stage_synthetic(0, [n], 5)
            assert eng.depth_reset() == n
            contigs = {0: _synth.synthetic_contigs_chunked([n], 5)}
            rng = np.random.default_rng(8)
            d = np.zeros(n, dtype=np.uint32)
            for a, m in zip(rng.integers(0, n - 3000, 300), rng.integers(1, 3000, 300)):
                d[a:a + m] += 1
            d[TOPS * TILE - 3:TOPS * TILE + 3] = 2  # across the seam of the scan's iterations
            d[n - 5:] = 1
            dev = to_dev(eng, d)
        except (SimmrError, MemoryError, torch.cuda.OutOfMemoryError) as e:
            if isinstance(e, SimmrError) and e.code != _abi.ENOMEM:
                raise
            pytest.skip("the memory cannot be had")
        lens = {0: [n]}
        for md in (1, 2):
            want = _regions.regions(d, lens, md, 1)
            got = eng.regions(md, 1, depth=dev)
            _regions.assert_regions(got, want, ("many tiles", md))
            assert np.array_equal(got["seq"].cpu().numpy(), _regions.bases(want, contigs))
        assert int(want["start"][-1]) + int(want["len"][-1]) > TOPS * TILE
    finally:
        eng.close()


# ---- (i) ----------------------------------------------------------------------------------------------------------------
def test_bases_are_the_strains():
    eng = new_engine()
    try:
        rng = np.random.default_rng(6)
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 9000)].copy()
        seq[rng.integers(0, 9000, 400)] = ord("N")
        original = {0: [seq, _synth.synthetic_contigs([4097], 3)[0]]}
        eng.stage_genome(0, original[0])
        n_sites = eng.strain(0, 0.9, 99, sites=False)
        strain = {0: [eng.unstage(0, c, 0, original[0][c].size) for c in range(2)]}
        assert n_sites > 500 and sum(int((a != b).sum()) for a, b in zip(original[0], strain[0])) == n_sites
        n = eng.depth_reset()
        d = np.ones(n, dtype=np.uint32)
        d[5000:5003] = 0
        lens = {0: [9000, 4097]}
        want = check(eng, d, lens, strain, 1, 1, "strain")
        assert want["len"].tolist() == [5000, 3997, 4097]
        got = eng.regions(depth=to_dev(eng, d))["seq"].cpu().numpy()
        assert not np.array_equal(got, _regions.bases(want, original))
    finally:
        eng.close()


# ---- (j) ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    eng = new_engine()
    try:
        eng.stage_synthetic(0, [5000, 300], 2)
        contigs = {0: _synth.synthetic_contigs([5000, 300], 2)}
        d = np.zeros(5300, dtype=np.uint32)
        d[10:40] = 1
        d[4990:5010] = 2
        dev = to_dev(eng, d)
        with pytest.raises(SimmrError) as ei:  # before a reset
            eng.regions_plan(dev)
        assert ei.value.code == _abi.ESTATE
        eng.depth_reset()
        for md, ml in ((0, 1), (1, 0)):
            with pytest.raises(SimmrError) as ei:
                eng.regions_plan(dev, md, ml)
            assert ei.value.code == _abi.EINVAL
        with pytest.raises(SimmrError) as ei:  # no plan yet
            eng.regions_emit(dev, _abi.RegionsOut())
        assert ei.value.code == _abi.ESTATE
        n, nb = eng.regions_plan(dev)
        assert (n, nb) == (3, 50)
        # small capacities: nothing written, the plan kept
        cols = {name: torch.full((n + 1,), -3, dtype=torch.int32 if t == np.uint32 else torch.int64, device=eng.device) for name, t in _regions.COLUMNS}
        seq = torch.full((64,), 0x5a, dtype=torch.uint8, device=eng.device)
        ptrs = [cols[name].data_ptr() for name, _ in _regions.COLUMNS]
        for out in (_abi.RegionsOut(*ptrs, n - 1, seq.data_ptr(), 64), _abi.RegionsOut(*ptrs, n, seq.data_ptr(), nb - 1),
                    _abi.RegionsOut(None, None, None, None, None, cols["seq_off"].data_ptr(), 0, None, 0)):
            with pytest.raises(SimmrError) as ei:
                eng.regions_emit(dev, out)
            assert ei.value.code == _abi.ERANGE
            assert all(bool((c == -3).all()) for c in cols.values()) and bool((seq == 0x5a).all())
        # seq == NULL skips the bases; a column that is NULL is skipped too
        want = _regions.regions(d, {0: [5000, 300]})
        eng.regions_emit(dev, _abi.RegionsOut(*ptrs, n, None, 0))
        got = {name: cols[name][: n + (name == "seq_off")].cpu().numpy().view(t) for name, t in _regions.COLUMNS}
        _regions.assert_regions(got, want, "columns alone")
        assert bool((seq == 0x5a).all()) and want["depth_sum"].tolist() == [30, 20, 20]
        eng.regions_emit(None, _abi.RegionsOut(None, None, None, None, None, None, 0, seq.data_ptr(), 64))  # the bases alone
        assert seq[:nb].cpu().numpy().tobytes() == _regions.bases(want, contigs).tobytes() and bool((seq[nb:] == 0x5a).all())
        # Engine.regions(seq=False)
        got = eng.regions(depth=dev, seq=False)
        assert got["seq"] is None
        _regions.assert_regions(got, want, "seq=False")
        # a reset or a staging call ends the plan
        eng.regions_plan(dev)
        eng.depth_reset()
        with pytest.raises(SimmrError) as ei:
            eng.regions_emit(dev, _abi.RegionsOut(*ptrs, n, None, 0))
        assert ei.value.code == _abi.ESTATE
        eng.regions_plan(dev)
        eng.stage_synthetic(1, [100], 3)
        for call in (lambda: eng.regions_emit(dev, _abi.RegionsOut(*ptrs, n, None, 0)), lambda: eng.regions_plan(dev)):
            with pytest.raises(SimmrError) as ei:  # after staging
                call()
            assert ei.value.code == _abi.ESTATE
    finally:
        eng.close()


# ---- (k) ----------------------------------------------------------------------------------------------------------------
def test_twice_gives_identical_bytes(staged):
    eng, lens, contigs, n = staged
    rng = np.random.default_rng(12)
    dev = to_dev(eng, (rng.random(n) < 0.6).astype(np.uint32) * rng.integers(1, 9, n).astype(np.uint32))
    a, b = eng.regions(2, 3, depth=dev), eng.regions(2, 3, depth=dev)
    for name, _ in _regions.COLUMNS:
        assert a[name].tobytes() == b[name].tobytes(), name
    assert a["seq"].cpu().numpy().tobytes() == b["seq"].cpu().numpy().tobytes() and a["len"].size > 1000
    assert eng.last_regions_ms() > 0
