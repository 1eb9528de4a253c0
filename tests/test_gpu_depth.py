"""Coverage depth on the device (simmr_depth_reset / _add / _emit / _summarize, include/simmr_hip.h) against the numpy
restatement of the header's definition (tests/_depth.py), applied to the ORACLE's columns; the device reads are first shown
to be the oracle's, so nothing expected here comes from the pass under test.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import MinimalLongErrorProfile, MinimalShortErrorProfile, SimmrError, _abi
from simmr_amd.engine import Engine, Reads
from tests import _depth, _oracle, _synth
from tests._hand_built import hand_built
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu
COLS = ("seq_off", "start", "end", "contig", "flags", "qual", "seq")
TILE, TOPS = _depth.constants()
LENS1 = [300_000, 90_001, 30_017, 70_000, 123_457]


@pytest.fixture(scope="module")
def deng():
    """an engine of this module's own: depth[] covers every genome staged in an engine, so the layout must be known"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def genomes(deng):
    # (the genomes of tests/test_gpu_stats.py)
    rng = np.random.default_rng(21)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30000)].copy()
    seq[rng.integers(0, 30000, 3000)] = ord("N")
    seq[rng.integers(0, 30000, 500)] = ord("-")
    seq[12_000:12_400] = ord("N")
    g = {0: _oracle.HostGenome(_synth.synthetic_contigs([1_000_000], 1)),
         1: _oracle.HostGenome(_synth.synthetic_contigs(LENS1, 7)),
         3: _oracle.HostGenome([seq])}
    deng.stage_synthetic(0, [1_000_000], 1)
    deng.stage_genome(1, g[1].contigs)
    deng.stage_genome(3, g[3].contigs)
    return g


@pytest.fixture(scope="module")
def lens(genomes):
    return {s: [int(c.size) for c in g.contigs] for s, g in genomes.items()}


@pytest.fixture(params=[0, 16], ids=["compact", "slot16"])
def layout(request, deng):
    deng.set_read_slots(request.param)
    try:
        yield request.param
    finally:
        deng.set_read_slots(0)


def column_reads(device, cols):
    """Reads that carry start, end, contig and genome only (the other columns are never read by the depth pass)"""
    import torch
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(device)
    n = len(cols["start"])
    dummy = torch.zeros(16, dtype=torch.uint8, device=device)
    return Reads(seq=dummy, qual=dummy, seq_off=torch.zeros(n + 1, dtype=torch.int64, device=device), start=t(cols["start"], np.int64),
                 end=t(cols["end"], np.int64), contig=t(cols["contig"], np.int32), genome=t(cols["genome"], np.int32),
                 read_id=torch.zeros(max(n, 1), dtype=torch.int32, device=device), flags=torch.zeros(max(n, 1), dtype=torch.uint8, device=device),
                 n_reads=n, total_bases=0)


def make_cols(reads):
    """[(genome, contig, lo, L, reverse)] -> columns"""
    g, c, lo, L, rev = (np.array(x, dtype=np.int64) for x in zip(*reads))
    return {"start": np.where(rev == 1, lo + L, lo).astype(np.uint64), "end": np.where(rev == 1, lo, lo + L).astype(np.uint64),
            "contig": c.astype(np.uint32), "genome": g.astype(np.uint32)}


def cat(*cols):
    return {k: np.concatenate([c[k] for c in cols]) for k in ("start", "end", "contig", "genome")}


def device_depth(eng, *reads):
    eng.depth_reset()
    for r in reads:
        eng.depth_add(r)
    return eng.depth()


def check_all(eng, d_dev, cols, lens, windows, what):
    want = _depth.depth(cols, lens)
    got = d_dev.cpu().numpy()
    assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8])
    for w in windows:
        s = eng.depth_summary(w, d_dev)
        _depth.assert_summary(s, _depth.summary(want, lens, w), f"{what}, window {w}")
    L = np.abs(cols["end"].astype(np.int64) - cols["start"].astype(np.int64))
    assert int(s["depth_sum"].sum()) == int(L.sum()) and int(s["hist"].sum()) == want.size
    return want, s


# ---- 1 ----------------------------------------------------------------------------------------------------------------
def test_minimal_short_pairs(deng, oracle, genomes, lens, layout):
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX).pod()
    for gidx, reads, seed, first, count in ((1, 3001, 5, 0, _abi.U64_MAX), (0, 8000, 42, 1100, 900)):
        dev = deng.simulate_pe_reads_from_genome(gidx, prof, reads, seed, first=first, count=count, qual_offset=33)
        o = _oracle.simulate_pe(oracle, genomes[gidx], prof, reads, seed, first=first, count=count, qual_offset=33).trimmed()
        h = dev.to_host()
        assert_same(h, o, cols=COLS)
        o = dict(o, genome=h["genome"])
        want, s = check_all(deng, device_depth(deng, dev), o, lens, (0, 1000), f"genome {gidx} first {first}")
        assert want.max() >= 2 and s["covered"].sum() > 0 and deng.last_depth_ms() > 0


# ---- 2 ----------------------------------------------------------------------------------------------------------------
def test_long_reads_two_genomes(deng, oracle, genomes, lens, layout):
    lp = MinimalLongErrorProfile(gamma_mean=3000.0, gamma_std=2500.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    dev = deng.simulate_long_reads([1, 0], [150, 100], lp, 3, qual_offset=33)
    o = _oracle.simulate_long(oracle, [genomes[1], genomes[0]], [150, 100], lp, 3, qual_offset=33).trimmed()
    h = dev.to_host()
    assert_same(h, o, cols=COLS)
    o = dict(o, genome=h["genome"])
    assert set(np.unique(o["genome"])) == {0, 1}
    check_all(deng, device_depth(deng, dev), o, lens, (0, 1000), "long reads")


# ---- 3 ----------------------------------------------------------------------------------------------------------------
def edge_reads(lens):
    """the smallest shapes at which the mark, the scan and the windows can go wrong"""
    reads = [(1, 0, 500, 0, 0), (1, 1, 90_001, 0, 1),                         # L = 0, also at the contig's very end
             (1, 1, 90_001 - 150, 150, 0), (1, 1, 90_001 - 1, 1, 1),          # ends exactly at its contig's end
             (1, 4, 123_457 - 200, 200, 1),                                   # ... at the end of a genome
             (3, 0, 30_000 - 77, 77, 0), (3, 0, 29_999, 1, 0),                # ... at the very last position of depth[]
             (1, 2, 0, 30_017, 0), (1, 2, 0, 30_017, 1),                      # a whole contig, both strands
             (0, 0, 0, 1, 0)]                                                 # the very first position
    for x in (TILE - 1, TILE, TILE + 1):                                      # dense positions on a tile's edge (genome 0 starts at 0)
        reads += [(0, 0, x, 150, 0), (0, 0, x - 149, 150, 1)]
    reads.append((0, 0, 2 * TILE - 5, 2 * TILE + 10, 0))                      # spans three tiles: a carry enters a tile
    p = 40_000                                                                # 5000 reads on one position: contention, depth_max past 255
    reads += [(1, 3, p - (i % 100), 100 + (i % 100), i & 1) for i in range(5000)]
    return make_cols(reads)


def test_hand_built_columns(deng, oracle, genomes, lens, layout):
    dev, host = hand_built(oracle, genomes, layout, deng.device, np.random.default_rng(5))
    edges = edge_reads(lens)
    cols = cat({k: host[k] for k in ("start", "end", "contig", "genome")}, edges)
    d = device_depth(deng, dev, column_reads(deng.device, edges))
    want, s = check_all(deng, d, cols, lens, (1, 7, 1000, 30_017, 1_000_001, 0), "hand-built")
    f13 = deng.depth_contig_first(1, 3)
    assert f13 == 1_000_000 + 300_000 + 90_001 + 30_017 and want[f13 + 40_000] >= 5000
    assert s["depth_max"][4] >= 5000 and s["hist"][255] > 0 and want[TILE - 1] >= 2 and want[2 * TILE + 7] >= 1
    assert deng.depth_contig_first(0, 0) == 0 and deng.depth_contig_first(3, 0) == want.size - 30_000 and want[-1] >= 2
    # a window as long as a contig is that contig's row; one larger than every contig gives one window per contig
    w = deng.depth_summary(1_000_001, d)
    assert np.array_equal(w["win_sum"], w["depth_sum"]) and np.array_equal(w["win_max"], w["depth_max"]) and len(w["win_sum"]) == 7


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def test_the_level_above_the_tiles_loops():
    """one genome with more than two iterations' worth of tile sums, sized from the kernels' constants"""
    n = 2 * TOPS * TILE + 3 * TILE + 77
    assert n < (1 << 25) and -(-(n + 1) // TILE) > 2 * TOPS
    eng = Engine(0)
    try:
        eng.stage_synthetic(0, [n - 5000, 5000], 9)
        rng = np.random.default_rng(3)
        lo = rng.integers(0, n - 5000 - 400, 20_000)
        L = rng.integers(0, 400, 20_000)
        reads = [(0, 0, int(a), int(b), int(a) & 1) for a, b in zip(lo, L)]
        reads += [(0, 0, TOPS * TILE - 3, 6, 0), (0, 0, 2 * TOPS * TILE - 1, 2, 1), (0, 0, 0, n - 5000, 0), (0, 1, 0, 5000, 1), (0, 1, 4999, 1, 0)]
        cols = make_cols(reads)
        lens = {0: [n - 5000, 5000]}
        assert eng.depth_reset() == n
        eng.depth_add(column_reads(eng.device, cols))
        d = eng.depth()
        want = _depth.depth(cols, lens)
        got = d.cpu().numpy()
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        assert want[2 * TOPS * TILE] >= 2 and want[-1] == 2 and want.min() >= 1
        _depth.assert_summary(eng.depth_summary(100_000, d), _depth.summary(want, lens, 100_000), "large genome")
    finally:
        eng.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------
def test_additivity(deng, oracle, genomes, lens):
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
    a = deng.simulate_pe_reads_from_genome(1, prof, 2000, 5, first=0, count=500, qual_offset=33)
    b = deng.simulate_pe_reads_from_genome(1, prof, 2000, 5, first=500, count=500, qual_offset=33)
    whole = deng.simulate_pe_reads_from_genome(1, prof, 2000, 5, qual_offset=33)
    o = _oracle.simulate_pe(oracle, genomes[1], prof, 2000, 5, qual_offset=33).trimmed()
    h = whole.to_host()
    assert_same(h, o, cols=COLS)
    want = _depth.depth(dict(o, genome=h["genome"]), lens)
    d_whole = device_depth(deng, whole).cpu().numpy()
    assert np.array_equal(d_whole, want)
    assert np.array_equal(device_depth(deng, a, b).cpu().numpy(), want) and np.array_equal(device_depth(deng, b, a).cpu().numpy(), want)
    # emit, add more, emit again: the difference array is left as it is
    deng.depth_reset()
    deng.depth_add(a)
    d_a = deng.depth().cpu().numpy()
    deng.depth_add(b)
    assert np.array_equal(deng.depth().cpu().numpy(), want) and d_a.sum() < want.sum()
    # two engines' arrays summed on the host
    other = Engine(0)
    try:
        other.stage_synthetic(0, [1_000_000], 1)
        other.stage_genome(1, genomes[1].contigs)
        other.stage_genome(3, genomes[3].contigs)
        d_b = device_depth(other, b).cpu().numpy()
    finally:
        other.close()
    assert np.array_equal(d_a + d_b, want)


# ---- 6 ----------------------------------------------------------------------------------------------------------------
def test_refusals(deng, oracle, genomes, lens):
    import torch
    good_cols = make_cols([(1, 0, 10, 150, 0), (1, 2, 30_017 - 150, 150, 1), (3, 0, 0, 40, 0)])
    good = column_reads(deng.device, good_cols)
    pod = good.pod()
    fresh = Engine(0)
    try:  # add, emit and summarize before a reset; staging after a reset
        assert fresh.lib.simmr_depth_add(fresh._h, C.byref(pod), good.n_reads) == _abi.ESTATE
        assert fresh.lib.simmr_depth_emit(fresh._h, None, 0) == _abi.ESTATE
        ms = C.c_float()
        assert fresh.lib.simmr_last_depth_ms(fresh._h, C.byref(ms)) == _abi.ESTATE
        fresh.stage_synthetic(0, [5000], 1)
        assert fresh.depth_reset() == 5000
        fresh.stage_synthetic(1, [700], 2)
        one = column_reads(fresh.device, make_cols([(0, 0, 0, 10, 0)]))
        with pytest.raises(SimmrError) as ei:
            fresh.depth_add(one)
        assert ei.value.code == _abi.ESTATE and "staged" in ei.value.msg
        assert fresh.depth_reset() == 5700
        fresh.depth_add(one)
        assert int(fresh.depth().cpu().numpy().sum()) == 10
    finally:
        fresh.close()
    n = deng.depth_reset()
    assert n == sum(sum(v) for v in lens.values())
    # seq, qual and seq_off are not read: NULL is taken
    bare = good.pod()
    bare.seq = bare.qual = bare.seq_off = None
    assert deng.lib.simmr_depth_add(deng._h, C.byref(bare), good.n_reads) == 0
    nostart = good.pod()
    nostart.start = None
    assert deng.lib.simmr_depth_add(deng._h, C.byref(nostart), good.n_reads) == _abi.EINVAL
    assert deng.lib.simmr_depth_add(deng._h, C.byref(pod), 1 << 31) == _abi.ERANGE
    # capacity one short: nothing written
    canary = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=deng.device)
    assert deng.lib.simmr_depth_emit(deng._h, C.c_void_p(canary.data_ptr()), n - 1) == _abi.ERANGE
    assert bool((canary == 0x5A5A5A5A).all())
    # exactly n_positions entries: the entry behind them stays
    canary = torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device=deng.device)
    assert deng.lib.simmr_depth_emit(deng._h, C.c_void_p(canary.data_ptr()), n) == 0
    assert bool((canary[n:] == 0x5A5A5A5A).all()) and np.array_equal(canary[:n].cpu().numpy().view(np.uint32), _depth.depth(good_cols, lens))
    win = _abi.DepthWindows(None, None, None, 3, 0)
    assert deng.lib.simmr_depth_summarize(deng._h, C.c_void_p(canary.data_ptr()), 1000, None, 0, None, C.byref(win)) == _abi.ERANGE
    assert win.n_windows == sum(-(-x // 1000) for v in lens.values() for x in v)
    # bad reads answer through the sticky word, and never fault
    bads = [make_cols([(1, 2, 30_017 - 149, 150, 0)]),            # one base past its contig
            make_cols([(1, 5, 0, 10, 0)]),                         # contig index == n_contigs
            make_cols([(2, 0, 0, 10, 0)]), make_cols([(77, 0, 0, 10, 1)]),   # a slot that is not staged / beyond the table
            make_cols([(3, 0, 30_001, 0, 0)]),                     # L = 0 behind the end
            {"start": np.array([5], np.uint64), "end": np.array([(1 << 64) - 3], np.uint64), "contig": np.array([0], np.uint32), "genome": np.array([0], np.uint32)}]
    for bad in bads:
        deng.depth_reset()
        deng.depth_add(column_reads(deng.device, cat(good_cols, bad, good_cols)))
        with pytest.raises(SimmrError) as ei:
            deng.depth()
        assert ei.value.code == _abi.EINVAL
        deng.depth_add(good)
        with pytest.raises(SimmrError):  # sticky until the reset
            deng.depth()
    def spoil(cols, specs):
        cols["genome"][5] = 77
    bad, _ = hand_built(oracle, genomes, 0, deng.device, np.random.default_rng(5), spoil)
    deng.depth_reset()
    deng.depth_add(bad)
    with pytest.raises(SimmrError):
        deng.depth()
    assert np.array_equal(device_depth(deng, good).cpu().numpy(), _depth.depth(good_cols, lens))
