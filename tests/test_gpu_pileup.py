"""Allele counts at listed sites on the device (simmr_pileup_reset / _add / _read, include/simmr_hip.h) against the numpy
restatement of the header's definition (tests/_pileup.py), applied to columns copied back from the device: nothing expected
here comes from the pass under test.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import MinimalLongErrorProfile, MinimalShortErrorProfile, PerfectShortErrorProfile, SimmrError, _abi
from simmr_amd.engine import Engine, Reads
from tests import _depth, _oracle, _pileup, _synth
from tests._hand_built import hand_built

pytestmark = pytest.mark.gpu
LENS1 = [300_000, 90_001, 30_017, 70_000, 123_457]
BYTES = np.frombuffer(b"ACGTACGTACGTNn-acgtR", dtype=np.uint8)  # what a read may hold: mostly bases, some of class 4


def stage_three(eng):
    """the three genomes of tests/test_gpu_depth.py: slots 0, 1 and 3, the last one with N and -"""
    rng = np.random.default_rng(21)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30000)].copy()
    seq[rng.integers(0, 30000, 3000)] = ord("N")
    seq[rng.integers(0, 30000, 500)] = ord("-")
    seq[12_000:12_400] = ord("N")
    g = {0: _oracle.HostGenome(_synth.synthetic_contigs([1_000_000], 1)),
         1: _oracle.HostGenome(_synth.synthetic_contigs(LENS1, 7)),
         3: _oracle.HostGenome([seq])}
    eng.stage_synthetic(0, [1_000_000], 1)
    eng.stage_genome(1, g[1].contigs)
    eng.stage_genome(3, g[3].contigs)
    return g


@pytest.fixture(scope="module")
def peng():
    """an engine of this module's own: the keys are positions in the layout of every genome staged in an engine"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def genomes(peng):
    return stage_three(peng)


@pytest.fixture(scope="module")
def lens(genomes):
    return {s: [int(c.size) for c in g.contigs] for s, g in genomes.items()}


@pytest.fixture
def fresh():
    """an engine whose genomes a test may diverge"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = Engine(0)
    try:
        yield e
    finally:
        e.close()


@pytest.fixture(params=[0, 16], ids=["compact", "slot16"])
def layout(request):
    return request.param


def make_reads(device, specs, layout, rng):
    """[(genome, contig, lo, L, reverse)] -> device columns in `layout` with bytes drawn from BYTES (the pass never compares a
    read with its genome)"""
    import torch
    g, c, lo, L, rev = (np.array(x, dtype=np.int64) for x in zip(*specs))
    n = len(specs)
    slot = (L + 15) // 16 * 16 if layout == 16 else L
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(slot, out=first[1:])
    total = int(first[n])
    seq = np.zeros(total + 16, dtype=np.uint8)
    seq_off = first.copy()
    if layout == 16:
        seq_off[:n] += np.where(rev == 1, slot - L, 0)  # reverse mates right-aligned
    for r in range(n):
        seq[seq_off[r]:seq_off[r] + L[r]] = BYTES[rng.integers(0, BYTES.size, L[r])]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(device)
    return Reads(seq=t(seq, np.uint8), qual=torch.zeros(16, dtype=torch.uint8, device=device), seq_off=t(seq_off, np.int64),
                 start=t(np.where(rev == 1, lo + L, lo), np.int64), end=t(np.where(rev == 1, lo, lo + L), np.int64), contig=t(c, np.int32),
                 genome=t(g, np.int32), read_id=t(np.arange(n), np.int32), flags=t(rev, np.uint8), n_reads=n, total_bases=total,
                 qual_offset=33, slot_bytes=layout)


def host_cols(reads):
    """the columns as they lie in HBM (seq_off[r] is the read's first base in both layouts); qual is not wanted"""
    n = reads.n_reads
    return {"seq": reads.seq.cpu().numpy(), "seq_off": reads.seq_off[: n + 1].cpu().numpy().astype(np.uint64),
            "start": reads.start[:n].cpu().numpy().astype(np.uint64), "end": reads.end[:n].cpu().numpy().astype(np.uint64),
            "contig": reads.contig[:n].cpu().numpy().astype(np.uint32), "genome": reads.genome[:n].cpu().numpy().astype(np.uint32),
            "flags": reads.flags[:n].cpu().numpy()}


def sorted_sites(triples):
    t = sorted(set(triples))
    return tuple(np.array([x[k] for x in t], dtype=dt) for k, dt in enumerate((np.uint32, np.uint32, np.uint64)))


def device_pileup(eng, sites, *reads):
    assert eng.pileup_reset(*sites) == len(sites[2])
    for r in reads:
        eng.pileup_add(r)
    return eng.pileup()


def check(eng, sites, lens, reads, what):
    got = device_pileup(eng, sites, *reads)
    want = sum(_pileup.pileup(host_cols(r), sites, lens) for r in reads)
    assert got.dtype == np.uint32 and got.shape == (len(sites[2]), 2, 5), what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8])
    return got


# ---- 1: hand-built reads ----------------------------------------------------------------------------------------------
def edge_sites(cols, lens):
    """a site at every read's first and last base, at lo - 1 and at lo + L where the contig has them, and position 0 of the
    next contig behind a read that ends at its contig's last base"""
    out = []
    for a, b, c, g in zip(cols["start"].astype(np.int64), cols["end"].astype(np.int64), cols["contig"], cols["genome"]):
        lo, L, n = int(min(a, b)), int(abs(b - a)), lens[int(g)][int(c)]
        out += [(int(g), int(c), p) for p in (lo - 1, lo, lo + L - 1, lo + L) if 0 <= p < n]
        if lo + L == n and int(c) + 1 < len(lens[int(g)]):
            out.append((int(g), int(c) + 1, 0))
    return out


def test_hand_built_reads(peng, oracle, genomes, lens, layout):
    dev, host = hand_built(oracle, genomes, layout, peng.device, np.random.default_rng(5))
    triples = edge_sites(host, lens)
    triples += [(3, 0, p) for p in range(11_990, 12_410, 7)]  # under the staged N run, and around it
    dash = np.flatnonzero(genomes[3].contigs[0][11_900:12_700] == ord("-")) + 11_900
    triples += [(3, 0, int(p)) for p in dash[:20]]
    sites = sorted_sites(triples)
    got = check(peng, sites, lens, [dev], "hand-built")
    key = {t: i for i, t in enumerate(zip(*(x.tolist() for x in sites)))}
    # the reads of genome 3 come as one window on both strands: both cover its first and its last base
    for p in (12_085, 12_085 + 510):
        assert got[key[(3, 0, p)], 0].sum() >= 1 and got[key[(3, 0, p)], 1].sum() >= 1, p
    # under the staged N run: two forward reads and one reverse read, all of class 4
    under_n = got[key[(3, 0, 12_109)]]
    assert under_n[0, 4] == 2 and under_n[1, 4] == 1 and under_n.sum() == 3, under_n
    at_dash = got[[key[(3, 0, int(p))] for p in dash[:20]]]
    assert at_dash[:, 1, 4].sum() > 0 and at_dash[:, 0, 4].sum() > 0
    # a read that ends at its contig's last base does not reach position 0 of the next contig
    assert (1, 3, 0) in key and got[key[(1, 3, 0)]].sum() == 0 and got[key[(1, 2, lens[1][2] - 1)]].sum() == 2
    # lo - 1 and lo + L of a lone read stay empty, its first and last base count once
    lone = key[(1, 0, 700)]
    assert got[lone].sum() == 1 and got[key[(1, 0, 699)]].sum() == 0 and got[key[(1, 0, 716)]].sum() == 1 and got[key[(1, 0, 717)]].sum() == 0


@pytest.mark.parametrize("n_sites", [0, 1])
def test_no_site_and_one_site(peng, genomes, lens, layout, n_sites):
    rng = np.random.default_rng(8)
    reads = make_reads(peng.device, [(1, 1, 500, 150, 0), (1, 1, 520, 150, 1), (1, 1, 700, 0, 0), (0, 0, 5, 40, 1)], layout, rng)
    sites = sorted_sites([(1, 1, 600)][:n_sites])
    got = check(peng, sites, lens, [reads], f"{n_sites} sites")
    assert got.shape == (n_sites, 2, 5) and int(got.sum()) == 2 * n_sites
    assert peng.last_pileup_ms() >= 0


# ---- 2: the expansion -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rev", [0, 1], ids=["forward", "reverse"])
@pytest.mark.parametrize("lane", [0, 17, 63])
def test_one_long_read_among_63_without_sites(peng, genomes, lens, layout, lane, rev):
    """1 666 pairs of one lane, none of the 63 others: the wave's steps all search for the same read"""
    rng = np.random.default_rng(9)
    specs = [(0, 0, 500_000 + 200 * i, 150, i & 1) for i in range(64)]
    specs[lane] = (0, 0, 100_000, 5000, rev)
    reads = make_reads(peng.device, specs, layout, rng)
    sites = sorted_sites([(0, 0, 100_000 + 3 * k) for k in range(1666)] + [(0, 0, 99_999), (0, 0, 105_000), (0, 0, 499_999)])
    got = check(peng, sites, lens, [reads], "one long read")
    assert int(got.sum()) == 1666 and int(got[:, 1 - rev].sum()) == 0


def test_a_wave_of_one_site_each(peng, genomes, lens, layout):
    rng = np.random.default_rng(10)
    specs = [(0, 0, 200_000 + 300 * i, 150, (i >> 1) & 1) for i in range(64)]
    sites = sorted_sites([(0, 0, 200_000 + 300 * i + (i * 149) // 63) for i in range(64)])  # from a read's first base to its last
    got = check(peng, sites, lens, [make_reads(peng.device, specs, layout, rng)], "one site each")
    assert np.array_equal(got.sum(axis=(1, 2)), np.ones(64, dtype=np.uint32))


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 129])
def test_read_counts_around_a_wave(peng, genomes, lens, layout, n_reads):
    rng = np.random.default_rng(11)
    lo = rng.integers(0, 20_000, 129)
    L = rng.integers(0, 700, 129)
    specs = [(1, 4, int(a), int(b), int(a) & 1) for a, b in zip(lo, L)][:n_reads]
    sites = sorted_sites([(1, 4, p) for p in range(0, 21_000, 13)] + [(1, 3, 69_999), (3, 0, 0)])
    got = check(peng, sites, lens, [make_reads(peng.device, specs, layout, rng)], f"{n_reads} reads")
    assert int(got.sum()) > 0


# ---- 3, 4: runs on a strain --------------------------------------------------------------------------------------------
def strain_sites(eng, slot, identity, seed):
    s = eng.strain(slot, identity, seed)
    return (np.full(s["pos"].size, slot, dtype=np.uint32), s["contig"], s["pos"]), s


@pytest.mark.parametrize("rng_mode", [_abi.RNG_REFERENCE, _abi.RNG_PHILOX], ids=["reference", "philox"])
def test_paired_end_run_on_a_strain(fresh, layout, rng_mode):
    stage_three(fresh)
    lens = {0: [1_000_000], 1: LENS1, 3: [30_000]}
    sites, _ = strain_sites(fresh, 1, 0.97, 77)
    assert 15_000 < sites[2].size < 22_000
    fresh.set_read_slots(layout)
    reads = fresh.simulate_pe_reads_from_genome(1, MinimalShortErrorProfile(rng_mode=rng_mode).pod(), 40_000, 5, qual_offset=33)
    assert reads.n_reads == 40_000
    got = check(fresh, sites, lens, [reads], "paired-end run")
    # the ten counts of every site sum to depth[] at its position
    fresh.depth_reset()
    fresh.depth_add(reads)
    d = fresh.depth().cpu().numpy()
    assert np.array_equal(got.sum(axis=(1, 2)), d[_pileup.site_keys(sites, lens)]) and got[:, 0].sum() > 0 and got[:, 1].sum() > 0


def test_long_read_run_on_a_strain(fresh):
    stage_three(fresh)
    lens = {0: [1_000_000], 1: LENS1, 3: [30_000]}
    sites, _ = strain_sites(fresh, 0, 0.99, 3)
    lp = MinimalLongErrorProfile(length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    reads = fresh.simulate_long_reads([0], [2000], lp, 3, qual_offset=33)
    got = check(fresh, sites, lens, [reads], "long-read run")
    assert int(got.sum()) > 100 * 2000  # a read covers hundreds of sites
    fresh.depth_reset()
    fresh.depth_add(reads)
    assert np.array_equal(got.sum(axis=(1, 2)), fresh.depth().cpu().numpy()[_pileup.site_keys(sites, lens)])


def test_perfect_reads_show_the_alternate(fresh):
    stage_three(fresh)
    lens = {0: [1_000_000], 1: LENS1, 3: [30_000]}
    sites, s = strain_sites(fresh, 1, 0.97, 9)
    reads = fresh.simulate_pe_reads_from_genome(1, PerfectShortErrorProfile().pod(), 20_000, 5, qual_offset=33)
    got = check(fresh, sites, lens, [reads], "perfect-short run")
    fresh.depth_reset()
    fresh.depth_add(reads)
    d = fresh.depth().cpu().numpy()[_pileup.site_keys(sites, lens)]
    alt = _pileup.CLASS[s["alt"]]
    at_alt = got[np.arange(alt.size), :, alt].sum(axis=1)
    assert np.array_equal(at_alt, d) and np.array_equal(got.sum(axis=(1, 2)), d) and (d > 0).sum() > 1000


# ---- 5: adds and resets -----------------------------------------------------------------------------------------------
def test_adds_and_resets(peng, genomes, lens):
    rng = np.random.default_rng(12)
    spec = lambda k: [(1, 0, int(a), int(b), int(a) & 1) for a, b in zip(rng.integers(0, 50_000, k), rng.integers(0, 400, k))]
    sites = sorted_sites([(1, 0, p) for p in range(0, 51_000, 17)])
    ab = make_reads(peng.device, spec(511), 0, np.random.default_rng(13))
    part = lambda i, j: Reads(seq=ab.seq, qual=ab.qual, seq_off=ab.seq_off[i:j + 1], start=ab.start[i:j], end=ab.end[i:j], contig=ab.contig[i:j],
                              genome=ab.genome[i:j], read_id=ab.read_id[i:j], flags=ab.flags[i:j], n_reads=j - i, total_bases=ab.total_bases,
                              qual_offset=33, slot_bytes=0)
    a, b = part(0, 300), part(300, 511)  # (the same bytes of seq[]: a part's offsets are the whole's)
    whole = check(peng, sites, lens, [ab], "one add")
    two = check(peng, sites, lens, [b, a], "two adds")
    assert np.array_equal(two, whole) and int(whole.sum()) > 1000
    assert np.array_equal(peng.pileup(), two) and np.array_equal(peng.pileup(), two)  # reading leaves the table as it is
    peng.pileup_add(a)
    assert np.array_equal(peng.pileup(), two + _pileup.pileup(host_cols(a), sites, lens))
    assert peng.pileup_reset(*sites) == len(sites[2]) and int(peng.pileup().sum()) == 0  # a reset zeroes the table


# ---- 6: refusals ------------------------------------------------------------------------------------------------------
BAD_SITES = [
    ("out of order", [(1, 0, 10), (1, 0, 30), (1, 0, 20), (1, 1, 0)], 2),
    ("contigs out of order", [(1, 1, 10), (1, 0, 30)], 1),
    ("slots out of order", [(0, 0, 5), (3, 0, 5), (1, 0, 5)], 2),
    ("a repeated site", [(0, 0, 5), (1, 2, 7), (1, 2, 7)], 2),
    ("pos == len", [(1, 0, 5), (1, 1, 90_001)], 1),
    ("pos == len of the last contig", [(3, 0, 30_000)], 0),
    ("an unstaged slot", [(1, 0, 5), (2, 0, 0)], 1),
    ("a slot beyond the table", [(77, 0, 0)], 0),
    ("a contig that does not exist", [(0, 0, 1), (0, 0, 2), (0, 0, 3), (1, 5, 0)], 3),
]


@pytest.mark.parametrize("what,triples,first_bad", BAD_SITES, ids=[b[0] for b in BAD_SITES])
def test_reset_refuses_a_bad_site_list(peng, genomes, what, triples, first_bad):
    cols = tuple(np.array([t[k] for t in triples], dtype=dt) for k, dt in enumerate((np.uint32, np.uint32, np.uint64)))
    with pytest.raises(SimmrError) as ei:
        peng.pileup_reset(*cols)
    assert ei.value.code == _abi.EINVAL and ei.value.msg.startswith(f"site {first_bad}:"), ei.value.msg
    # no table is in force after a refused reset
    reads = make_reads(peng.device, [(1, 0, 0, 10, 0)], 0, np.random.default_rng(1))
    pod = reads.pod()
    assert peng.lib.simmr_pileup_add(peng._h, C.byref(pod), 1) == _abi.ESTATE
    assert peng.lib.simmr_pileup_read(peng._h, None, 0) == _abi.ESTATE


def test_add_and_read_refusals(peng, genomes, lens):
    import torch
    rng = np.random.default_rng(14)
    good_specs = [(1, 0, 10, 150, 0), (1, 2, 30_017 - 150, 150, 1), (3, 0, 0, 40, 0)]
    good = make_reads(peng.device, good_specs, 0, rng)
    pod = good.pod()
    sites = sorted_sites([(1, 0, 10), (1, 0, 100), (1, 2, 30_016), (3, 0, 39), (3, 0, 40)])
    n = len(sites[2])
    other = Engine(0)
    try:  # add, read and the time before a reset; a staging call after one
        ms = C.c_float()
        assert other.lib.simmr_pileup_add(other._h, C.byref(pod), good.n_reads) == _abi.ESTATE
        assert other.lib.simmr_pileup_read(other._h, None, 0) == _abi.ESTATE
        assert other.lib.simmr_last_pileup_ms(other._h, C.byref(ms)) == _abi.ESTATE
        other.stage_synthetic(0, [5000], 1)
        one = make_reads(other.device, [(0, 0, 0, 10, 0)], 0, rng)
        assert other.pileup_reset([0], [0], [3]) == 1
        other.stage_synthetic(1, [700], 2)
        with pytest.raises(SimmrError) as ei:
            other.pileup_add(one)
        assert ei.value.code == _abi.ESTATE and "staged" in ei.value.msg
        assert other.pileup_reset([0, 1], [0, 0], [3, 699]) == 2
        other.pileup_add(one)
        assert other.pileup().sum(axis=(1, 2)).tolist() == [1, 0]
        other.strain(0, 0.9, 1, sites=False)  # simmr_strain_apply counts as staging
        with pytest.raises(SimmrError) as ei:
            other.pileup_add(one)
        assert ei.value.code == _abi.ESTATE
    finally:
        other.close()
    assert peng.pileup_reset(*sites) == n
    for col in ("seq", "seq_off", "start", "end", "contig", "genome", "flags"):
        bare = good.pod()
        setattr(bare, col, None)
        assert peng.lib.simmr_pileup_add(peng._h, C.byref(bare), good.n_reads) == _abi.EINVAL, col
    noqual = good.pod()
    noqual.qual = noqual.read_id = None  # qual is not read
    assert peng.lib.simmr_pileup_add(peng._h, C.byref(noqual), good.n_reads) == 0
    assert peng.lib.simmr_pileup_add(peng._h, C.byref(pod), 1 << 31) == _abi.ERANGE
    want = _pileup.pileup(host_cols(good), sites, lens)
    assert int(want.sum()) == 4
    # capacity one short: nothing written, on either side of the buffer or in it
    canary = torch.full((10 + 10 * n + 10,), 0x5A5A5A5A, dtype=torch.int32, device=peng.device)
    mid = canary.data_ptr() + 40
    assert peng.lib.simmr_pileup_read(peng._h, C.c_void_p(mid), n - 1) == _abi.ERANGE
    assert bool((canary == 0x5A5A5A5A).all())
    # exactly n sites: the entries in front of and behind them stay
    assert peng.lib.simmr_pileup_read(peng._h, C.c_void_p(mid), n) == 0
    assert bool((canary[:10] == 0x5A5A5A5A).all()) and bool((canary[10 + 10 * n:] == 0x5A5A5A5A).all())
    assert np.array_equal(canary[10:10 + 10 * n].cpu().numpy().view(np.uint32).reshape(n, 2, 5), want)
    # bad reads answer through the sticky word: they are refused by the bounds check and never loaded from
    def spoiled(change):
        r = make_reads(peng.device, good_specs + [(1, 2, 30_017 - 150, 150, 0)] + good_specs, 0, np.random.default_rng(15))
        change(r)
        return r
    def window_leaves_contig(r): r.start[3] += 1; r.end[3] += 1
    def contig_missing(r): r.contig[3] = 5
    def slot_unstaged(r): r.genome[3] = 2
    def slot_beyond(r): r.genome[3] = 77
    def huge_end(r): r.end[3] = -3
    def bytes_leave_seq(r): r.seq_off[3] = r.seq.numel() - 149
    def offset_beyond(r): r.seq_off[3] = 1 << 62
    for change in (window_leaves_contig, contig_missing, slot_unstaged, slot_beyond, huge_end, bytes_leave_seq, offset_beyond):
        peng.pileup_reset(*sites)
        peng.pileup_add(spoiled(change))
        canary.fill_(0x5A5A5A5A)
        assert peng.lib.simmr_pileup_read(peng._h, C.c_void_p(mid), n) == _abi.EINVAL, change.__name__
        assert bool((canary == 0x5A5A5A5A).all()), change.__name__
        peng.pileup_add(good)
        with pytest.raises(SimmrError):  # sticky until the reset
            peng.pileup()
    assert np.array_equal(device_pileup(peng, sites, good), want)
