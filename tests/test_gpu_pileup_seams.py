"""k_pileup_add (simmr_amd/csrc/pileup_kernels.hip) past the sizes of tests/test_gpu_pileup.py: a wave's second and third trip
through the persistent grid, a read's second scan round, a count past 16 bits on one site, the 64-pair steps of the expansion
with a read's first and last pair on a step's edge, the ends of the site list, and bytes of seq[] at and past 4 GiB.  The reads
and sites are those of tests/_pileup_cases.py; what is expected is tests/_seams.py:pileup_from_columns (held to the plain model
of tests/_pileup.py by tests/test_seams_host.py) of the columns as copied back from the device.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import SimmrError, _abi
from simmr_amd.engine import Engine, Reads
from tests import _pileup, _pileup_cases, _seams
from tests.test_gpu_pileup import stage_three

pytestmark = pytest.mark.gpu
WG, ROUND, WGS_PER_CU = _pileup.constants()
LENS = _pileup_cases.LENS


@pytest.fixture(scope="module")
def seng():
    """an engine of this module's own with the three genomes of tests/test_gpu_pileup.py"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = Engine(0)
    try:
        g = stage_three(e)
        assert {s: [int(c.size) for c in h.contigs] for s, h in g.items()} == LENS
        yield e
    finally:
        e.close()


def to_device(cols, device):
    """the host columns of _pileup_cases.read_columns as Reads in HBM"""
    import torch
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(device)
    n = len(cols["start"])
    return Reads(seq=t(cols["seq"], np.uint8), qual=torch.zeros(16, dtype=torch.uint8, device=device), seq_off=t(cols["seq_off"], np.int64),
                 start=t(cols["start"], np.int64), end=t(cols["end"], np.int64), contig=t(cols["contig"], np.int32), genome=t(cols["genome"], np.int32),
                 read_id=t(np.arange(n), np.int32), flags=t(cols["flags"], np.uint8), n_reads=n, total_bases=cols["total_bases"], qual_offset=33,
                 slot_bytes=cols["layout"])


def host_cols(reads, seq_from=0):
    """the columns as they lie in HBM, seq[] from byte `seq_from` on"""
    n = reads.n_reads
    return {"seq": reads.seq[seq_from:].cpu().numpy(), "seq_off": reads.seq_off[:n].cpu().numpy().astype(np.uint64),
            "start": reads.start[:n].cpu().numpy().astype(np.uint64), "end": reads.end[:n].cpu().numpy().astype(np.uint64),
            "contig": reads.contig[:n].cpu().numpy().astype(np.uint32), "genome": reads.genome[:n].cpu().numpy().astype(np.uint32),
            "flags": reads.flags[:n].cpu().numpy()}


def check(eng, sites, lens, adds, what, seq_from=0):
    """reset, every add, read; against the model's sum over the adds"""
    assert eng.pileup_reset(*sites) == len(sites[2])
    for r in adds:
        eng.pileup_add(r)
    got = eng.pileup()
    want = sum(_seams.pileup_from_columns(host_cols(r, seq_from), sites, lens, seq_base=seq_from) for r in adds)
    assert got.dtype == np.uint32 and got.shape == (len(sites[2]), 2, 5), what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8])
    return got


def pairs_per_read(cols, sites, lens):
    """(pairs, first site) of every read, from the model's keys and two searchsorted calls"""
    keys = _seams.pileup_keys(sites, lens)
    first, _ = _seams.pileup_layout(lens)
    a, b = cols["start"].astype(np.int64), cols["end"].astype(np.int64)
    klo = first[cols["genome"].astype(np.int64), cols["contig"].astype(np.int64)] + np.minimum(a, b)
    s0 = np.searchsorted(keys, klo, side="left")
    return np.searchsorted(keys, klo + np.abs(b - a), side="left") - s0, s0


def skip_without_memory(e):
    """the rule of tests/test_gpu_regions.py::test_more_tiles_than_one_scan_iteration: a refusal of memory skips, nothing else does"""
    if isinstance(e, SimmrError) and e.code != _abi.ENOMEM:
        raise e
    pytest.skip("the memory cannot be had")


# ---- (a) every wave takes a second batch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 16], ids=["compact", "slot16"])
def test_every_wave_takes_a_second_and_a_third_batch(seng, layout):
    import torch
    waves = int(torch.cuda.get_device_properties(0).multi_processor_count) * WGS_PER_CU * (WG // 64)
    n_reads = 2 * 64 * waves + 7 * 64 + 3
    assert -(-n_reads // 64) > 2 * waves and n_reads % 64 != 0, "resize: every wave must take two batches, some a third, and the last batch is partial"
    rng = np.random.default_rng(31 + layout)
    g, c, lo, L, rev = _pileup_cases.spread_reads(n_reads, LENS, rng)
    L[-3:], lo[-3:] = 39, np.minimum(lo[-3:], 29_000)  # the three reads of the last batch have pairs whatever was drawn
    reads = to_device(_pileup_cases.read_columns(g, c, lo, L, rev, layout, rng), seng.device)
    sites = _pileup_cases.every_kth_position(LENS, 13)
    got = check(seng, sites, LENS, [reads], "grid trips")
    cols = host_cols(reads)
    n_pairs, _ = pairs_per_read(cols, sites, LENS)
    assert int(got.sum()) == int(n_pairs.sum()) > n_reads and got[:, 0].sum() > 0 and got[:, 1].sum() > 0
    assert (n_pairs == 0).sum() > n_reads // 8 and n_pairs.max() == 3 and set(cols["genome"].tolist()) == {0, 1, 3}
    # the last batch of the second trip, the partial third trip and the partial last batch all hold pairs
    for lo, hi in ((2 * 64 * waves - 64, 2 * 64 * waves), (2 * 64 * waves, n_reads - 3), (n_reads - 3, n_reads)):
        assert n_pairs[lo:hi].sum() > 0, (lo, hi)


# ---- (b) a read takes a second round --------------------------------------------------------------------------------------------
def test_a_read_takes_a_second_round():
    import torch
    n = ROUND + 4096 + 77
    lens = {0: [n]}
    rng = np.random.default_rng(32)
    lane = np.arange(64)
    short = lambda first: (np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.int64), first + 200_000 * lane, np.array([0, 1, 150])[lane % 3], lane & 1)
    g, c, lo, L, rev = short(1000)
    lo[5], L[5], rev[5] = 11, ROUND + 70, 0    # 70 pairs in its second round
    lo[40], L[40], rev[40] = 14, ROUND + 1, 1  # one pair in its second round
    assert L[5] > ROUND and L[40] > ROUND and lo[5] + L[5] <= n and (np.delete(lo + L, [5, 40]) < ROUND).all()
    adds = [_pileup_cases.read_columns(g, c, lo, L, rev, 0, rng), _pileup_cases.read_columns(*short(100_500), 0, rng)]
    total = int(L.sum() + adds[1]["total_bases"])
    eng = Engine(0)
    try:
        try:
            eng.stage_synthetic(0, [n], 5)
            assert eng.pileup_reset(torch.zeros(n, dtype=torch.int32, device=eng.device), torch.zeros(n, dtype=torch.int32, device=eng.device),
                                    torch.arange(n, dtype=torch.int64, device=eng.device)) == n  # every position is a site
            dev = [to_device(a, eng.device) for a in adds]
            for r in dev:
                eng.pileup_add(r)
            got = eng.pileup()
            sites = (np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint64))
            keys = _seams.pileup_keys(sites, lens)
            want = sum(_seams.pileup_from_columns(host_cols(r), sites, lens, 1 << 20, keys=keys) for r in dev)
        except (SimmrError, MemoryError, torch.cuda.OutOfMemoryError) as e:
            skip_without_memory(e)
        # both sides of each long read's round seam, per strand: nobody else lies there
        for at, strand, covered in ((11 + ROUND - 1, 0, 1), (11 + ROUND, 0, 1), (11 + ROUND + 69, 0, 1), (11 + ROUND + 70, 0, 0),
                                    (14 + ROUND - 1, 1, 1), (14 + ROUND, 1, 1), (14 + ROUND + 1, 1, 0), (10, 0, 0), (11, 0, 1), (13, 1, 0), (14, 1, 1)):
            assert got[at, strand].sum() == covered and np.array_equal(got[at], want[at]), (at, strand, got[at], want[at])
        assert int(got.sum(dtype=np.uint64)) == total and int(got[:, 0].sum(dtype=np.uint64)) > ROUND and int(got[:, 1].sum(dtype=np.uint64)) > ROUND
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    finally:
        eng.close()


# ---- (c) counts past 16 bits on one site ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("identical", [False, True], ids=["every offset", "one read"])
def test_a_count_past_16_bits(seng, identical):
    rng = np.random.default_rng(33)
    reads, sites = _pileup_cases.deep_case(70_000, identical, rng)
    got = check(seng, sites, LENS, [to_device(_pileup_cases.read_columns(*reads, 0, rng, shared=identical), seng.device)], "one deep column")
    at_p = got[2].astype(np.int64)
    assert at_p.sum() == 70_000 and got[0].sum() == 0 and got[4].sum() == 0
    if identical:
        assert at_p.max() == 70_000 and at_p[1].sum() == 70_000  # one cell holds them all
    else:
        assert at_p[0].sum() == 35_000 and at_p[1].sum() == 35_000 and at_p.sum() > 65_535
        assert got[1].sum() > 0 and got[3].sum() > 0 and got[1].sum() + got[3].sum() < 2 * 70_000


# ---- (d) step seams of the expansion --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", _pileup_cases.STRANDS)
@pytest.mark.parametrize("name", _pileup_cases.STEP_COUNTS)
def test_pairs_on_the_edges_of_a_step(seng, name, which):
    reads, sites, counts = _pileup_cases.step_case(name, which)
    dev = to_device(_pileup_cases.read_columns(*reads, 0, np.random.default_rng(34)), seng.device)
    n_pairs, _ = pairs_per_read(host_cols(dev), sites, LENS)
    assert np.array_equal(n_pairs, counts) and np.array_equal(counts[:64], _pileup_cases.STEP_COUNTS[name]) and not counts[64:128].any()
    got = check(seng, sites, LENS, [dev], name)
    assert int(got.sum()) == 2 * int(_pileup_cases.STEP_COUNTS[name].sum())
    assert int(got[:, 0].sum()) == int(counts[reads[4] == 0].sum()) and int(got[:, 1].sum()) == int(counts[reads[4] == 1].sum())


# ---- (e) the ends of the site list ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 16], ids=["compact", "slot16"])
@pytest.mark.parametrize("before", [0, 3])
@pytest.mark.parametrize("m", [149, 150, 151, 152])
def test_a_read_whose_sites_end_with_the_list(seng, m, before, layout):
    reads, sites = _pileup_cases.list_end_case(m, before)
    dev = to_device(_pileup_cases.read_columns(*reads, layout, np.random.default_rng(35)), seng.device)
    n_pairs, s0 = pairs_per_read(host_cols(dev), sites, LENS)
    n, L = len(sites[2]), _pileup_cases.END_L
    assert n - s0[0] == n - s0[1] == m and m - L in (-1, 0, 1, 2) and n_pairs[0] == n_pairs[1] == min(m, L)
    assert n_pairs[2:6].sum() == 0 and n_pairs[6] == n_pairs[7] == n  # below and above the list; the whole list
    got = check(seng, sites, LENS, [dev], f"{m} sites behind s0")
    assert got[:, 0].sum() == got[:, 1].sum() == n_pairs.sum() // 2


@pytest.mark.parametrize("pos", [(40_000,), (40_000, 40_001), (40_000, 40_149), (40_000, 40_150)], ids=lambda p: f"{len(p)}-{p[-1] - p[0]}")
def test_a_list_of_one_and_of_two_sites(seng, pos):
    reads, sites = _pileup_cases.short_list_case(np.array(pos))
    dev = to_device(_pileup_cases.read_columns(*reads, 0, np.random.default_rng(36)), seng.device)
    n_pairs, _ = pairs_per_read(host_cols(dev), sites, LENS)
    assert len(sites[2]) in (1, 2) and n_pairs[12] == n_pairs[13] == len(pos) and n_pairs[4:6].sum() == 0 and n_pairs[8:12].sum() == 0
    got = check(seng, sites, LENS, [dev], f"{len(pos)} sites")
    assert int(got.sum()) == int(n_pairs.sum()) and got[:, 0].sum() == got[:, 1].sum()


# ---- (f) bytes at and past 4 GiB ------------------------------------------------------------------------------------------------
def test_bytes_at_and_past_4_gib(seng):
    import torch
    cap, tail = 2**32 + 65536, 65536 + 4096
    base = cap - tail  # the first byte written, and the first copied back
    rng = np.random.default_rng(37)
    n = 200
    g, c, lo, L, rev = _pileup_cases.spread_reads(n, LENS, rng, lmax=300)
    L[:5] = np.minimum(np.maximum(L[:5], 100), 299)
    lo[:5] = np.minimum(lo[:5], np.array([LENS[int(a)][int(b)] for a, b in zip(g[:5], c[:5])]) - L[:5])
    off = base + rng.integers(0, tail - 300, n)
    off[0] = 2**32                 # starts exactly at 4 GiB
    off[1] = cap - L[1]            # ends exactly at seq_capacity
    off[2] = 2**32 - L[2] // 2     # lies across 4 GiB
    off[3] = 2**32 - L[3]          # ends on the last byte below 4 GiB
    off[4] = 2**32 - 1             # one byte below, the rest above
    assert off.max() >= 2**32 and (off < 2**32).sum() > 3 and (off >= 2**32).sum() > 100 and (off + L <= cap).all()
    keys = np.flatnonzero(rng.random(sum(sum(v) for v in LENS.values())) < 0.1)
    first, _ = _seams.pileup_layout(LENS)
    rows = [(s, k) for s in sorted(LENS) for k in range(len(LENS[s]))]
    row = np.searchsorted(np.array([first[r] for r in rows]), keys, side="right") - 1
    sites = _pileup_cases.site_columns(np.array([r[0] for r in rows])[row], np.array([r[1] for r in rows])[row], keys - np.array([first[r] for r in rows])[row])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(seng.device)
    try:
        seq = torch.empty(cap, dtype=torch.uint8, device=seng.device)
        seq[base:] = t(_pileup_cases.BYTES[rng.integers(0, _pileup_cases.BYTES.size, tail)], np.uint8)
    except (MemoryError, torch.cuda.OutOfMemoryError) as e:
        skip_without_memory(e)
    make = lambda seq_off: Reads(seq=seq, qual=torch.zeros(16, dtype=torch.uint8, device=seng.device), seq_off=t(np.concatenate([seq_off, [cap]]), np.int64),
                                 start=t(np.where(rev == 1, lo + L, lo), np.int64), end=t(np.where(rev == 1, lo, lo + L), np.int64), contig=t(c, np.int32),
                                 genome=t(g, np.int32), read_id=t(np.arange(n), np.int32), flags=t(rev, np.uint8), n_reads=n, total_bases=cap,
                                 qual_offset=33, slot_bytes=0)
    reads = make(off)
    cols = host_cols(reads, base)
    assert cols["seq"].size == tail and int(cols["seq_off"].max()) >= 2**32 and reads.pod().seq_capacity == cap
    n_pairs, _ = pairs_per_read(cols, sites, LENS)
    assert (n_pairs[:5] > 0).all() and set(cols["flags"].tolist()) == {0, 1}
    got = check(seng, sites, LENS, [reads], "bytes past 4 GiB", seq_from=base)
    assert int(got.sum()) == int(n_pairs.sum()) > 1000
    # the read that ended at seq_capacity, moved one byte on: the sticky word answers, and nothing is written
    off[1] += 1
    n_sites = len(sites[2])
    assert seng.pileup_reset(*sites) == n_sites
    seng.pileup_add(make(off))
    canary = torch.full((10 + 10 * n_sites + 10,), 0x5A5A5A5A, dtype=torch.int32, device=seng.device)
    assert seng.lib.simmr_pileup_read(seng._h, C.c_void_p(canary.data_ptr() + 40), n_sites) == _abi.EINVAL
    assert bool((canary == 0x5A5A5A5A).all())
