"""Strain divergence on the device (simmr_strain_plan / simmr_strain_apply, include/simmr_hip.h) against the numpy
restatement of "strain sites, version 1" (tests/_strain.py): every case stages a genome, plans, applies and reads the contigs
back with simmr_unstage_contig; contigs and site columns must equal the model byte for byte."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import MinimalShortErrorProfile, SimmrError, _abi
from simmr_amd.engine import Engine
from tests import _oracle, _strain, _synth

pytestmark = pytest.mark.gpu
TILE, TOPS = _strain.constants()
SEED = 0x0123_4567_89AB_CDEF
IDENTITIES = [1.0, 0.97, 0.25]
CANARY = 0xA5


@pytest.fixture(scope="module")
def seng():
    """an engine of this module's own: the tests restage and rewrite its genome slots"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = Engine(0)
    yield e
    e.close()


def acgt(rng, n):
    return _strain.ACGT[rng.integers(0, 4, n)].copy()


def unstage_all(eng, slot, lens):
    return [eng.unstage(slot, c, 0, n) for c, n in enumerate(lens)]


def assert_diverged(eng, slot, contigs, identity, seed, what, sizes=None):
    """stage, plan + apply through Engine.strain, read back: planes and columns are the model's"""
    eng.stage_genome(slot, contigs, sizes)
    want_contigs, want = _strain.diverge(contigs, identity, seed)
    got = eng.strain(slot, identity, seed)
    for k in ("contig", "pos", "ref", "alt"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, got[k][:8], want[k][:8])
    back = unstage_all(eng, slot, [c.size for c in contigs])
    for c, (b, w) in enumerate(zip(back, want_contigs)):
        assert np.array_equal(b, w), (what, c, np.flatnonzero(b != w)[:8])
    return want


@pytest.mark.parametrize("identity", IDENTITIES)
def test_small_contigs(seng, identity):
    """contigs shorter than, equal to and one past a plane word, and one short of a 64-base boundary: one genome each, and all
    of them in one genome"""
    rng = np.random.default_rng(1)
    lens = [1, 3, 15, 16, 17, 63]
    contigs = [acgt(rng, n) for n in lens]
    for c in contigs:
        assert_diverged(seng, 0, [c], identity, SEED, f"one contig of {c.size}")
    want = assert_diverged(seng, 0, contigs, identity, SEED, "six small contigs")
    assert (want["pos"].size == 0) == (identity == 1.0)


@pytest.mark.parametrize("identity", IDENTITIES)
def test_tile_edges(seng, identity):
    rng = np.random.default_rng(2)
    for n in (TILE - 1, TILE, TILE + 1):
        want = assert_diverged(seng, 0, [acgt(rng, n)], identity, SEED, f"one contig of {n}")
        if identity < 1.0:
            assert want["pos"].size > 50 and want["pos"].max() >= n - 200  # sites up to the end of the last tile


@pytest.mark.parametrize("seed", [SEED, SEED ^ (1 << 40)], ids=["seed", "seed-high-word"])
@pytest.mark.parametrize("identity", IDENTITIES)
def test_three_contigs_and_both_seed_words(seng, identity, seed):
    """the contig index is in the counter, both seed words in the key: equal contigs get different sites"""
    rng = np.random.default_rng(3)
    a = acgt(rng, 2 * TILE + 100)
    want = assert_diverged(seng, 1, [a, a.copy(), acgt(rng, 777)], identity, seed, "three contigs")
    if identity < 1.0:
        p = [want["pos"][want["contig"] == c] for c in range(3)]
        assert all(x.size for x in p) and not np.array_equal(p[0], p[1])
        other = _strain.diverge([a], identity, seed ^ (1 << 40))[1]["pos"]
        assert not np.array_equal(p[0], other)


@pytest.mark.parametrize("identity", IDENTITIES)
def test_exception_runs_across_word_and_tile_boundaries(seng, identity):
    rng = np.random.default_rng(4)
    seq = acgt(rng, 3 * TILE + 41)
    seq[10:23] = ord("N")                    # crosses a word
    seq[TILE - 9:TILE + 30] = ord("-")       # crosses a tile
    seq[2 * TILE - 1:2 * TILE + 1] = ord("N")
    seq[rng.integers(0, seq.size, 400)] = ord("N")
    seq[-3:] = ord("-")
    want = assert_diverged(seng, 0, [acgt(rng, 100), seq], identity, SEED, "N and - runs")
    exc = (seq == ord("N")) | (seq == ord("-"))
    assert not exc[want["pos"][want["contig"] == 1].astype(np.int64)].any()


@pytest.mark.parametrize("identity", [0.97, 0.25])
def test_contiguous_style_genome(seng, identity):
    """a genome whose Seq.size differs from its length (--contiguous: records joined by 'N'): positions are Seq.seq's"""
    rng = np.random.default_rng(5)
    parts = [acgt(rng, n) for n in (500, 1, 2000)]
    whole = np.concatenate([np.concatenate([p, np.frombuffer(b"N", dtype=np.uint8)]) for p in parts])
    assert_diverged(seng, 2, [whole], identity, SEED, "contiguous", sizes=[sum(p.size for p in parts)])
    assert seng.genome_info(2) == (1, 2501)


@pytest.fixture(scope="module")
def looping():
    """just enough tiles that k_strain_scan_tiles' loop runs twice"""
    n = TOPS * TILE + 5 * TILE + 77
    assert TOPS < -(-n // TILE) <= 2 * TOPS
    return n, _synth.synthetic_contigs([n], 9)


@pytest.mark.parametrize("identity", IDENTITIES)
def test_scan_loops_twice(seng, looping, identity):
    n, contigs = looping
    seng.stage_synthetic(0, [n], 9)
    assert np.array_equal(seng.unstage(0, 0, n - 5000, 5000), contigs[0][-5000:])
    want_contigs, want = _strain.diverge(contigs, identity, SEED)
    got = seng.strain(0, identity, SEED)
    for k in ("contig", "pos", "ref", "alt"):
        assert np.array_equal(got[k], want[k]), (k, got[k][:8], want[k][:8])
    assert np.array_equal(seng.unstage(0, 0, 0, n), want_contigs[0])
    if identity < 1.0:
        assert want["pos"][-1] >= TOPS * TILE  # sites behind the first iteration's tiles
        assert seng.last_strain_ms() > 0.0


# ---- refusals and state ---------------------------------------------------------------------------------------------
def raw_plan(eng, slot, identity, seed):
    n = C.c_uint64(12345)
    return eng.lib.simmr_strain_plan(eng._h, slot, C.c_double(identity), C.c_uint64(seed), C.byref(n)), int(n.value)


class Columns:
    """the four columns between canaries: `n` entries, `pad` more on each side"""

    def __init__(self, eng, n, pad=64):
        import torch
        self.n, self.pad = n, pad
        self.t = {k: torch.full(((n + 2 * pad) * w,), CANARY, dtype=torch.uint8, device=eng.device)
                  for k, w in (("contig", 4), ("pos", 8), ("ref", 1), ("alt", 1))}
        self.w = {"contig": 4, "pos": 8, "ref": 1, "alt": 1}

    def pod(self, capacity, skip=()):
        p = {k: (None if k in skip else self.t[k].data_ptr() + self.pad * self.w[k]) for k in self.t}
        return _abi.StrainOut(p["contig"], p["pos"], p["ref"], p["alt"], capacity)

    def host(self, k):
        return self.t[k].cpu().numpy()

    def untouched(self, k):
        return bool((self.host(k) == CANARY).all())

    def canaries_hold(self, k):
        h, lo, hi = self.host(k), self.pad * self.w[k], (self.pad + self.n) * self.w[k]
        return bool((h[:lo] == CANARY).all() and (h[hi:] == CANARY).all())

    def column(self, k, dtype):
        h = self.host(k)
        return h[self.pad * self.w[k]:(self.pad + self.n) * self.w[k]].view(dtype)


@pytest.fixture()
def staged(seng):
    rng = np.random.default_rng(6)
    contigs = [acgt(rng, TILE + 300), acgt(rng, 90)]
    contigs[0][50:70] = ord("N")
    seng.stage_genome(0, contigs)
    return contigs


def planes_equal(eng, contigs, slot=0):
    return all(np.array_equal(b, c) for b, c in zip(unstage_all(eng, slot, [c.size for c in contigs]), contigs))


def test_plan_alone_changes_nothing(seng, staged):
    rc, n = raw_plan(seng, 0, 0.9, SEED)
    assert rc == 0 and n == _strain.diverge(staged, 0.9, SEED)[1]["pos"].size > 100
    assert planes_equal(seng, staged)
    # a second plan replaces the first
    assert raw_plan(seng, 0, 0.5, SEED) == (0, _strain.diverge(staged, 0.5, SEED)[1]["pos"].size)
    assert planes_equal(seng, staged)


def test_apply_without_columns_still_diverges(seng, staged):
    want, _ = _strain.diverge(staged, 0.9, SEED)
    assert seng.strain(0, 0.9, SEED, sites=False) == _strain.diverge(staged, 0.9, SEED)[1]["pos"].size
    assert planes_equal(seng, want)
    # a struct whose columns are all NULL, capacity 0
    seng.stage_genome(0, staged)
    assert raw_plan(seng, 0, 0.9, SEED)[0] == 0
    out = _abi.StrainOut(None, None, None, None, 0)
    assert seng.lib.simmr_strain_apply(seng._h, 0, C.byref(out)) == 0 and planes_equal(seng, want)


def test_columns_are_written_between_canaries_and_any_may_be_null(seng, staged):
    want_contigs, want = _strain.diverge(staged, 0.9, SEED)
    n = want["pos"].size
    for skip in ((), ("contig", "ref"), ("pos", "alt")):
        seng.stage_genome(0, staged)
        assert raw_plan(seng, 0, 0.9, SEED) == (0, n)
        cols = Columns(seng, n)
        out = cols.pod(n, skip)
        assert seng.lib.simmr_strain_apply(seng._h, 0, C.byref(out)) == 0
        for k, dt in (("contig", np.uint32), ("pos", np.uint64), ("ref", np.uint8), ("alt", np.uint8)):
            if k in skip:
                assert cols.untouched(k), k
            else:
                assert cols.canaries_hold(k) and np.array_equal(cols.column(k, dt), want[k]), k
        assert planes_equal(seng, want_contigs)


def test_short_capacity_is_refused_with_nothing_written(seng, staged):
    n = _strain.diverge(staged, 0.9, SEED)[1]["pos"].size
    assert raw_plan(seng, 0, 0.9, SEED) == (0, n)
    cols = Columns(seng, n)
    for capacity, skip in ((n - 1, ()), (0, ("contig", "pos", "ref"))):
        out = cols.pod(capacity, skip)
        assert seng.lib.simmr_strain_apply(seng._h, 0, C.byref(out)) == _abi.ERANGE
        assert all(cols.untouched(k) for k in cols.t) and planes_equal(seng, staged)
    # the plan is kept: the call with room goes through
    out = cols.pod(n)
    assert seng.lib.simmr_strain_apply(seng._h, 0, C.byref(out)) == 0 and not planes_equal(seng, staged)


def test_apply_needs_a_plan_for_that_genome_and_consumes_it(seng, staged):
    e = Engine(0)  # (an engine that never saw a strain plan)
    try:
        e.stage_genome(0, staged)
        assert e.lib.simmr_strain_apply(e._h, 0, None) == _abi.ESTATE and planes_equal(e, staged)
    finally:
        e.close()
    seng.stage_genome(1, staged)
    assert raw_plan(seng, 0, 0.9, SEED)[0] == 0
    assert seng.lib.simmr_strain_apply(seng._h, 1, None) == _abi.ESTATE  # planned for slot 0
    assert planes_equal(seng, staged) and planes_equal(seng, staged, 1)
    assert seng.lib.simmr_strain_apply(seng._h, 0, None) == 0
    want, _ = _strain.diverge(staged, 0.9, SEED)
    assert planes_equal(seng, want)
    # consumed: a genome is not diverged twice by accident
    cols = Columns(seng, 4096)
    out = cols.pod(4096)
    assert seng.lib.simmr_strain_apply(seng._h, 0, C.byref(out)) == _abi.ESTATE
    assert planes_equal(seng, want) and all(cols.untouched(k) for k in cols.t)


def test_a_staging_call_in_between_discards_the_plan(seng, staged):
    assert raw_plan(seng, 0, 0.9, SEED)[0] == 0
    seng.stage_genome(3, [staged[1]])  # another slot: the epoch still counts on
    cols = Columns(seng, 4096)
    out = cols.pod(4096)
    assert seng.lib.simmr_strain_apply(seng._h, 0, C.byref(out)) == _abi.ESTATE
    assert planes_equal(seng, staged) and all(cols.untouched(k) for k in cols.t)
    with pytest.raises(SimmrError) as err:
        seng._check(seng.lib.simmr_strain_apply(seng._h, 0, None))
    assert err.value.code == _abi.ESTATE


@pytest.mark.parametrize("identity", [0.2499, 1.0001, -1.0, float("nan"), float("inf")])
def test_identity_out_of_range_is_refused(seng, staged, identity):
    rc, n = raw_plan(seng, 0, identity, SEED)
    assert rc == _abi.EINVAL and n == 12345 and planes_equal(seng, staged)


def test_unstaged_slot_is_refused(seng, staged):
    assert raw_plan(seng, 57, 0.9, SEED)[0] == _abi.EINVAL
    assert seng.lib.simmr_strain_apply(seng._h, 57, None) == _abi.EINVAL
    assert seng.lib.simmr_strain_plan(seng._h, 0, C.c_double(0.9), C.c_uint64(1), None) == _abi.EINVAL


def test_truth_plan_made_before_an_apply_is_dropped(seng, staged):
    rng = np.random.default_rng(8)
    contigs = [acgt(rng, 20_000)]
    seng.stage_genome(0, contigs)
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX).pod()
    reads = seng.simulate_pe_reads_from_genome(0, prof, 200, 3)
    seng.truth_plan(reads)
    seng.strain(0, 0.97, SEED, sites=False)
    import torch
    nm = torch.zeros(reads.n_reads, dtype=torch.int32, device=seng.device)
    out = _abi.TruthOut(nm.data_ptr(), None, None, None, None, None, reads.n_reads, 0)
    pod = reads.pod()
    assert seng.lib.simmr_truth_emit(seng._h, C.byref(pod), C.byref(out)) == _abi.ESTATE
    # and so is the plan in force: an emit asks for a new one
    with pytest.raises(SimmrError):
        seng._check(seng.lib.simmr_pe_emit(seng._h, 0, C.byref(pod)))


# ---- end to end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng_mode", [_abi.RNG_REFERENCE, _abi.RNG_PHILOX], ids=["reference", "philox"])
def test_reads_are_drawn_from_the_diverged_planes(seng, oracle, rng_mode):
    """After an apply at 0.97 a minimal-short run's reads are the oracle's reads from the diverged contigs, and their truth
    (simmr_truth_*: a diff against the staged planes) is the model's truth of those reads against the diverged contigs — the
    sequencing errors, not the strain's sites: the emit kernels and the truth pass read the rewritten planes."""
    from tests.test_gpu_truth import check
    rng = np.random.default_rng(10)
    contigs = [acgt(rng, 60_000), acgt(rng, 9_001)]
    contigs[0][30_000:30_050] = ord("N")
    seng.stage_genome(0, contigs)
    diverged, sites = _strain.diverge(contigs, 0.97, SEED)
    assert seng.strain(0, 0.97, SEED, sites=False) == sites["pos"].size > 1500
    genomes = {0: _oracle.HostGenome(diverged)}
    prof = MinimalShortErrorProfile(rng_mode=rng_mode).pod()
    dev = seng.simulate_pe_reads_from_genome(0, prof, 2000, 11, qual_offset=33)
    ora = _oracle.simulate_pe(oracle, genomes[0], prof, 2000, 11, qual_offset=33)
    got = check(seng, oracle, genomes, dev, ora, "reads of the strain")
    # against the ORIGINAL contigs the same reads differ far more often: the strain's sites are in them
    from tests import _truth
    o = dict(ora.trimmed(), genome=dev.to_host()["genome"])
    against_original = _truth.model(oracle, o, {0: _oracle.HostGenome(contigs)})
    assert int(against_original["nm"].sum()) > int(got["nm"].sum()) + 5000
