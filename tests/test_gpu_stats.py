"""Run statistics on the device (simmr_stats_reset / simmr_stats_add / simmr_stats_read, include/simmr_hip.h) against the
numpy restatement of the header's tables (tests/_stats.py), applied to the ORACLE's reads and the host genome bytes; the
device reads are first shown to be the oracle's, so nothing expected here comes from the pass under test.  Every comparison
is exact."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import (CustomShortErrorProfile, MinimalLongErrorProfile, MinimalShortErrorProfile, PerfectShortErrorProfile,
                       SimmrError, _abi)
from tests import _model, _oracle, _stats, _synth
from tests._hand_built import hand_built
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu
RNG_MODES = [_abi.RNG_REFERENCE, _abi.RNG_PHILOX, _abi.RNG_PHILOX_FULL]
RNG_IDS = ["reference", "philox", "philox-full"]
COLS = ("seq_off", "start", "end", "contig", "flags", "qual", "seq")


@pytest.fixture(scope="module")
def genomes(engine):
    # (the genomes of tests/test_gpu_truth.py)
    rng = np.random.default_rng(21)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30000)].copy()
    seq[rng.integers(0, 30000, 3000)] = ord("N")
    seq[rng.integers(0, 30000, 500)] = ord("-")
    seq[12_000:12_400] = ord("N")
    g = {0: _oracle.HostGenome(_synth.synthetic_contigs([1_000_000], 1)),
         1: _oracle.HostGenome(_synth.synthetic_contigs([300_000, 90_001, 30_017, 70_000, 123_457], 7)),
         3: _oracle.HostGenome([seq])}
    engine.stage_synthetic(0, [1_000_000], 1)
    engine.stage_genome(1, g[1].contigs)
    engine.stage_genome(3, g[3].contigs)
    return g


@pytest.fixture(params=[0, 16], ids=["compact", "slot16"])
def layout(request, engine):
    engine.set_read_slots(request.param)
    try:
        yield request.param
    finally:
        engine.set_read_slots(0)


def device_stats(eng, reads, n_sets):
    eng.stats_reset()
    eng.stats_add(reads, n_sets)
    return eng.stats()


def check(eng, oracle, genomes, dev, ora, n_sets, what, qual_offset=33):
    """the device reads are the oracle's; the device tables are the model of the oracle's reads"""
    o, h = ora.trimmed(), dev.to_host()
    assert_same(h, o, cols=COLS)
    o = dict(o, genome=h["genome"])
    want = _stats.model(oracle, o, genomes, n_sets, qual_offset)
    got = device_stats(eng, dev, n_sets)
    _stats.assert_stats(got, want, what)
    return got, want, o


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng_mode", RNG_MODES, ids=RNG_IDS)
def test_minimal_short_pairs(engine, oracle, genomes, layout, rng_mode):
    prof = MinimalShortErrorProfile(rng_mode=rng_mode).pod()
    for gidx, reads, seed, first, count in ((1, 3001, 5, 0, _abi.U64_MAX), (0, 8000, 42, 1100, 900)):
        dev = engine.simulate_pe_reads_from_genome(gidx, prof, reads, seed, first=first, count=count, qual_offset=33)
        ora = _oracle.simulate_pe(oracle, genomes[gidx], prof, reads, seed, first=first, count=count, qual_offset=33)
        got, _, o = check(engine, oracle, genomes, dev, ora, 2, f"genome {gidx} first {first}")
        assert got["reads"][0] == got["reads"][1] == dev.n_reads // 2 and got["qual_mismatch"].sum() > 0
        assert got["qual_n"].sum() == got["bases"].sum() == got["pair"].sum() == got["cycle_n"].sum()


def test_raw_phred_qualities(engine, oracle, genomes, layout):
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX).pod()
    dev = engine.simulate_pe_reads_from_genome(1, prof, 3001, 5, qual_offset=0)
    ora = _oracle.simulate_pe(oracle, genomes[1], prof, 3001, 5, qual_offset=0)
    got, _, _ = check(engine, oracle, genomes, dev, ora, 2, "qual_offset 0", qual_offset=0)
    dev33 = engine.simulate_pe_reads_from_genome(1, prof, 3001, 5, qual_offset=33)
    _stats.assert_stats(device_stats(engine, dev33, 2), got, "the same Phred scores behind either offset")


# ---- 2 ----------------------------------------------------------------------------------------------------------------
def test_accumulation_and_reset(engine, oracle, genomes, layout):
    prof = MinimalShortErrorProfile(mean_phred_score=14, rng_mode=_abi.RNG_PHILOX).pod()
    shards, models = [], []
    for gidx, reads, seed in ((1, 2001, 5), (0, 1500, 9)):
        dev = engine.simulate_pe_reads_from_genome(gidx, prof, reads, seed, qual_offset=33)
        o = dict(_oracle.simulate_pe(oracle, genomes[gidx], prof, reads, seed, qual_offset=33).trimmed())
        assert_same(dev.to_host(), o, cols=COLS)
        o["genome"] = dev.to_host()["genome"]
        shards.append(dev)
        models.append(_stats.model(oracle, o, genomes, 2, 33))
    engine.stats_reset()
    _stats.assert_stats(engine.stats(), _stats.zeros(), "after a reset")
    engine.stats_add(shards[0], 2)
    _stats.assert_stats(engine.stats(), models[0], "first shard")  # (a read between two adds)
    engine.stats_add(shards[1], 2)
    _stats.assert_stats(engine.stats(), _stats.add(models[0], models[1]), "both shards")
    assert engine.last_stats_ms() > 0
    engine.stats_reset()
    _stats.assert_stats(engine.stats(), _stats.zeros(), "after the second reset")


# ---- 3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng_mode", [_abi.RNG_REFERENCE, _abi.RNG_PHILOX], ids=["reference", "philox"])
def test_exception_bases_are_class_other(engine, oracle, genomes, layout, rng_mode):
    prof = MinimalShortErrorProfile(mean_phred_score=8, rng_mode=rng_mode).pod()
    dev = engine.simulate_pe_reads_from_genome(3, prof, 3000, 8, qual_offset=33)
    ora = _oracle.simulate_pe(oracle, genomes[3], prof, 3000, 8, qual_offset=33)
    got, want, _ = check(engine, oracle, genomes, dev, ora, 2, "N and - runs")
    assert got["pair"][4].sum() > 0 and got["pair"][:, 4].sum() > 0
    assert np.array_equal(got["pair"][4], want["pair"][4]) and np.array_equal(got["pair"][:, 4], want["pair"][:, 4])
    assert got["pair"].sum() - np.trace(got["pair"]) == got["qual_mismatch"].sum() > 1000


# ---- 4 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng_mode", [_abi.RNG_REFERENCE, _abi.RNG_PHILOX], ids=["reference", "philox"])
def test_long_reads_two_genomes(engine, oracle, genomes, layout, rng_mode):
    lp = MinimalLongErrorProfile(gamma_mean=3000.0, gamma_std=2500.0, length_mode=_abi.LEN_PER_READ, rng_mode=rng_mode).pod()
    dev = engine.simulate_long_reads([1, 0], [150, 100], lp, 3, qual_offset=33)
    ora = _oracle.simulate_long(oracle, [genomes[1], genomes[0]], [150, 100], lp, 3, qual_offset=33)
    got, _, o = check(engine, oracle, genomes, dev, ora, 1, "long reads")
    L = np.abs(o["end"].astype(np.int64) - o["start"].astype(np.int64))
    assert L.max() > 4096 and set(np.unique(o["genome"])) == {0, 1}
    assert got["reads"][0] == 250 and got["reads"][1] == 0 and not got["cycle_n"][1].any()
    assert got["cycle_n"].sum() == np.minimum(L, 512).sum() < got["bases"][0] == got["qual_n"].sum() == L.sum()


def test_long_reads_of_65535_bases(engine, oracle, genomes, layout):
    lp = MinimalLongErrorProfile(gamma_mean=200000.0, gamma_std=200.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    dev = engine.simulate_long_reads([0], [6], lp, 9, qual_offset=33)
    ora = _oracle.simulate_long(oracle, [genomes[0]], [6], lp, 9, qual_offset=33)
    got, _, _ = check(engine, oracle, genomes, dev, ora, 1, "65 535-base reads")
    assert got["bases"][0] == 6 * 65535 == got["qual_n"].sum() == got["pair"].sum()
    assert (got["cycle_n"][0] == 6).all() and got["cycle_base"].sum() == 6 * 512
    assert got["nm_hist"].sum() == 6 and got["gc_hist"].sum() == 6


# ---- 5 ----------------------------------------------------------------------------------------------------------------
def test_custom_short_model_quality_per_cycle(engine, oracle, genomes):
    prof = CustomShortErrorProfile(_model.synthetic_short_model(n_positions=120, seed=42)).pod()
    dev = engine.simulate_pe_reads_from_genome(1, prof, 3001, 6, qual_offset=33)
    ora = _oracle.simulate_pe(oracle, genomes[1], prof, 3001, 6, qual_offset=33)
    got, want, _ = check(engine, oracle, genomes, dev, ora, 2, "custom short model")
    assert np.array_equal(got["cycle_qsum"], want["cycle_qsum"]) and got["cycle_qsum"][:, :80].all()
    assert not np.array_equal(got["cycle_qsum"][0, :80] * got["cycle_n"][0, 0], got["cycle_qsum"][0, 0] * got["cycle_n"][0, :80])  # (per-position laws)


# ---- 6 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sets", [1, 2])
def test_hand_built_columns(engine, oracle, genomes, layout, n_sets):
    dev, host = hand_built(oracle, genomes, layout, engine.device, np.random.default_rng(5))
    want = _stats.model(oracle, host, genomes, n_sets, 33)
    got = device_stats(engine, dev, n_sets)
    _stats.assert_stats(got, want, f"hand-built, {n_sets} sets")
    assert got["nm_hist"][63] == 2 and got["gc_hist"][100] >= 2 and got["reads"].sum() == dev.n_reads
    assert got["pair"][:4, 4].sum() > 0 and got["pair"][4, :4].sum() > 0 and got["cycle_n"][:, 511].sum() == 9
    if layout == 16:  # the same reads in either layout
        other, _ = hand_built(oracle, genomes, 0, engine.device, np.random.default_rng(5))
        _stats.assert_stats(device_stats(engine, other, n_sets), got, "compact against slot16")


# ---- 7 ----------------------------------------------------------------------------------------------------------------
def test_workgroups_loop(engine, oracle, genomes):
    import torch
    defines = _stats.constants()
    wg_reads, per_cu = defines["STATS_WG_READS"], defines["STATS_WGS_PER_CU"]
    assert defines["STATS_LANES"] * wg_reads == 256
    grid_cap = per_cu * int(torch.cuda.get_device_properties(0).multi_processor_count)
    n_reads = 2 * grid_cap * wg_reads + 7 * wg_reads + 2
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
    engine.set_read_slots(16)
    try:
        engine.counters_reset()
        dev = engine.simulate_pe_reads_from_genome(0, prof, n_reads, 42, qual_offset=33)
    finally:
        engine.set_read_slots(0)
    subs = int(engine.counters()[_abi.CNT_SUBSTITUTIONS])
    assert dev.slot_bytes == 16 and -(-dev.n_reads // wg_reads) >= 2 * grid_cap, "resize: every workgroup must take two batches"
    ora = _oracle.simulate_pe(oracle, genomes[0], prof, n_reads, 42, qual_offset=33, max_len=160)
    got, _, o = check(engine, oracle, genomes, dev, ora, 2, "workgroups loop")
    L = np.abs(o["end"].astype(np.int64) - o["start"].astype(np.int64))
    assert got["qual_mismatch"].sum() == int(engine.truth(dev).nm[:dev.n_reads].sum()) == subs > 0
    assert got["bases"].sum() == L.sum() and got["cycle_n"][:, 0].sum() == np.count_nonzero(L)


# ---- 8 ----------------------------------------------------------------------------------------------------------------
def test_a_byte_changed_after_the_emit_moves_one_count(engine, oracle, genomes, layout):
    prof = PerfectShortErrorProfile().pod() if layout == 0 else MinimalShortErrorProfile(mean_phred_score=90, rng_mode=_abi.RNG_PHILOX).pod()
    dev = engine.simulate_pe_reads_from_genome(0, prof, 400, 11, qual_offset=33)
    assert dev.slot_bytes == layout
    base = device_stats(engine, dev, 2)
    assert base["qual_mismatch"].sum() == 0 and np.trace(base["pair"]) == base["pair"].sum()
    raw = dev.raw_to_host()
    r, j = 11, 37  # a reverse mate (set 1)
    assert raw["flags"][r] & 1
    first = int(raw["seq_off"][r])
    old = chr(int(raw["seq"][first + j]))
    new = "ACGT"[("ACGT".index(old) + 2) % 4]
    q = (int(raw["qual"][((first & ~15) if layout == 16 else first) + j]) - 33) & 255
    dev.seq[first + j] = ord(new)
    got = device_stats(engine, dev, 2)
    e, w = "ACGT".index(old), "ACGT".index(new)
    want = {k: v.copy() for k, v in base.items()}
    want["pair"][e, e] -= 1; want["pair"][e, w] += 1
    want["qual_mismatch"][q] += 1
    want["cycle_mismatch"][1, j] += 1
    want["cycle_base"][1, j, e] -= 1; want["cycle_base"][1, j, w] += 1
    want["nm_hist"][0] -= 1; want["nm_hist"][1] += 1
    L = abs(int(raw["end"][r]) - int(raw["start"][r]))
    seq = raw["seq"][first:first + L].copy()
    gc = lambda s: 100 * int(np.isin(s, list(b"GC")).sum()) // L
    want["gc_hist"][gc(seq)] -= 1
    seq[j] = ord(new)
    want["gc_hist"][gc(seq)] += 1
    _stats.assert_stats(got, want, "one byte changed")


# ---- 9 ----------------------------------------------------------------------------------------------------------------
def test_bad_reads_answer_through_the_error_word(engine, oracle, genomes, layout):
    def spoil(cols, specs):
        r = next(i for i, s in enumerate(specs) if s[3] == 150 and not s[4])  # the read that ends at its contig's end
        cols["start"][r] += 10
        cols["end"][r] += 10                                                  # the same length, ten bases past the end
        cols["genome"][5] = 77                                                # not a staged slot
    bad, _ = hand_built(oracle, genomes, layout, engine.device, np.random.default_rng(5), spoil)
    good, host = hand_built(oracle, genomes, layout, engine.device, np.random.default_rng(5))
    engine.stats_reset()
    engine.stats_add(bad, 2)  # returns: the add only enqueues
    with pytest.raises(SimmrError) as ei:
        engine.stats()
    assert ei.value.code == _abi.EINVAL
    engine.stats_add(good, 2)
    with pytest.raises(SimmrError):  # sticky until the reset
        engine.stats()
    engine.stats_reset()
    engine.stats_add(good, 2)
    _stats.assert_stats(engine.stats(), _stats.model(oracle, host, genomes, 2, 33), "after the reset")


# ---- 10 ---------------------------------------------------------------------------------------------------------------
def test_argument_checks(engine, genomes):
    from simmr_amd.engine import Engine
    dev = engine.simulate_pe_reads_from_genome(1, PerfectShortErrorProfile().pod(), 200, 3, qual_offset=33)
    lib, h = engine.lib, engine._h
    engine.stats_reset()
    pod = dev.pod()
    assert lib.simmr_stats_add(h, C.byref(pod), dev.n_reads, 3) == _abi.EINVAL
    assert lib.simmr_stats_add(h, C.byref(pod), dev.n_reads, 0) == _abi.EINVAL
    noqual = dev.pod()
    noqual.qual = None
    assert lib.simmr_stats_add(h, C.byref(noqual), dev.n_reads, 2) == _abi.EINVAL
    assert b"qual" in lib.simmr_last_error(h)
    _stats.assert_stats(engine.stats(), _stats.zeros(), "refused adds add nothing")
    fresh = Engine(0)
    try:
        st = _abi.RunStats()
        assert fresh.lib.simmr_stats_read(fresh._h, C.byref(st)) == _abi.ESTATE
        assert fresh.lib.simmr_stats_add(fresh._h, C.byref(pod), dev.n_reads, 2) == _abi.ESTATE
    finally:
        fresh.close()
