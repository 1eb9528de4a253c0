"""Fitting an error model on the device (simmr_fit_reset / simmr_fit_add / simmr_fit_plan / simmr_fit_emit, include/simmr_hip.h)
against the plain restatement of its rules (tests/_fit.py), applied to the ORACLE's reads and the host genome bytes; the device
reads are first shown to be the oracle's, so nothing expected here comes from the pass under test.  Integer tables and the f32
probabilities are compared exactly, the f64 densities at the tolerance tests/_fit.assert_close derives."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import (CustomShortErrorProfile, MinimalLongErrorProfile, MinimalShortErrorProfile, PerfectShortErrorProfile,
                       SimmrError, _abi)
from tests import _fit, _fit_cases, _model, _oracle
from tests._hand_built import hand_built
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu
RNG_MODES = [_abi.RNG_REFERENCE, _abi.RNG_PHILOX, _abi.RNG_PHILOX_FULL]
RNG_IDS = ["reference", "philox", "philox-full"]
COLS = ("seq_off", "start", "end", "contig", "flags", "qual", "seq")


@pytest.fixture(scope="module")
def genomes(engine):
    # (the genomes of tests/test_gpu_truth.py)
    g = _fit_cases.host_genomes()
    _fit_cases.stage(engine, g)
    return g


@pytest.fixture(params=[0, 16], ids=["compact", "slot16"])
def layout(request, engine):
    engine.set_read_slots(request.param)
    try:
        yield request.param
    finally:
        engine.set_read_slots(0)


def fit(eng, shards, n_sets, k=7, max_alt=20, cap=1 << 18):
    eng.fit_reset(k, max_alt, cap)
    for s in shards:
        eng.fit_add(s, n_sets)
    return eng.fit_model()


def oracle_columns(dev, ora):
    """the device reads are the oracle's: the oracle's columns (with the device's genome column) for the model"""
    o, h = ora.trimmed(), dev.to_host()
    assert_same(h, o, cols=COLS)
    return dict(o, genome=h["genome"])


# ---- 1: hand-built reads ------------------------------------------------------------------------------------------------
def window_reads(oracle, genomes, device, layout, k, max_alt):
    """Reads copied from genome 1 contig 0 with chosen bytes altered: lengths k - 1, k, k + 1 and 2 k (0, 0, 1 and k windows),
    a written N (one, and k of them), alternates with equal counts, and more than max_alt alternates of one reference k-mer
    with a tie across the cut; and reads over the N / '-' runs of genome 3 (an expected N inside and at the edge of a window)."""
    specs = []  # genome, contig, lo, L, rev, {offset: byte}: tests/_fit_cases.py builds the columns
    for i, L in enumerate((k - 1, k, k + 1, 2 * k)):
        for rev in (0, 1):
            specs.append((1, 0, 500 + 40 * i, L, rev, {}))
    specs.append((1, 0, 2000, 3 * k, 0, {k: "N"}))                             # one written N
    specs.append((1, 0, 2100, 3 * k, 1, {j: "N" for j in range(k, 2 * k)}))    # k of them: an all-N query window
    specs.append((1, 0, 2200, 3 * k, 0, {0: "N", 3 * k - 1: "N"}))             # at the read's ends
    # one reference window (contig 0, 3000 .. 3000 + k) under max_alt + 6 different written k-mers: 3 k substitutions of one base
    # each (k >= 3: 9 .. 30 of them) seen once, so every count ties, across the cut too; two of them seen twice
    base = genomes[1].contigs[0][3000:3000 + k + 1]
    n_alt = 0
    for pos in range(k):
        for step in (1, 2, 3):
            ch = "ACGT"[("ACGT".find(chr(base[pos])) + step) % 4]
            specs.append((1, 0, 3000, k + 1, 0, {pos: ch}))
            n_alt += 1
            if n_alt in (2, 5):
                specs.append((1, 0, 3000, k + 1, 0, {pos: ch}))
    assert n_alt > max_alt
    for lo in (11_990, 11_995, 12_000 - k, 12_395, 12_400 - 1, 100, 731):      # the N run of genome 3: its edges inside windows
        for rev in (0, 1):
            specs.append((3, 0, lo, 4 * k, rev, {}))
    host = _fit_cases.reads_of(oracle, genomes, specs, np.random.default_rng(k))
    return _fit_cases.device_reads(host, layout, device), host


@pytest.mark.parametrize("k", [3, 7, 10])
def test_hand_built_windows(engine, oracle, genomes, layout, k):
    max_alt = 5
    dev, host = window_reads(oracle, genomes, engine.device, layout, k, max_alt)
    got = fit(engine, [dev], 1, k=k, max_alt=max_alt)
    want = _fit.model(oracle, [host], genomes, 1, 33, k, max_alt)
    _fit.assert_model(got, want, f"hand-built windows, k {k}")
    per_ref = np.diff(got["kmer_first"].astype(np.int64))
    assert per_ref.max() == max_alt and (got["pair_alt"] >> np.uint32(3 * (k - 1))).max() == 4  # the cut bites; an N-padded alternate
    i = int(np.argmax(per_ref))
    cut = got["pair_count"][int(got["kmer_first"][i]):int(got["kmer_first"][i + 1])]
    assert cut[-1] == 1 and float(got["pair_prob"][int(got["kmer_first"][i]):int(got["kmer_first"][i + 1])].sum()) < 1.0  # a tie across the cut, not renormalised


@pytest.mark.parametrize("n_sets", [1, 2])
def test_hand_built_columns(engine, oracle, genomes, layout, n_sets):
    """tests/_hand_built.py: lengths 0 .. 513 in both orientations, edits at the reads' ends, a written N, the N run of genome 3"""
    dev, host = hand_built(oracle, genomes, layout, engine.device, np.random.default_rng(5))
    got = fit(engine, [dev], n_sets)
    _fit.assert_model(got, _fit.model(oracle, [host], genomes, n_sets, 33, 7, 20), f"hand-built, {n_sets} sets")
    assert got["n_positions"] == 513 and got["qual_hist"][512].sum() >= 1 and got["n_reads"] == dev.n_reads


# ---- 2: simulated shards ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng_mode", RNG_MODES, ids=RNG_IDS)
def test_minimal_short_pairs(engine, oracle, genomes, layout, rng_mode):
    prof = MinimalShortErrorProfile(mean_phred_score=20, rng_mode=rng_mode).pod()
    dev = engine.simulate_pe_reads_from_genome(1, prof, 2001, 5, qual_offset=33)
    o = oracle_columns(dev, _oracle.simulate_pe(oracle, genomes[1], prof, 2001, 5, qual_offset=33))
    got = fit(engine, [dev], 2)
    _fit.assert_model(got, _fit.model(oracle, [o], genomes, 2, 33, 7, 20), "minimal-short pairs")
    assert got["n_inserts"] == dev.n_reads and got["n_insert_bins"] > 1 and not got["is_long"]
    assert (got["pair_alt"] != np.repeat(got["kmer_ref"], np.diff(got["kmer_first"].astype(np.int64)))).sum() > 1000  # changed windows
    assert engine.last_fit_ms() > 0


def test_one_add_against_three(engine, oracle, genomes, layout):
    prof = MinimalShortErrorProfile(mean_phred_score=14, rng_mode=_abi.RNG_PHILOX).pod()
    whole = engine.simulate_pe_reads_from_genome(1, prof, 1500, 9, qual_offset=33)
    parts = [engine.simulate_pe_reads_from_genome(1, prof, 1500, 9, first=f, count=c, qual_offset=33) for f, c in ((0, 400), (400, 1), (401, 1099))]
    a, b = fit(engine, [whole], 2), fit(engine, parts, 2)
    assert a["model_bytes"] == b["model_bytes"]
    for name in _abi.FIT_COLUMNS:
        assert np.array_equal(a[name], b[name]), name


def test_perfect_short_is_the_point_mass(engine, oracle, genomes):
    prof = PerfectShortErrorProfile().pod()
    dev = engine.simulate_pe_reads_from_genome(0, prof, 1000, 3, qual_offset=33)
    o = oracle_columns(dev, _oracle.simulate_pe(oracle, genomes[0], prof, 1000, 3, qual_offset=33))
    got = fit(engine, [dev], 2)
    _fit.assert_model(got, _fit.model(oracle, [o], genomes, 2, 33, 7, 20), "perfect-short")
    assert np.array_equal(np.diff(got["kmer_first"].astype(np.int64)), np.ones(got["n_ref_kmers"], dtype=np.int64))
    assert np.array_equal(got["pair_alt"], got["kmer_ref"]) and (got["pair_prob"] == np.float32(1.0)).all()
    point = np.zeros(_abi.FIT_DENSITIES)
    point[60] = 1.0
    assert got["n_positions"] > 0 and (got["qual_density"] == point).all()
    assert got["n_length_bins"] == 1 and got["length_density"][0] == 1.0 and got["length_lo"][0] == got["length_hi"][0] == got["n_positions"]


def test_minimal_long_reads_pass_512_positions(engine, oracle, genomes, layout):
    lp = MinimalLongErrorProfile(gamma_mean=600.0, gamma_std=400.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    dev = engine.simulate_long_reads([1, 0], [150, 100], lp, 3, qual_offset=33)
    o = oracle_columns(dev, _oracle.simulate_long(oracle, [genomes[1], genomes[0]], [150, 100], lp, 3, qual_offset=33))
    got = fit(engine, [dev], 1, k=8)
    _fit.assert_model(got, _fit.model(oracle, [o], genomes, 1, 33, 8, 20), "minimal-long")
    assert got["n_positions"] > 1024 and got["qual_hist"][-1].sum() == 1 and got["is_long"] and got["n_insert_bins"] == 0
    assert got["qual_density"][-1].sum() == 1.0  # one observation: the point mass


# ---- 3: the loop: fit, load, simulate ------------------------------------------------------------------------------------
def test_custom_short_model_fits_and_loads(engine, oracle, genomes):
    prof = CustomShortErrorProfile(_model.synthetic_short_model(n_positions=120, seed=42)).pod()
    dev = engine.simulate_pe_reads_from_genome(1, prof, 2001, 6, qual_offset=33)
    o = oracle_columns(dev, _oracle.simulate_pe(oracle, genomes[1], prof, 2001, 6, qual_offset=33))
    got = fit(engine, [dev], 2)
    _fit.assert_model(got, _fit.model(oracle, [o], genomes, 2, 33, 7, 20), "custom-short")
    fitted = CustomShortErrorProfile(got["model_bytes"]).pod()
    again = engine.simulate_pe_reads_from_genome(1, fitted, 500, 7, qual_offset=33)
    h = again.to_host()
    L = np.abs(h["end"].astype(np.int64) - h["start"].astype(np.int64))
    assert again.n_reads > 0 and L.min() >= int(got["length_lo"].min()) and L.max() <= int(got["length_hi"].max())


# ---- 4: errors -------------------------------------------------------------------------------------------------------------
def test_errors(engine, oracle, genomes):
    from simmr_amd.engine import Engine
    lib, h = engine.lib, engine._h
    prof = MinimalShortErrorProfile(mean_phred_score=14, rng_mode=_abi.RNG_PHILOX).pod()
    dev = engine.simulate_pe_reads_from_genome(1, prof, 1000, 9, qual_offset=33)
    pod, info = dev.pod(), _abi.FitInfo()
    for k in (2, 11):
        assert lib.simmr_fit_reset(h, k, 20, 1000) == _abi.EINVAL
    engine.fit_reset(7, 20, 1000)
    assert lib.simmr_fit_add(h, C.byref(pod), dev.n_reads, 3) == _abi.EINVAL
    assert lib.simmr_fit_add(h, C.byref(pod), dev.n_reads - 1, 2) == _abi.EINVAL
    noqual = dev.pod()
    noqual.qual = None
    assert lib.simmr_fit_add(h, C.byref(noqual), dev.n_reads, 2) == _abi.EINVAL and b"qual" in lib.simmr_last_error(h)
    assert lib.simmr_fit_emit(h, C.byref(_abi.FitOut())) == _abi.ESTATE  # no plan yet
    # a pair table too small
    engine.fit_reset(7, 20, 1)
    engine.fit_add(dev, 2)
    assert lib.simmr_fit_plan(h, C.byref(info)) == _abi.ERANGE
    # a genome staged between the reset and the add: the tables are sums over reads and the add reads what is staged when it
    # runs (the rule of the statistics pass), so the model is that of the same reads without the staging call
    want = fit(engine, [dev], 2)
    engine.fit_reset(7, 20, 1 << 18)
    engine.stage_genome(5, [genomes[3].contigs[0][:5000]])
    engine.fit_add(dev, 2)
    assert engine.fit_model()["model_bytes"] == want["model_bytes"]
    # a read naming an unstaged slot: sticky until the reset
    def spoil(cols, specs):
        cols["genome"][5] = 77
    bad, _ = hand_built(oracle, genomes, 0, engine.device, np.random.default_rng(5), spoil)
    engine.fit_reset(7, 20, 1 << 18)
    engine.fit_add(bad, 1)  # returns: the add only enqueues
    assert lib.simmr_fit_plan(h, C.byref(info)) == _abi.EINVAL
    engine.fit_add(dev, 2)
    with pytest.raises(SimmrError) as ei:
        engine.fit_model()
    assert ei.value.code == _abi.EINVAL
    fresh = Engine(0)
    try:
        assert fresh.lib.simmr_fit_add(fresh._h, C.byref(pod), dev.n_reads, 2) == _abi.ESTATE
        assert fresh.lib.simmr_fit_plan(fresh._h, C.byref(info)) == _abi.ESTATE
    finally:
        fresh.close()
