"""The column route of the model fit (simmr_fit_add; fit_kernels.hip, fit_device.hpp, fit.hip) past its first grid trip, flush, row
round and probe.  The cases come from tests/_fit_cases.py, whose builders assert that each byte sits on the lane, round or batch
it is for (tests/test_fit_host.py pins that without a GPU); what is expected is tests/_fit.model on the host columns — or, for
the flush case, uniform_batches' scaled model, which the host test holds to tests/_fit.model — compared by
tests/_fit.assert_model: integer tables and f32 probabilities exactly, f64 densities at the tolerance tests/_fit.assert_close
derives for n <= 1e5 observations (every case but the flush stays below that; the flush case has point masses only).  Every
size is a formula of tests/_fit.constants() and the CU count.

Which path each test is the first to enter:
  test_grid_trips
      k_fit_add's `batch += gridDim.x`: more than two trips of every workgroup, a third of one, a last batch of 8 reads (a paired
      shard has an even number of reads, so 32 x (2 x CUs + 1) + 8, not + 7); one add against three cut inside a batch;
  test_flush
      the flush at since_flush == FIT_FLUSH_BATCHES in the middle of the loop: three workgroups take 513 batches, with the dense
      table, the quality table, the lengths and the inserts all in LDS;
  test_round_seams
      `g0 += FIT_LANES`: carry_w / carry_h from lane 15 to lane 0 with a changed base on each side of offsets 256 and 512 for
      every k, the shuffle from a lane to the next at 16, and the window count where the last group holds 1 .. k + 1 bases;
  test_every_k
      k_fit_ref_scan with idle threads (k = 4), one entry a thread (5), the first share above one (6), and k = 9;
  test_pair_table_fills_and_wraps, test_pair_table_at_contract_load
      fit_pair_add's probe chains: a table filled to its last slot (chains as long as the table, through `& hmask`), one pair
      more (FIT_ERR_FULL), and the load the header promises to take (pair_capacity == the distinct changed pairs);
  test_insert_edges
      the insert histogram at FIT_LDS_LEN (LDS against HBM) and at SIMMR_FIT_MAX_INSERT (kept against dropped);
  test_quality_edges
      FIT_ERR_QUAL (q = 94, a byte below qual_offset) and q = 93 taken, in LDS and in HBM;
  test_longest_read
      the walker's bound on this route: FIT_MAX_L taken (256 rounds of a row), FIT_MAX_L + 1 refused;
  test_reset_clears_what_was_dirty
      simmr_fit_reset's partial clear after planned long reads, after an add without a plan, and across another k and capacity."""
import ctypes as C
import math
import time

import numpy as np
import pytest

from simmr_amd import MinimalShortErrorProfile, SimmrError, _abi
from tests import _fit, _oracle
from tests import _fit_cases as cases
from tests import test_gpu_fit as base
from tests.test_gpu_fit import fit, genomes, layout, oracle_columns  # noqa: F401 (genomes and layout are fixtures)

pytestmark = pytest.mark.gpu


def n_cu():
    """the count fit.hip sizes its grid from: hipDeviceProp_t::multiProcessorCount, which the binding does not expose"""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def same_bytes(a, b, what):
    assert a["model_bytes"] == b["model_bytes"], what
    for name in _abi.FIT_COLUMNS:
        assert np.array_equal(a[name], b[name]), (what, name)


def plan_code(engine):
    return engine.lib.simmr_fit_plan(engine._h, C.byref(_abi.FitInfo()))


def built(engine, oracle, genomes, specs, layout=0, seed=0):
    host = cases.reads_of(oracle, genomes, specs, np.random.default_rng(seed))
    return cases.device_reads(host, layout, engine.device), host


# ---- the batch loop ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trips(engine, oracle, genomes):
    """32 x (2 x CUs + 1) + 8 reads of minimal-short pairs in two lengths, shown to be the oracle's, as one set of columns, and
    the model of them (made once for both layouts)"""
    cus = n_cu()
    reads = cases.WG_READS * (2 * cus + 1) + 8
    shards = []
    for length, n, seed in ((40, reads // 4 * 2, 11), (150, reads - reads // 4 * 2, 12)):
        prof = MinimalShortErrorProfile(read_length=length, insert_size=60, mean_phred_score=14, rng_mode=_abi.RNG_PHILOX).pod()
        dev = engine.simulate_pe_reads_from_genome(1, prof, n, seed, qual_offset=33)
        shards.append(oracle_columns(dev, _oracle.simulate_pe(oracle, genomes[1], prof, n, seed, qual_offset=33)))
    host = cases.joined(shards)
    return host, _fit.model(oracle, [host], genomes, 2, 33, 7, 20), cus


def test_grid_trips(engine, genomes, layout, trips):
    host, want, cus = trips
    n = len(host["start"])
    batches = -(-n // cases.WG_READS)
    assert n == cases.WG_READS * (2 * cus + 1) + 8 and batches > 2 * min(batches, cus) and n < 100_000
    L = np.diff(host["seq_off"].astype(np.int64))
    assert L[: n // 2].mean() < 60 < 120 < L[n // 2:].mean()
    whole = fit(engine, [cases.device_reads(host, layout, engine.device)], 2, cap=1 << 20)  # (some 840 000 distinct changed pairs)
    _fit.assert_model(whole, want, f"{batches} batches on {cus} workgroups")
    assert whole["n_reads"] == n and whole["n_inserts"] > 0
    cuts = (0, cases.WG_READS * cus + 10, cases.WG_READS * cus + 12, n)  # inside a batch, and a shard of one pair
    parts = [cases.device_reads(cases.rows(host, a, b), layout, engine.device) for a, b in zip(cuts, cuts[1:])]
    same_bytes(fit(engine, parts, 2, cap=1 << 20), whole, "one add against three")


def test_flush(engine, oracle, genomes):
    import torch
    cus = n_cu()
    n_batches = cases.FLUSH_BATCHES * cus + 3
    assert math.ceil(n_batches / min(n_batches, cus)) == cases.FLUSH_BATCHES + 1 == 513
    t0 = time.perf_counter()
    try:
        big = cases.uniform_batches(oracle, genomes, n_batches)
        dev = cases.device_reads(big.host, 0, engine.device)
    except (SimmrError, MemoryError, torch.cuda.OutOfMemoryError) as e:
        if isinstance(e, SimmrError) and e.code != _abi.ENOMEM:
            raise
        pytest.skip("the memory cannot be had")
    got = fit(engine, [dev], 2, k=cases.UNIFORM_K)
    _fit.assert_model(got, big.model, f"{n_batches} uniform batches")
    assert got["n_reads"] == got["n_inserts"] == cases.WG_READS * n_batches
    del dev
    # the same engine without a flush: one workgroup's 512 batches on 512 workgroups, the same model scaled down
    small = cases.uniform_batches(oracle, genomes, cases.FLUSH_BATCHES)
    assert math.ceil(small.n_batches / min(small.n_batches, cus)) <= cases.FLUSH_BATCHES
    less = fit(engine, [cases.device_reads(small.host, 0, engine.device)], 2, k=cases.UNIFORM_K)
    _fit.assert_model(less, small.model, "uniform batches without a flush")
    for name in ("kmer_ref", "kmer_first", "pair_alt", "pair_prob", "qual_density", "length_density", "insert_density"):
        assert np.array_equal(less[name], got[name]), name
    for name in ("pair_count", "qual_hist", "length_hist", "insert_hist"):
        assert np.array_equal(less[name] * np.uint64(n_batches), got[name] * np.uint64(cases.FLUSH_BATCHES)), name
    print(f"test_flush: {cases.WG_READS * n_batches} reads, {time.perf_counter() - t0:.2f} s of wall time")


# ---- the row's rounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", cases.KS)
def test_round_seams(engine, oracle, genomes, layout, k):
    case = cases.seam_rows(k)
    dev, host = built(engine, oracle, genomes, case.specs, layout, k)
    got = fit(engine, [dev], 1, k=k)
    _fit.assert_model(got, _fit.model(oracle, [host], genomes, 1, 33, k, 20), f"rows at the columns {cases.EDGES}, k {k}")
    assert [int(got["length_hist"][v]) for v in (255, 256, 257, 258)] == [2, 2, 2, 2]
    assert got["n_pairs"] > got["n_ref_kmers"] > 0 and got["n_positions"] == case.n_positions and (k <= cases.LDS_K) == (k in (3, 7))


@pytest.mark.parametrize("k", [4, 5, 6, 9])
def test_every_k(engine, oracle, genomes, layout, k):
    base.test_hand_built_windows(engine, oracle, genomes, layout, k)


# ---- the pair table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 2, 4, 64, 128])
def test_pair_table_fills_and_wraps(engine, oracle, genomes, c):
    slots = 2 * c
    assert slots <= cases.MAX_PROBE and slots & (slots - 1) == 0  # a probe sees the whole table whatever the hash
    max_alt = 2 * cases.MAX_PROBE
    full = cases.full_table(slots)
    dev, host = built(engine, oracle, genomes, full.specs)
    got = fit(engine, [dev], 1, k=full.k, max_alt=max_alt, cap=c)
    _fit.assert_model(got, _fit.model(oracle, [host], genomes, 1, 33, full.k, max_alt), f"{slots} pairs in {slots} slots")
    assert got["n_pairs"] == slots + 1 and got["n_ref_kmers"] == 1 and sorted(got["pair_count"][1:]) == sorted(full.times)
    over = cases.full_table(slots + 1)
    dev, host = built(engine, oracle, genomes, over.specs)
    engine.fit_reset(over.k, max_alt, c)
    engine.fit_add(dev, 1)
    assert plan_code(engine) == _abi.ERANGE and b"full" in engine.lib.simmr_last_error(engine._h)
    got = fit(engine, [dev], 1, k=over.k, max_alt=max_alt, cap=2 * c)
    _fit.assert_model(got, _fit.model(oracle, [host], genomes, 1, 33, over.k, max_alt), f"{slots + 1} pairs in {2 * slots} slots")
    assert got["n_pairs"] == slots + 2


def test_pair_table_at_contract_load(engine, oracle, genomes):
    k, uncut, n = 10, 1 << 20, 250
    prof = MinimalShortErrorProfile(mean_phred_score=14, rng_mode=_abi.RNG_PHILOX).pod()
    dev = engine.simulate_pe_reads_from_genome(1, prof, n, 31, qual_offset=33)
    o = oracle_columns(dev, _oracle.simulate_pe(oracle, genomes[1], prof, n, 31, qual_offset=33))
    want = _fit.model(oracle, [o], genomes, 2, 33, k, uncut)
    D = len(want["pair_alt"]) - len(want["kmer_ref"])  # nothing is cut: every reference k-mer has its own pair and its changed ones
    slots = 1 << max(1, math.ceil(math.log2(2 * D)))
    print(f"test_pair_table_at_contract_load: {D} distinct changed pairs, {slots} slots")
    assert 20_000 < D <= slots // 2 and D > 0.4 * slots  # close to the half-full table the header allows
    got = fit(engine, [dev], 2, k=k, max_alt=uncut, cap=D)
    _fit.assert_model(got, want, f"pair_capacity {D}")
    assert got["n_pairs"] - got["n_ref_kmers"] == D


# ---- inserts, qualities, the longest read ------------------------------------------------------------------------------------
def test_insert_edges(engine, oracle, genomes, layout):
    case = cases.insert_pairs()
    dev, host = built(engine, oracle, genomes, case.specs, layout, 3)
    got = fit(engine, [dev], 2)
    _fit.assert_model(got, _fit.model(oracle, [host], genomes, 2, 33, 7, 20), "inserts at the edges")
    for span in (cases.LDS_LEN - 1, cases.LDS_LEN, _fit.MAX_INSERT):
        assert got["insert_hist"][span] == case.kept.count(span) >= 6, span
    assert got["n_inserts"] == len(case.kept) == got["insert_hist"].sum() and got["insert_hist"].size == _fit.MAX_INSERT + 1
    assert got["insert_hist"][_fit.MAX_INSERT + 1:].sum() == 0 and got["n_reads"] == 2 * len(case.spans)


def test_quality_edges(engine, oracle, genomes, layout):
    good = cases.quality_reads()
    dev, host = built(engine, oracle, genomes, good.specs, layout)
    got = fit(engine, [dev], 1)
    want = _fit.model(oracle, [host], genomes, 1, 33, 7, 20)
    _fit.assert_model(got, want, "q = 93")
    for j in good.at:
        assert got["qual_hist"][j, 93] == 4 and got["qual_hist"][j].sum() == 4, j
    assert good.at == (0, 159, 160, good.L - 1) and got["qual_hist"][:, 93].sum() == 16
    for byte in (33 + 94, 33 - 1):
        bad, _ = built(engine, oracle, genomes, cases.quality_reads(first=byte).specs, layout)
        engine.fit_reset(7, 20, 1 << 18)
        engine.fit_add(bad, 1)  # returns: the add only enqueues
        assert plan_code(engine) == _abi.EINVAL and b"quality" in engine.lib.simmr_last_error(engine._h)
        engine.fit_add(dev, 1)  # sticky until the reset
        with pytest.raises(SimmrError) as ei:
            engine.fit_model()
        assert ei.value.code == _abi.EINVAL
        same_bytes(fit(engine, [dev], 1), got, "the good reads after the reset")


def test_longest_read(engine, oracle, genomes, layout):
    case = cases.longest_reads()
    dev, host = built(engine, oracle, genomes, case.specs, layout)
    got = fit(engine, [dev], 1)
    _fit.assert_model(got, _fit.model(oracle, [host], genomes, 1, 33, 7, 20), "reads of FIT_MAX_L bases")
    assert got["n_positions"] == cases.MAX_L == 65535 and got["length_hist"][65535] == 2 and got["length_hist"][65534] == 1
    assert got["qual_hist"][65534].sum() == 2 and got["is_long"]
    bad, _ = built(engine, oracle, genomes, case.specs + case.too_long, layout)
    engine.fit_reset(7, 20, 1 << 18)
    engine.fit_add(bad, 1)
    assert plan_code(engine) == _abi.EINVAL and b"65535" in engine.lib.simmr_last_error(engine._h)
    same_bytes(fit(engine, [dev], 1), got, "the three good reads after the reset")


def test_reset_clears_what_was_dirty(engine, oracle, genomes):
    from simmr_amd.engine import Engine
    long_specs = [(0, 0, 5000 + 3000 * i, 1100 + 450 * i, i & 1, {7: 1, 1030 + i: 2}) for i in range(4)]
    short_specs = cases.seam_rows(3).specs[:26] + cases.full_table(9).specs

    def on_a_fresh_engine(specs, seed, **how):
        fresh = Engine(0)
        try:
            cases.stage(fresh, genomes)
            return fit(fresh, [built(fresh, oracle, genomes, specs, 0, seed)[0]], 1, **how)
        finally:
            fresh.close()
    want_long, want_short = on_a_fresh_engine(long_specs, 1), on_a_fresh_engine(short_specs, 2)
    want_short8 = on_a_fresh_engine(short_specs, 2, k=8, cap=1000)
    long_r, _ = built(engine, oracle, genomes, long_specs, 0, 1)
    short_r, _ = built(engine, oracle, genomes, short_specs, 0, 2)
    assert want_long["n_positions"] > cases.LDS_LEN and want_short["n_positions"] < 64
    same_bytes(fit(engine, [long_r], 1), want_long, "long reads, planned")
    same_bytes(fit(engine, [short_r], 1), want_short, "short reads after planned long ones")   # dirty_pos rows cleared
    engine.fit_reset(7, 20, 1 << 18)
    engine.fit_add(long_r, 1)                                                                   # no plan: unplanned_add
    same_bytes(fit(engine, [short_r], 1), want_short, "short reads after an add without a plan")
    same_bytes(fit(engine, [short_r], 1, k=8, cap=1000), want_short8, "another k and capacity")  # clean_dense / clean_slots
    same_bytes(fit(engine, [long_r], 1), want_long, "long reads again")
    same_bytes(fit(engine, [short_r], 1), want_short, "short reads at the end")
