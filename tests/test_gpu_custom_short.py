"""Custom-short pairs (k_emit_custom_pe, the custom branch of k_plan_pe) where the kernels' branches follow the model file:
table widths around 64 and 128 entries and the gather above, PDF headers at the end of the LDS image, bins that take the
whole word or reject words, lengths and inserts `as u16`, and the edges of the launch.  Every case is the device against
the oracle on every column, then the property of tests/_custom_pdf.py (written from the model alone) and the run counters.
tests/test_custom_short_models_host.py shows, without a GPU, that every case is at the edge it is named for."""
import os

import numpy as np
import pytest

from simmr_amd import SimmrError, _abi
from tests import _custom_pdf as cp
from tests import _oracle
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

SLOT = 34


def _both(engine, oracle, model, contigs, seed, reads=cp.READS, qoff=33, eng=None, max_len=1024, threads=cp.THREADS, **kw):
    """device and oracle on the same inputs: (device columns, oracle columns); counters left for the caller"""
    eng = eng or engine
    eng.stage_genome(SLOT, contigs)
    prof = model.profile()
    pod = prof.pod()
    eng.counters_reset()
    dev = eng.simulate_pe_reads_from_genome(SLOT, pod, reads, seed, qual_offset=qoff, **kw)
    ora = _oracle.simulate_pe(oracle, _oracle.HostGenome(contigs), pod, reads, seed, qual_offset=qoff, max_len=max_len,
                              threads=threads, **kw)
    d = dev.to_host()
    assert dev.total_bases == d["qual"].size
    return d, ora.trimmed()


def _check(engine, oracle, model, contigs, seed, qoff=33, what="", **kw):
    eng = kw.get("eng") or engine
    d, o = _both(engine, oracle, model, contigs, seed, qoff=qoff, **kw)
    assert_same(d, o, what=what)
    cp.qualities_allowed(model, d, qoff)
    c = eng.counters()
    raw = (d["qual"].astype(np.int64) - qoff) % 256
    assert c[_abi.CNT_QUAL_SUM] == raw.sum()
    assert c[_abi.CNT_SUBSTITUTIONS] == 0 and c[_abi.CNT_BASES] == d["qual"].size
    return d


@pytest.mark.parametrize("name", list(cp.CASES))
def test_directed_case(engine, oracle, name):
    """(a) the width ladder, (b) mixed shapes in one read, (c) the LDS header edge at n_quality 515, 511 and 512, (d) lengths
    1..16 and 480..520 in one wave, (e) a full-range bin at qual_offset 0 and 200, (f) rejecting bins on a 200-wide table,
    (g) lengths and inserts above 65535, (h) no insert PDF, (i) length and insert PDFs wider than 128 bins: 323 pairs each"""
    model, contigs, seed = cp.case_inputs(name)
    for qoff in cp.QOFF.get(name, (33,)):
        d = _check(engine, oracle, model, contigs, seed, qoff=qoff, what=f"{name} qoff {qoff}: ")
        L = np.diff(d["seq_off"].astype(np.int64))[0::2]
        assert L.size == cp.PAIRS
        if name == "d-divergent":
            assert set((L % 16).tolist()) == set(range(16))  # store_tail at every length mod 16
        if name == "g-as-u16":
            assert 90 <= L.min() and L.max() <= 140


def test_grid_loop_and_shard(engine, oracle, monkeypatch):
    """(j) SIMMR_GRID_MULT reaches launch_custom_pe (engine.hip: custom_pe_mult), but its smallest grid is 8 workgroups of
    256 pairs per CU, so the grid-stride loop is taken a second time only above 8 * 256 * n_cu pairs: 70 more than that, the
    last 70 in a second pass of workgroup 0.  The oracle's time grows with pairs x model bytes, so the (129, 129) tables
    stand at 8 positions and the lengths are 4..20 (they still pass n_quality).  Then a shard of the same run against that
    range of the whole."""
    import torch
    from simmr_amd.engine import Engine
    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    pairs = 8 * 256 * n_cu + 70
    model = cp.ladder_model(129, 129, lo=4, hi=20, positions=8)
    contigs = cp.case_genome(70)
    monkeypatch.setenv("SIMMR_GRID_MULT", "1")  # (read once, at engine creation)
    eng = Engine(0)
    try:
        d = _check(engine, oracle, model, contigs, 77, eng=eng, reads=2 * pairs + 1, max_len=20, threads=16, what="grid loop: ")
        assert d["read_id"].size == 2 * pairs
        prof = model.profile()
        part = eng.simulate_pe_reads_from_genome(SLOT, prof.pod(), 2 * pairs + 1, 77, first=131, count=200, qual_offset=33).to_host()
        lo, hi = 2 * 131, 2 * 331
        base = d["seq_off"][lo]
        assert np.array_equal(part["seq_off"], d["seq_off"][lo:hi + 1] - base)
        for c in ("start", "end", "contig", "read_id", "flags"):
            assert np.array_equal(part[c], d[c][lo:hi]), c
        for c in ("seq", "qual"):
            assert np.array_equal(part[c], d[c][int(base):int(d["seq_off"][hi])]), c
    finally:
        eng.close()


def test_full_range_length_bin_is_refused_by_both(engine, oracle):
    """a bin (0, 0xFFFFFFFF) in the LENGTH PDF: L is a random u16 and runs past every contig — an error on both sides"""
    model, contigs = cp.full_range_length_model(), cp.case_genome(50)
    engine.stage_genome(SLOT, contigs)
    prof = model.profile()
    with pytest.raises(RuntimeError):
        _oracle.simulate_pe(oracle, _oracle.HostGenome(contigs), prof.pod(), cp.READS, 9)
    with pytest.raises(SimmrError) as ei:
        engine.simulate_pe_reads_from_genome(SLOT, prof.pod(), cp.READS, 9)
    assert ei.value.code == _abi.ERANGE


@pytest.mark.parametrize("n", [2, 130], ids=["narrow", "wide"])
def test_bad_bin_on_each_path(engine, oracle, n):
    """(k) a density without a range, picked with probability 1, through the register tables and through the gather:
    SIMMR_ERANGE, and the engine goes on working"""
    model, contigs = cp.bad_bin_model(n), cp.case_genome(51)
    engine.stage_genome(SLOT, contigs)
    prof = model.profile()
    with pytest.raises(SimmrError) as ei:
        engine.simulate_pe_reads_from_genome(SLOT, prof.pod(), cp.READS, 1)
    assert ei.value.code == _abi.ERANGE
    model, contigs, seed = cp.case_inputs("a-ladder-64-64")
    _check(engine, oracle, model, contigs, seed, what="after the error: ")


# SIMMR_SWEEP_SEEDS=1,2,3: other sweeps for a soak run (as tests/test_gpu_random.py)
SWEEP_SEEDS = [int(x) for x in os.environ.get("SIMMR_SWEEP_SEEDS", "7,11,2024").split(",")]


@pytest.mark.parametrize("sweep_seed", SWEEP_SEEDS)
def test_random_custom_short_models(engine, oracle, sweep_seed):
    """60 random models (tests/_custom_pdf.py: sweep_case) on random genomes, read counts and shards: a refusal must be
    mutual; where both run, every column is the oracle's and the qualities are scores of their positions' PDFs"""
    rng = np.random.default_rng(sweep_seed)
    n_ok = 0
    for it in range(60):
        s = cp.sweep_case(rng)
        engine.stage_genome(SLOT, s["contigs"])
        prof = s["model"].profile()
        pod = prof.pod()
        kw = dict(first=s["first"], count=s["count"], read_id_base=3, qual_offset=s["qoff"])
        dev = ora = None
        dev_err = ora_err = ""
        try:
            ora = _oracle.simulate_pe(oracle, _oracle.HostGenome(s["contigs"]), pod, s["reads"], s["seed"], threads=cp.THREADS, **kw)
        except RuntimeError as ex:
            ora_err = str(ex)
        engine.counters_reset()
        try:
            dev = engine.simulate_pe_reads_from_genome(SLOT, pod, s["reads"], s["seed"], **kw)
        except SimmrError as ex:
            dev_err = str(ex)
        assert (dev is None) == (ora is None), (f"it{it}: device " + ("refused: " + dev_err if dev is None else "ran") +
                                                 ", oracle " + ("refused: " + ora_err if ora is None else "ran"))
        if dev is None:
            continue
        d = dev.to_host()
        assert_same(d, ora.trimmed(), what=f"it{it} ")
        cp.qualities_allowed(s["model"], d, s["qoff"])
        c = engine.counters()  # (lanes past their read's end, at random shapes, add nothing)
        assert c[_abi.CNT_QUAL_SUM] == ((d["qual"].astype(np.int64) - s["qoff"]) % 256).sum(), it
        assert c[_abi.CNT_SUBSTITUTIONS] == 0 and c[_abi.CNT_BASES] == d["qual"].size, it
        n_ok += 1
    assert n_ok >= 45
