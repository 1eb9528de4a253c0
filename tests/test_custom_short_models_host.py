"""The shaped custom-short models of tests/_custom_pdf.py against the oracle alone (no GPU): every builder's blob reads back
as what it was made from, every directed case of tests/test_gpu_custom_short.py runs on the oracle, gives qualities that
the model allows (a property stated without the oracle's code) and really is at the edge it is named for, and the random
sweep's generator mostly gives models that run."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _custom_pdf as cp
from tests import _oracle


def _same_bins(got: cp.OrcBins, want):
    density, ranges = got.lists()
    assert density == [float(x) for x in want[0]]  # (f64 written and read back: exact)
    assert ranges == [(int(a), int(b)) for a, b in want[1]]


def _roundtrip(oracle, model):
    m = cp.parse_with_oracle(oracle, model.blob)
    assert m.n_quality == model.n_quality and not m.is_long
    for p in range(model.n_quality):
        _same_bins(m.quality[p], model.quality[p])
    _same_bins(m.read_length_bins, model.length)
    assert bool(m.has_insert_bins) == (model.insert is not None)
    if model.insert is not None:
        _same_bins(m.insert_bins, model.insert)
    assert m.read_length_mean == model.len_mean and m.insert_size_mean == model.ins_mean
    oracle.orc_custom_new.restype = C.c_void_p
    oracle.orc_custom_new.argtypes = [C.c_char_p, C.c_uint64]
    oracle.orc_custom_minimum_genome_size.restype = C.c_uint16
    oracle.orc_custom_minimum_genome_size.argtypes = [C.c_void_p]
    c = oracle.orc_custom_new(model.blob, len(model.blob))
    assert c and oracle.orc_custom_minimum_genome_size(c) == model.required


@pytest.mark.parametrize("name", list(cp.CASES))
def test_case_models_roundtrip(oracle, name):
    model = cp.CASES[name]()
    _roundtrip(oracle, model)
    if name.startswith("a-ladder"):
        n, nb = (int(x) for x in name.split("-")[2:])
        assert all((len(d), len(r)) == (n, nb) for d, r in model.quality) and model.n_quality == 60
        if n > nb:  # the surplus densities are exact zeros
            assert all(x == 0.0 for d, _ in model.quality for x in d[nb:])


def test_other_builders_roundtrip(oracle):
    for model in (cp.full_range_length_model(), cp.bad_bin_model(2), cp.bad_bin_model(130)):
        _roundtrip(oracle, model)
    rng = np.random.default_rng(3)
    for _ in range(5):
        _roundtrip(oracle, cp.sweep_case(rng)["model"])


def test_allowed_scores_is_what_the_model_says():
    """the property's table on hand-written PDFs: zero densities, a wide bin, a score past 255, a surplus density, the clamp
    to the last PDF, a bin that allows every byte"""
    q = [([0.5, 0.0, 0.5], [(3, 3), (9, 9), (250, 258)]),
         ([0.2, 0.8, 0.0], [(7, 7), (300, 300)]),
         ([0.7, 0.3], [(1, 1), cp.FULL])]
    m = cp.Model(q, ([1.0], [(5, 5)]), None, 5, 0)
    a, every = cp.allowed_scores(m, 0)
    assert not every and set(np.flatnonzero(a)) == {3, 250, 251, 252, 253, 254, 255, 0, 1, 2}
    a, every = cp.allowed_scores(m, 1)
    assert not every and set(np.flatnonzero(a)) == {7, 300 - 256}
    for p in (2, 3, 99):
        assert cp.allowed_scores(m, p)[1]
    cols = {"seq_off": np.array([0, 2, 4], np.uint64), "qual": np.array([36, 40, (33 + 255) % 256, 77], np.uint8)}
    assert cp.qualities_allowed(m, cols, 33) == 0
    cols["qual"][3] = 33 + 8  # position 1 of the second read: 8 is no score of PDF 1
    with pytest.raises(AssertionError):
        cp.qualities_allowed(m, cols, 33)
    cols["qual"][3] = 33 + 3  # a score of PDF 0 only
    with pytest.raises(AssertionError):
        cp.qualities_allowed(m, cols, 33)


def _oracle_run(oracle, model, contigs, seed, reads=cp.READS, qoff=33, **kw):
    prof = model.profile()
    return _oracle.simulate_pe(oracle, _oracle.HostGenome(contigs), prof.pod(), reads, seed, qual_offset=qoff, threads=cp.THREADS, **kw).trimmed()


@pytest.mark.parametrize("name", list(cp.CASES))
def test_directed_cases_on_the_oracle(oracle, name):
    model, contigs, seed = cp.case_inputs(name)
    assert min(c.size for c in contigs) > model.required
    for qoff in cp.QOFF.get(name, (33,)):
        out = _oracle_run(oracle, model, contigs, seed, qoff=qoff)
        lens = np.diff(out["seq_off"].astype(np.int64))
        L = lens[0::2]
        assert L.size == cp.PAIRS and np.array_equal(L, lens[1::2])
        skipped = cp.qualities_allowed(model, out, qoff)
        widths = [(len(d), len(r)) for d, r in model.quality]
        if name.startswith("a-ladder"):
            assert L.min() < model.n_quality < L.max() and 40 <= L.min() and L.max() <= 90  # L passes n_quality
        elif name == "b-mixed":
            below = widths[:int(L.min())]
            assert any(cp.is_narrow(w) for w in below) and any(not cp.is_narrow(w) for w in below)
            assert set(below) == set(cp.MIXED)  # every shape of the cycle, so every change of shape between neighbours
        elif name.startswith("c-lds-edge"):
            assert (L > 512).sum() >= 20 and (L < 510).sum() >= 20 and L.max() > model.n_quality
        elif name == "d-divergent":
            assert set((L % 16).tolist()) == set(range(16)) and (L <= 16).sum() >= 64 and (L >= 480).sum() >= 64
        elif name == "e-full-range":
            assert skipped > 0.2 * out["qual"].size * 5 / 90  # (every read has at least positions 0, 7, 16 and 33)
            full = (out["qual"].astype(np.int64) - qoff) % 256
            p0 = full[out["seq_off"][:-1].astype(np.int64)]
            assert (p0 >= 70).sum() > 50  # position 0's full-range bin is drawn, and its word's low byte is kept
        elif name == "g-as-u16":
            # every L is the drawn score mod 65536: the scores drawn again here, from the pairs' seeds and the length PDF
            assert L.max() < 65536 and 90 <= L.min() and L.max() <= 140
            cidx = np.zeros(cp.PAIRS, np.uint32)
            seeds = np.zeros(cp.PAIRS, np.uint64)
            assert oracle.orc_pe_outer(3, seed, 0, cp.PAIRS, cidx.ctypes.data, seeds.ctypes.data, None) == 0
            m = cp.parse_with_oracle(oracle, model.blob)
            pdf = (C.c_uint8 * 256)()  # opaque orc_pdf storage
            oracle.orc_pdf_new.argtypes = [C.POINTER(cp.OrcBins), C.c_void_p]
            oracle.orc_pdf_sample.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]
            assert oracle.orc_pdf_new(C.byref(m.read_length_bins), pdf) == 0
            v = C.c_uint32()
            for k in range(cp.PAIRS):
                assert oracle.orc_pdf_sample(pdf, int(seeds[k]), C.byref(v)) == 0
                assert v.value >= 65536 + 90 and v.value % 65536 == L[k]
        elif name == "h-no-insert":
            mate1, mate2 = out["start"][0::2].astype(np.int64), out["end"][1::2].astype(np.int64)  # (fwd_start, rev_end)
            redrawn = (out["flags"][1::2] & _abi.FLAG_REDRAWN) != 0
            assert (np.where(mate1 < L, mate2 == 0, mate2 == mate1 - L) | redrawn).all() and (mate2 == 0).sum() > 0
        elif name == "i-wide-length-insert":
            assert len(model.length[0]) > 128 and len(model.insert[0]) > 128 and len(set(L.tolist())) > 100


def test_expected_refusals_on_the_oracle(oracle):
    """a full-range bin in the length PDF draws L as a random u16: no contig here holds such reads.  A density without a
    range that takes all the weight: the reference's index panic."""
    contigs = cp.case_genome(50)
    for model in (cp.full_range_length_model(), cp.bad_bin_model(2), cp.bad_bin_model(130)):
        with pytest.raises(RuntimeError):
            _oracle_run(oracle, model, contigs, 9)


def test_sweep_generator_mostly_runs_on_the_oracle(oracle):
    """the generator of test_gpu_custom_short.py's random sweep, with that test's default seeds: at least 50 of 60
    iterations run, every other one is a refusal, and what runs has the property"""
    for sweep_seed in (7, 11, 2024):
        rng = np.random.default_rng(sweep_seed)
        n_ok = n_refused = 0
        for it in range(60):
            s = cp.sweep_case(rng)
            prof = s["model"].profile()
            try:
                out = _oracle.simulate_pe(oracle, _oracle.HostGenome(s["contigs"]), prof.pod(), s["reads"], s["seed"], first=s["first"],
                                          count=s["count"], read_id_base=3, qual_offset=s["qoff"], threads=cp.THREADS).trimmed()
            except RuntimeError:
                n_refused += 1
                continue
            cp.qualities_allowed(s["model"], out, s["qoff"])
            n_ok += 1
        assert n_ok >= 50 and n_ok + n_refused == 60, (sweep_seed, n_ok, n_refused)


def test_models_of_equal_size_keep_their_own_oracle_entry(oracle):
    """The oracle caches built models by a hash of the file's bytes and its length (oracle/simulate.c: custom_of), eight at
    a time.  Twelve models of one size that differ in a single score — in its low bits, or only in bit 31 or bit 63 of an
    8-byte word, which a word-wise hash must not lose — each give their own score, in turn and again after eviction."""
    contigs = cp.case_genome(52)
    scores = [30, 31, 32, 33, 30 + 2 ** 31, 31 + 2 ** 31, 40, 41, 42, 43, 44, 45]
    models = []
    for k, s in enumerate(scores):
        # (an (lo, hi) pair is one 8-byte word of the file at this offset parity or straddles two: both bins are set)
        q = [([0.0, 1.0], [(7, 7 + 2 ** 31 * (k % 2)), (s, s)])] * 5
        models.append(cp.Model(q, ([1.0], [(20, 20)]), None, 20, 0))
    assert len({len(m.blob) for m in models}) == 1 and len({m.blob for m in models}) == len(models)
    for _ in range(2):
        for m, s in zip(models, scores):
            out = _oracle_run(oracle, m, contigs, 3, reads=40, qoff=0)
            assert (out["qual"] == (s & 0xff)).all() and out["qual"].size == 40 * 20
