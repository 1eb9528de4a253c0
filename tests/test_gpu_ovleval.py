"""simmr_ovleval_* on the GPU against the plain model of tests/_ovleval.py, entry for entry: the counts, by_len, and the columns
key_a / key_b / ov / best / hits of every true pair.  Small texts written out here, the refusals, and a simulated long-read run
whose overlaps are the truth and, perturbed on the host, the candidate."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import MinimalLongErrorProfile, SimmrError, _abi
from simmr_amd.engine import Engine
from tests import _ovleval
from tests._ovleval import rec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    e.stage_synthetic(0, [20_000], 31)
    yield e
    e.close()


def same(ev, model, what):
    """every table and column of the device object equals the model's"""
    counts, by = ev.read()
    want_counts, want_by = model.read()
    assert counts == want_counts, (what, {k: (counts[k], want_counts[k]) for k in counts if counts[k] != want_counts[k]})
    assert by.shape == want_by.shape == (41, 2) and np.array_equal(by, want_by), what
    for got, want, name in zip(ev.pairs(), model.pairs(), ("key_a", "key_b", "ov", "best", "hits")):
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, name)


def against_model(eng, truth_texts, cand_texts, what, pct=10):
    model = _ovleval.evaluate(truth_texts, cand_texts, pct)
    ev = eng.overlap_eval(pct)
    try:
        for t in truth_texts:
            ev.truth_add(t)
        assert ev.truth_plan() == (len(model.order), len(model.reads)), what
        for t in cand_texts:
            ev.add(t)
        same(ev, model, what)
    finally:
        ev.close()
    return model


TRUTH = rec(1, 1000, 100, 300, "+", 2, 900, 0, 200) + rec("3/1", 500, 0, 500, "-", "3/2", 500, 0, 500) + rec(9, 5000, 4000, 5000, "+", 2, 900, 400, 900)


def test_empty_texts(eng):
    m = against_model(eng, [b""], [b""], "empty")
    assert m.read()[0]["truth_entries"] == 0
    against_model(eng, [], [TRUTH], "no truth, every record of an unknown read")
    against_model(eng, [TRUTH], [], "no candidate: every pair missed")
    against_model(eng, [b"\n\n"], [b"\n"], "empty lines alone")


def test_one_record_and_the_open_last_line(eng):
    one = rec(1, 1000, 100, 300, "+", 2, 900, 0, 200)
    m = against_model(eng, [one], [one], "one record")
    assert m.read()[0]["correct"] == 1 and m.read()[1][8, 0] == 1   # ov 200: eight bits
    against_model(eng, [one[:-1]], [one[:-1]], "no newline at the end")
    against_model(eng, [b"\n" + TRUTH.replace(b"\n", b"\n\n")], [b"\n\n" + TRUTH[:-1]], "empty lines between the records")
    against_model(eng, [TRUTH], [TRUTH.replace(b"\t255\n", b"\t255\ttp:A:S\tcm:i:12\n")], "tags behind the twelfth field")


def test_each_outcome(eng):
    cand = (rec(1, 1000, 100, 300, "+", 2, 900, 0, 200)            # correct
            + rec(2, 900, 0, 200, "+", 1, 1000, 100, 300)          # the pair in reversed order: correct, a second hit
            + rec(1, 1000, 100, 300, "-", 2, 900, 0, 200)          # wrong_strand
            + rec(1, 1000, 100, 119, "+", 2, 900, 0, 200)          # wrong_interval: 19 of 200 on the query
            + rec(1, 1000, 100, 120, "+", 2, 900, 0, 200)          # 20 of 200: the criterion met exactly
            + rec(1, 1000, 0, 10, "+", 9, 5000, 0, 10)             # no_pair
            + rec(1, 1000, 0, 10, "+", 1, 1000, 0, 10)             # self
            + rec(7, 1000, 0, 10, "+", 1, 1000, 0, 10)             # unknown_read: no read of the truth
            + rec("r1", 1000, 0, 10, "+", 1, 1000, 0, 10)          # unknown_read: no read name
            + rec("7/1", 10, 0, 10, "+", "7/1", 10, 0, 10)         # unknown before self
            + rec("3/2", 500, 0, 500, "-", "3/1", 500, 0, 500)     # keys that differ in the mate bit alone
            + rec(3, 500, 0, 500, "-", "3/2", 500, 0, 500))        # "3" is "3/1": the key does not keep the suffix
    m = against_model(eng, [TRUTH], [cand], "each outcome")
    c = m.read()[0]
    assert (c["correct"], c["wrong_strand"], c["wrong_interval"], c["no_pair"], c["self"], c["unknown_read"], c["wrong"]) == (5, 1, 1, 1, 1, 3, 6)
    assert (c["pairs_found"], c["pairs_missed"], c["pairs_multiple"], c["truth_reads"]) == (2, 1, 2, 5)
    for pct in (1, 50, 100):
        against_model(eng, [TRUTH], [cand], f"each outcome at {pct} percent", pct)


def test_ids_of_one_and_eighteen_digits(eng):
    big = 10 ** 18 - 1
    truth = rec(0, 10, 0, 10, "+", 1, 10, 0, 10) + rec(f"{big}/2", 2 ** 40 - 1, 0, 2 ** 40 - 1, "-", f"{big}/1", 10, 0, 10) + rec(big - 1, 10, 0, 0, "+", 0, 10, 10, 10)
    m = against_model(eng, [truth], [truth + rec(f"{big}/2", 2 ** 40 - 1, 5, 2 ** 40 - 1, "-", big, 10, 0, 10)], "wide ids")
    assert m.pairs()[1].max() == big << 1 | 1 and m.read()[1][40, 0] == 1 and m.read()[1][0, 1] == 1  # an empty interval is never found


MALFORMED = {
    "eleven fields": b"1\t10\t0\t10\t+\t2\t10\t0\t10\t10\t10\n",
    "a length that is no number": rec(1, "1e3", 0, 10, "+", 2, 10, 0, 10),
    "an empty number": rec(1, 10, "", 10, "+", 2, 10, 0, 10),
    "nineteen digits": rec(1, 10, 0, 10, "+", 2, 10, 0, 10, tail=(0, 0, 10 ** 18)),
    "a strand of two bytes": rec(1, 10, 0, 10, "+-", 2, 10, 0, 10),
    "a strand of *": rec(1, 10, 0, 10, "*", 2, 10, 0, 10),
    "start behind end": rec(1, 10, 6, 5, "+", 2, 10, 0, 10),
    "end behind the length": rec(1, 10, 0, 10, "+", 2, 10, 0, 11),
    "a length of 2^40": rec(1, 2 ** 40, 0, 10, "+", 2, 10, 0, 10),
    "a carriage return": rec(1, 10, 0, 10, "+", 2, 10, 0, 10)[:-1] + b"\r\n",
}
TRUTH_ONLY = {
    "a name that is no read id": rec("read1", 10, 0, 10, "+", 2, 10, 0, 10),
    "a suffix of /3": rec("1/3", 10, 0, 10, "+", 2, 10, 0, 10),
    "one read on both sides": rec("4/1", 10, 0, 10, "+", 4, 10, 0, 10),
}


@pytest.mark.parametrize("what", list(MALFORMED))
def test_malformed_candidate_record(eng, what):
    with pytest.raises(_ovleval.Malformed):
        _ovleval.evaluate([TRUTH], [MALFORMED[what]]).read()
    ev = eng.overlap_eval()
    try:
        ev.truth_add(TRUTH)
        ev.truth_plan()
        ev.add(TRUTH + MALFORMED[what] + TRUTH)
        with pytest.raises(SimmrError) as err:
            ev.read()
        assert err.value.code == _abi.EINVAL and "malformed candidate record" in str(err.value)
        canary = _abi.OvlevalCounts(*([7] * 16))
        by = np.full((41, 2), 7, dtype=np.uint64)
        assert ev.lib.simmr_ovleval_read(ev._h, C.byref(canary), by.ctypes.data_as(C.POINTER(C.c_uint64))) == _abi.EINVAL
        assert canary.lines == 7 and (by == 7).all()   # nothing written
    finally:
        ev.close()


@pytest.mark.parametrize("what", list(MALFORMED) + list(TRUTH_ONLY))
def test_malformed_truth_record(eng, what):
    bad = {**MALFORMED, **TRUTH_ONLY}[what]
    with pytest.raises(_ovleval.Malformed):
        _ovleval.evaluate([TRUTH + bad], [])
    ev = eng.overlap_eval()
    try:
        ev.truth_add(TRUTH)
        ev.truth_add(bad)
        with pytest.raises(SimmrError) as err:
            ev.truth_plan()
        assert err.value.code == _abi.EINVAL and "malformed truth record" in str(err.value)
        with pytest.raises(SimmrError) as err:
            ev.add(TRUTH)
        assert err.value.code == _abi.ESTATE
        with pytest.raises(SimmrError) as err:
            ev.read()
        assert err.value.code == _abi.EINVAL
        ev.reset()
        ev.truth_add(TRUTH)
        assert ev.truth_plan() == (3, 5)
    finally:
        ev.close()


def test_a_pair_given_twice(eng):
    twice = TRUTH + rec(2, 900, 5, 100, "-", 1, 1000, 0, 50)  # the first pair again, the other way round
    with pytest.raises(_ovleval.DuplicatePair):
        _ovleval.evaluate([twice], [])
    ev = eng.overlap_eval()
    try:
        ev.truth_add(twice)
        with pytest.raises(SimmrError) as err:
            ev.truth_plan()
        assert err.value.code == _abi.EINVAL and "one pair" in str(err.value)
        with pytest.raises(SimmrError) as err:
            ev.pairs()
        assert err.value.code == _abi.ESTATE
    finally:
        ev.close()


def test_state_and_capacity_refusals(eng):
    import torch
    lib = eng.lib
    h = C.c_void_p()
    assert lib.simmr_ovleval_create(eng._h, C.byref(h)) == 0
    try:
        text = torch.from_numpy(np.frombuffer(TRUTH, dtype=np.uint8).copy()).to(eng.device)
        p, n = C.c_void_p(text.data_ptr()), text.numel()
        ms = C.c_float()
        assert lib.simmr_ovleval_truth_add(h, p, n) == _abi.ESTATE and lib.simmr_ovleval_truth_plan(h, None, None) == _abi.ESTATE
        assert lib.simmr_ovleval_read(h, None, None) == _abi.ESTATE and lib.simmr_last_ovleval_ms(h, C.byref(ms)) == _abi.ESTATE
        assert lib.simmr_ovleval_reset(h, 101) == _abi.EINVAL and lib.simmr_ovleval_reset(h, 0) == 0
        assert lib.simmr_ovleval_add(h, p, n) == _abi.ESTATE and lib.simmr_ovleval_emit(h, None, None, None, None, None, 0) == _abi.ESTATE
        assert lib.simmr_ovleval_truth_add(h, None, 5) == _abi.EINVAL and lib.simmr_ovleval_truth_add(h, p, 0xf0000001) == _abi.ENOTSUP
        assert lib.simmr_ovleval_truth_add(h, p, n) == 0 and lib.simmr_ovleval_truth_plan(h, None, None) == 0
        assert lib.simmr_ovleval_add(h, None, 5) == _abi.EINVAL and lib.simmr_ovleval_add(h, p, 0xf0000001) == _abi.ENOTSUP
        assert lib.simmr_ovleval_add(h, p, n) == 0
        assert lib.simmr_last_ovleval_ms(h, None) == _abi.EINVAL and lib.simmr_last_ovleval_ms(h, C.byref(ms)) == 0 and ms.value > 0
        cols = torch.full((3,), 7, dtype=torch.int64, device=eng.device)
        q = C.c_void_p(cols.data_ptr())
        assert lib.simmr_ovleval_emit(h, q, None, None, None, None, 2) == _abi.ERANGE and (cols == 7).all()   # one short: nothing written
        assert lib.simmr_ovleval_emit(h, q, None, None, None, None, 3) == 0 and cols.cpu().tolist() == [2, 4, 6]
        assert lib.simmr_ovleval_emit(h, None, None, None, None, None, 3) == 0
        # a truth add drops the plan
        assert lib.simmr_ovleval_truth_add(h, p, 0) == 0 and lib.simmr_ovleval_add(h, p, n) == _abi.ESTATE
    finally:
        lib.simmr_ovleval_destroy(h)


def test_a_plan_starts_the_candidate_side_over(eng):
    ev = eng.overlap_eval()
    try:
        ev.truth_add(TRUTH)
        ev.truth_plan()
        ev.add(TRUTH)
        assert ev.read()[0]["correct"] == 3
        assert ev.truth_plan() == (3, 5)
        c, by = ev.read()
        assert (c["lines"], c["correct"], c["pairs_missed"], c["truth_lines"], c["truth_reads"]) == (0, 0, 3, 3, 5) and by[:, 1].sum() == 3
        ev.add(TRUTH)
        same(ev, _ovleval.evaluate([TRUTH], [TRUTH]), "behind a second plan")
    finally:
        ev.close()


# ---- a simulated long-read run ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_truth(eng):
    lp = MinimalLongErrorProfile(gamma_mean=1500.0, gamma_std=1000.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    dev = eng.simulate_long_reads([0], [300], lp, 9, qual_offset=33)
    eng.overlap_reset(False)
    eng.overlap_add(dev)
    return bytes(eng.overlaps(200, text=True).cpu().numpy())


def test_a_run_against_itself_and_against_a_perturbed_copy(eng, run_truth):
    n = len(_ovleval.lines(run_truth))
    assert 2000 < n < 40_000
    m = against_model(eng, [run_truth], [run_truth], "the run against itself")
    c = m.read()[0]
    assert (c["correct"], c["wrong"], c["pairs_found"], c["pairs_missed"], c["pairs_multiple"]) == (n, 0, n, 0, 0)
    cand = _ovleval.derive(run_truth, outside_id=10 ** 9)
    m = against_model(eng, [run_truth], [cand], "the perturbed copy")
    c = m.read()[0]
    assert min(c["wrong_strand"], c["wrong_interval"], c["unknown_read"], c["pairs_missed"], c["pairs_multiple"], c["pairs_found"]) > n // 40
    assert _ovleval.report(*m.read()).count(b"\nL\t") >= 3


def test_cuts_of_either_text_give_the_same_tables(eng, run_truth):
    text = b"".join(_ovleval.lines(run_truth)[i] + b"\n" for i in range(0, 400, 10))  # forty lines
    cand = _ovleval.derive(text, outside_id=10 ** 9)
    whole = _ovleval.evaluate([text], [cand])
    ends = [i + 1 for i, b in enumerate(text) if b == 10]
    assert len(ends) == 40
    ev = eng.overlap_eval()
    try:
        for cut in ends:
            ev.reset()
            ev.truth_add(text[:cut])
            ev.truth_add(text[cut:])
            ev.truth_plan()
            ev.add(cand)
            same(ev, whole, f"the truth cut at {cut}")
        cand_ends = [i + 1 for i, b in enumerate(cand) if b == 10]
        ev.reset()
        ev.truth_add(text)
        for cut in cand_ends:
            ev.truth_plan()
            ev.add(cand[:cut])
            ev.add(cand[cut:])
            same(ev, whole, f"the candidate cut at {cut}")
        ev.truth_plan()
        for a, b in zip([0] + cand_ends, cand_ends):   # a line an add
            ev.add(cand[a:b])
        same(ev, whole, "a line an add")
    finally:
        ev.close()
