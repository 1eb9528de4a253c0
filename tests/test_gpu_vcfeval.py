"""simmr_vcfeval_* on the GPU against the plain model of tests/_vcfeval.py for exact equality: every count, by_qual, by_ad and
the columns key / alleles / ad / best / hits of every true site.  The hand-written records of tests/test_vcfeval_host.py (every
rule, every QUAL and GT form, every malformed form on either side), cuts of both texts into adds, the refusals."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import SimmrError, _abi
from simmr_amd.engine import Engine, cut_at_line_ends
from tests import _vcfeval
from tests._vcfeval import rec, site
from tests.test_vcfeval_host import CANDIDATE_ONLY, GT_FORMS, MALFORMED, NAMES, QUAL_ROWS, RULES, TRUTH, TRUTH_ONLY

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def same(ev, model, what):
    """every table and column of the device object equals the model's"""
    counts, by_qual, by_ad = ev.read()
    want_counts, want_qual, want_ad = model.read()
    assert counts == want_counts, (what, {k: (counts[k], want_counts[k]) for k in counts if counts[k] != want_counts[k]})
    assert by_qual.shape == want_qual.shape == (256, 2) and np.array_equal(by_qual, want_qual), what
    assert by_ad.shape == want_ad.shape == (33, 2) and np.array_equal(by_ad, want_ad), what
    for got, want, name in zip(ev.sites(), model.sites(), ("key", "alleles", "ad", "best", "hits")):
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, name)


def against_model(eng, truth_pieces, call_pieces, what, names=NAMES, use_filtered=False):
    model = _vcfeval.evaluate(truth_pieces, call_pieces, names, use_filtered)
    ev = eng.vcf_eval_open(names, use_filtered)
    try:
        for t in truth_pieces:
            ev.truth_add(t)
        assert ev.truth_plan() == len(model.order), what
        for t in call_pieces:
            ev.add(t)
        same(ev, model, what)
    finally:
        ev.close()
    return model


EVERY_RULE = (b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\n"
              + b"".join(r[1] for r in RULES) + b"".join(rec("chr1", 100, "A", "T", qual=q) for q, _ in QUAL_ROWS)
              + b"".join(rec("chr1", 100, "A", "T,C", qual=40) if g is None else rec("chr1", 100, "A", "T,C", qual=40, fmt="GT:DP", sample=g + ":12\t0/0:3") for g, _ in GT_FORMS)
              + rec("chr1", 100, "A", "T,C", fmt="DP:GT", sample="12:0/0") + rec("chr1", 100, "A", "T,C", fmt="GT") + rec("chr1", 102, "G", "C", qual=77, filt="q10;dp"))


def test_empty_texts(eng):
    m = against_model(eng, [b""], [b""], "empty")
    assert m.read()[0]["truth_entries"] == 0
    against_model(eng, [], [EVERY_RULE], "an empty truth: every call on a known contig finds no site")
    against_model(eng, [TRUTH], [], "an empty candidate: every site missed")
    against_model(eng, [b"\n\n"], [b"\n"], "empty lines alone")
    m = against_model(eng, [b"#only a header\n"], [EVERY_RULE], "no names", names=[])
    assert m.read()[0]["unknown_contig"] == m.read()[0]["calls"] > 0


def test_every_rule_in_one_text_and_one_by_one(eng):
    for use_filtered in (False, True):
        m = against_model(eng, [TRUTH], [EVERY_RULE], f"every rule, use_filtered {use_filtered}", use_filtered=use_filtered)
        c = m.read()[0]
        assert min(c["symbolic"], c["indel"], c["long_allele"], c["ref_call_allele"], c["ref_call"], c["qual_missing"], c["unknown_contig"], c["no_site"],
                   c["ref_mismatch"], c["wrong_allele"], c["correct"], c["sites_multiple"]) > 0 and (c["filtered"] > 0) != use_filtered
    for what, cand, _ in RULES:
        against_model(eng, [TRUTH], [cand], what)
    for gt, _ in GT_FORMS:
        cand = rec("chr1", 100, "A", "T,C", qual=40) if gt is None else rec("chr1", 100, "A", "T,C", qual=40, fmt="GT:DP", sample=gt + ":12")
        against_model(eng, [TRUTH], [cand], f"GT {gt}")


@pytest.mark.parametrize("text,row", QUAL_ROWS)
def test_each_qual_form(eng, text, row):
    m = against_model(eng, [TRUTH], [rec("chr1", 100, "A", "T", qual=text)], f"QUAL {text}")
    assert m.read()[1][row, 0] == 1


def test_the_open_last_line_and_empty_lines(eng):
    against_model(eng, [TRUTH[:-1]], [EVERY_RULE[:-1]], "no newline at the end")
    against_model(eng, [b"\n" + TRUTH.replace(b"\n", b"\n\n")], [b"\n\n" + EVERY_RULE.replace(b"\n", b"\n\n\n")[:-3]], "empty lines between the records")


@pytest.mark.parametrize("pieces", [1, 2, 7])
def test_cuts_of_either_text_give_the_same_tables(eng, pieces):
    truth = TRUTH + b"".join(site("chr2", 50 + 2 * i, "ACGT"[i % 4], "CGTA"[i % 4], 3, 1 << (i % 20)) for i in range(40))
    cand = EVERY_RULE + _vcfeval.derive(truth, b"chrX")
    whole = _vcfeval.evaluate([truth], [cand], NAMES)
    t, c = cut_at_line_ends(truth, pieces), cut_at_line_ends(cand, pieces)
    assert len(t) == len(c) == pieces and b"".join(t) == truth and all(p.endswith(b"\n") for p in t + c)
    m = against_model(eng, t, c, f"{pieces} adds a side")
    assert m.read()[0] == whole.read()[0] and np.array_equal(m.sites()[3], whole.sites()[3])
    got = eng.vcf_eval(truth, cand, NAMES, pieces=pieces)   # the one-call form
    assert got[0] == whole.read()[0] and np.array_equal(got[1], whole.read()[1]) and np.array_equal(got[2], whole.read()[2])
    assert all(np.array_equal(a, b) for a, b in zip(got[3], whole.sites()))


@pytest.mark.parametrize("what", list(MALFORMED) + list(CANDIDATE_ONLY))
def test_malformed_candidate_record(eng, what):
    bad = {**MALFORMED, **CANDIDATE_ONLY}[what]
    with pytest.raises(_vcfeval.Malformed):
        _vcfeval.evaluate([TRUTH], [bad], NAMES).read()
    ev = eng.vcf_eval_open(NAMES)
    try:
        ev.truth_add(TRUTH)
        ev.truth_plan()
        ev.add(EVERY_RULE + bad + EVERY_RULE)
        with pytest.raises(SimmrError) as err:
            ev.read()
        assert err.value.code == _abi.EINVAL and "malformed candidate record" in str(err.value)
        canary = _abi.VcfevalCounts(*([7] * 24))
        by_qual, by_ad = np.full((256, 2), 7, dtype=np.uint64), np.full((33, 2), 7, dtype=np.uint64)
        p = C.POINTER(C.c_uint64)
        assert ev.lib.simmr_vcfeval_read(ev._h, C.byref(canary), by_qual.ctypes.data_as(p), by_ad.ctypes.data_as(p)) == _abi.EINVAL
        assert canary.lines == 7 and (by_qual == 7).all() and (by_ad == 7).all()   # nothing written
        assert ev.truth_plan() == 4   # sticky: a plan does not clear it
        with pytest.raises(SimmrError):
            ev.read()
    finally:
        ev.close()
    if what in CANDIDATE_ONLY:   # not read behind a filter
        against_model(eng, [TRUTH], [bad.replace(b"\t.\t.\t.\t", b"\t.\tlow\t.\t")], what + ", filtered")


@pytest.mark.parametrize("what", list(MALFORMED) + list(TRUTH_ONLY))
def test_malformed_truth_record(eng, what):
    bad = {**MALFORMED, **TRUTH_ONLY}[what]
    with pytest.raises(_vcfeval.Malformed):
        _vcfeval.evaluate([TRUTH + bad], [], NAMES)
    ev = eng.vcf_eval_open(NAMES)
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
        ev.reset(NAMES)
        ev.truth_add(TRUTH)
        assert ev.truth_plan() == 4
    finally:
        ev.close()
    if what in TRUTH_ONLY:   # ... and a candidate may hold it
        against_model(eng, [TRUTH], [bad], what + ", as a candidate")


def test_ad_items_and_the_sample_columns_of_a_truth(eng):
    truth = (TRUTH + rec("chr1", 2 ** 40, "A", "T", info="XAD=1;AD=4,4294967295;AD=x") + rec("chr2", 9, "g", "c", info="AD=0000000001,0000000002")
             + rec("chr2", 10, "G", "C", qual="1e-3", filt="low", info="DP=5;MAD=3,4", fmt="GT", sample="7/x"))
    m = against_model(eng, [truth], [truth], "AD items")
    assert m.sites()[2].tolist() == [7, 1, 300, 2 ** 32 - 1, 0, 2, 0] and m.read()[2][32].tolist() == [1, 0]


def test_a_duplicate_truth_key(eng):
    twice = TRUTH + rec("chr1", 102, "G", "C")
    with pytest.raises(_vcfeval.DuplicateKey):
        _vcfeval.evaluate([twice], [], NAMES)
    ev = eng.vcf_eval_open(NAMES)
    try:
        ev.truth_add(twice)
        with pytest.raises(SimmrError) as err:
            ev.truth_plan()
        assert err.value.code == _abi.EINVAL and "one position" in str(err.value)
        with pytest.raises(SimmrError) as err:
            ev.sites()
        assert err.value.code == _abi.ESTATE
    finally:
        ev.close()


def test_state_and_capacity_refusals(eng):
    import torch
    lib = eng.lib
    h = C.c_void_p()
    assert lib.simmr_vcfeval_create(eng._h, C.byref(h)) == 0
    try:
        text = torch.from_numpy(np.frombuffer(TRUTH, dtype=np.uint8).copy()).to(eng.device)
        p, n = C.c_void_p(text.data_ptr()), text.numel()
        ms = C.c_float()
        raw = [b"chr1", b"chr2"]
        cfg = _abi.VcfevalConfig(2, 0, (C.c_char_p * 2)(*raw))
        assert lib.simmr_vcfeval_truth_add(h, p, n) == _abi.ESTATE and lib.simmr_vcfeval_truth_plan(h, None) == _abi.ESTATE
        assert lib.simmr_vcfeval_read(h, None, None, None) == _abi.ESTATE and lib.simmr_last_vcfeval_ms(h, C.byref(ms)) == _abi.ESTATE
        assert lib.simmr_vcfeval_reset(h, None) == _abi.EINVAL
        assert lib.simmr_vcfeval_reset(h, C.byref(_abi.VcfevalConfig(2, 0, (C.c_char_p * 2)(b"a", b"a")))) == _abi.EINVAL      # a name twice
        assert lib.simmr_vcfeval_reset(h, C.byref(_abi.VcfevalConfig(1, 0, (C.c_char_p * 1)(b"a b")))) == _abi.ENOTSUP        # no reference name
        assert lib.simmr_vcfeval_reset(h, C.byref(_abi.VcfevalConfig(1, 0, (C.c_char_p * 1)(b"x" * 255)))) == _abi.ENOTSUP
        assert lib.simmr_vcfeval_reset(h, C.byref(_abi.VcfevalConfig((1 << 24) + 1, 0, (C.c_char_p * 1)(b"x")))) == _abi.ERANGE
        assert lib.simmr_vcfeval_truth_add(h, p, n) == _abi.ESTATE   # a refused reset is no reset
        assert lib.simmr_vcfeval_reset(h, C.byref(cfg)) == 0
        assert lib.simmr_vcfeval_add(h, p, n) == _abi.ESTATE and lib.simmr_vcfeval_emit(h, None, None, None, None, None, 0) == _abi.ESTATE
        assert lib.simmr_vcfeval_truth_add(h, None, 5) == _abi.EINVAL and lib.simmr_vcfeval_truth_add(h, p, 0xf0000001) == _abi.ENOTSUP
        assert lib.simmr_vcfeval_truth_add(h, p, n) == 0 and lib.simmr_vcfeval_truth_plan(h, None) == 0
        assert lib.simmr_vcfeval_add(h, None, 5) == _abi.EINVAL and lib.simmr_vcfeval_add(h, p, 0xf0000001) == _abi.ENOTSUP
        assert lib.simmr_vcfeval_add(h, p, n) == 0
        assert lib.simmr_last_vcfeval_ms(h, None) == _abi.EINVAL and lib.simmr_last_vcfeval_ms(h, C.byref(ms)) == 0 and ms.value > 0
        cols = torch.full((4,), 7, dtype=torch.int64, device=eng.device)
        q = C.c_void_p(cols.data_ptr())
        assert lib.simmr_vcfeval_emit(h, q, None, None, None, None, 3) == _abi.ERANGE and (cols == 7).all()   # one short: nothing written
        assert lib.simmr_vcfeval_emit(h, q, None, None, None, None, 4) == 0 and cols.cpu().tolist() == [99, 101, 199, 1 << 40 | 4]
        assert lib.simmr_vcfeval_emit(h, None, None, None, None, None, 4) == 0
        # a truth add drops the plan; a reset empties both sides
        assert lib.simmr_vcfeval_truth_add(h, p, 0) == 0 and lib.simmr_vcfeval_add(h, p, n) == _abi.ESTATE
        assert lib.simmr_vcfeval_reset(h, C.byref(cfg)) == 0
        c, left = _abi.VcfevalCounts(), C.c_uint64(9)
        assert lib.simmr_vcfeval_read(h, C.byref(c), None, None) == 0 and (c.truth_lines, c.truth_entries, c.lines, c.calls) == (0, 0, 0, 0)
        assert lib.simmr_vcfeval_truth_plan(h, C.byref(left)) == 0 and left.value == 0
    finally:
        lib.simmr_vcfeval_destroy(h)


def test_a_plan_starts_the_candidate_side_over(eng):
    ev = eng.vcf_eval_open(NAMES)
    try:
        ev.truth_add(TRUTH)
        ev.truth_plan()
        ev.add(TRUTH)
        assert ev.read()[0]["correct"] == 4
        assert ev.truth_plan() == 4
        c, by_qual, by_ad = ev.read()
        assert (c["lines"], c["correct"], c["sites_missed"], c["truth_lines"], c["truth_entries"]) == (0, 0, 4, 7, 4) and by_ad[:, 1].sum() == 4 and by_qual.sum() == 0
        ev.add(EVERY_RULE)
        same(ev, _vcfeval.evaluate([TRUTH], [EVERY_RULE], NAMES), "behind a second plan")
    finally:
        ev.close()
