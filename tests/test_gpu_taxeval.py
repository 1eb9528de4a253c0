"""simmr_taxeval_* on the GPU against the plain model of tests/_taxeval.py for exact equality: every count, by_rank,
reads_by_rank, the columns id / genome row / mates / seen / hits of every true read, the clade sums of every node and the
lineage of every node.  The hand-written records of tests/test_taxeval_host.py (every row of the class table, every step, every
malformed form on either side), cuts of both texts into adds, the refusals of the reset, of the plan and of the state order."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import SimmrError, _abi
from simmr_amd.engine import Engine, cut_at_line_ends
from tests import _taxeval
from tests._taxeval import call, tree_of, truth_line
from tests.test_taxeval_host import GENOMES, HEADER, MALFORMED_CALLS, MALFORMED_TRUTH, RULES, TAXONOMY, TREE_REFUSALS, TRUTH

pytestmark = pytest.mark.gpu

CODES = {"EINVAL": _abi.EINVAL, "ENOTSUP": _abi.ENOTSUP, "ERANGE": _abi.ERANGE}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def same(ev, model, what):
    """every table and column of the device object equals the model's"""
    counts, by_rank, reads_by_rank = ev.read()
    want_counts, want_rank, want_reads = model.read()
    assert counts == want_counts, (what, {k: (counts[k], want_counts[k]) for k in counts if counts[k] != want_counts[k]})
    assert by_rank.shape == want_rank.shape == (8, 5) and np.array_equal(by_rank, want_rank), (what, by_rank, want_rank)
    assert reads_by_rank.shape == (8, 5) and np.array_equal(reads_by_rank, want_reads), (what, reads_by_rank, want_reads)
    for got, want, name in zip(ev.reads(), model.reads(), ("id", "genome", "mates", "seen", "hits")):
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, name)
    for _ in range(2):   # taxa() called twice: the roll-up leaves the direct counts alone
        for got, want, name in zip(ev.taxa(), model.taxa(), ("taxid", "true", "called", "both")):
            assert got.dtype == want.dtype and np.array_equal(got, want), (what, name)


def against_model(eng, truth_pieces, call_pieces, what, taxonomy=TAXONOMY, genomes=GENOMES, ev=None):
    model = _taxeval.evaluate(truth_pieces, call_pieces, taxonomy, genomes)
    own = ev is None
    ev = eng.classify_eval_open(taxonomy, genomes) if own else ev
    try:
        for t in truth_pieces:
            ev.truth_add(t)
        assert ev.truth_plan() == len(model.id), what
        for t in call_pieces:
            ev.add(t)
        same(ev, model, what)
    finally:
        if own:
            ev.close()
    return model


EVERY_RULE = b"# a comment line\n" + b"".join(r[1] if r[1].endswith(b"\n") else r[1] + b"\n" for r in RULES)


def test_empty_texts(eng):
    m = against_model(eng, [b""], [b""], "empty")
    assert m.read()[0]["truth_entries"] == 0
    m = against_model(eng, [], [EVERY_RULE], "an empty truth: every read is unknown")
    assert m.read()[0]["unknown_read"] == m.read()[0]["records"] == len(RULES)
    against_model(eng, [TRUTH], [], "an empty candidate: every read missing")
    against_model(eng, [b"\n\n"], [b"\n"], "empty lines alone")
    against_model(eng, [HEADER], [EVERY_RULE], "a header alone", taxonomy=tree_of([]), genomes=[])


def test_every_rule_in_one_text_and_one_by_one(eng):
    m = against_model(eng, [TRUTH], [EVERY_RULE], "every rule")
    c, by_rank, _ = m.read()
    assert min(c["unknown_read"], c["unclassified"], c["unknown_taxon"], c["scored"], c["multiple"], c["header"]) > 0
    assert (by_rank.sum(axis=0) > 0).all()
    for what, cand, _, _, _ in RULES:
        against_model(eng, [TRUTH], [cand], what)


def test_the_open_last_line_and_empty_lines(eng):
    against_model(eng, [TRUTH[:-1]], [EVERY_RULE[:-1]], "no newline at the end")
    against_model(eng, [b"\n" + TRUTH.replace(b"\n", b"\n\n")], [b"\n\n" + EVERY_RULE.replace(b"\n", b"\n\n\n")[:-3]], "empty lines between the records")


def bigger():
    """300 reads of the five genomes, a third of them paired, and calls of every kind for them"""
    names = [g for g, _ in GENOMES]
    truth, calls = HEADER, b""
    pool = [61, 60, 50, 55, 45, 70, 71, 81, 90, 1, 2, 3, 999, 0]
    for i in range(300):
        g = names[i % 5]
        truth += (truth_line(1000 + i, 1, g) + truth_line(1000 + i, 2, g)) if i % 3 == 0 else truth_line(1000 + i, 0, g)
        if i % 11:
            calls += call(f"{1000 + i}/1" if i % 3 == 0 else 1000 + i, pool[(i * 7) % len(pool)], names=("x y" if i % 4 == 0 else None))
        if i % 6 == 0:
            calls += call(f"{1000 + i}/2", pool[(i * 5 + 1) % len(pool)])
    return truth, calls + call(5, 61) + call("abc", 61)


@pytest.mark.parametrize("pieces", [1, 2, 7])
def test_cuts_of_either_text_give_the_same_tables(eng, pieces):
    truth, cand = bigger()
    whole = _taxeval.evaluate([truth], [cand], TAXONOMY, GENOMES)
    t, c = cut_at_line_ends(truth, pieces), cut_at_line_ends(cand, pieces)
    assert len(t) == len(c) == pieces and b"".join(t) == truth and all(p.endswith(b"\n") for p in t + c)
    m = against_model(eng, t, c, f"{pieces} adds a side")
    assert m.read()[0] == whole.read()[0] and np.array_equal(m.reads()[3], whole.reads()[3]) and whole.read()[0]["truth_paired"] == 100
    got = eng.classify_eval(truth, cand, TAXONOMY, GENOMES, pieces=pieces)   # the one-call form
    assert got[0] == whole.read()[0] and np.array_equal(got[1], whole.read()[1]) and np.array_equal(got[2], whole.read()[2])
    assert all(np.array_equal(a, b) for a, b in zip(got[3], whole.reads())) and all(np.array_equal(a, b) for a, b in zip(got[4], whole.taxa()))


def canaries_stay(ev, word):
    """read() answers SIMMR_EINVAL with `word` in its message, and writes nothing"""
    with pytest.raises(SimmrError) as err:
        ev.read()
    assert err.value.code == _abi.EINVAL and word in str(err.value)
    canary = _abi.TaxevalCounts(*([7] * 13))
    by_rank, reads_by_rank = np.full((8, 5), 7, dtype=np.uint64), np.full((8, 5), 7, dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    assert ev.lib.simmr_taxeval_read(ev._h, C.byref(canary), by_rank.ctypes.data_as(p), reads_by_rank.ctypes.data_as(p)) == _abi.EINVAL
    assert all(getattr(canary, n) == 7 for n in _abi.TAXEVAL_COUNTS) and (by_rank == 7).all() and (reads_by_rank == 7).all()


@pytest.mark.parametrize("what", list(MALFORMED_CALLS))
def test_malformed_candidate_record(eng, what):
    ev = eng.classify_eval_open(TAXONOMY, GENOMES)
    try:
        ev.truth_add(TRUTH)
        ev.truth_plan()
        ev.add(EVERY_RULE + MALFORMED_CALLS[what] + EVERY_RULE)
        canaries_stay(ev, "malformed candidate record")
    finally:
        ev.close()


@pytest.mark.parametrize("what", list(MALFORMED_TRUTH))
def test_malformed_truth_record(eng, what):
    ev = eng.classify_eval_open(TAXONOMY, GENOMES)
    try:
        ev.truth_add(TRUTH + MALFORMED_TRUTH[what] + truth_line(77, 0, "gArch"))
        with pytest.raises(SimmrError) as err:
            ev.truth_plan()
        assert err.value.code == _abi.EINVAL and "malformed truth record" in str(err.value)
        canaries_stay(ev, "malformed truth record")
        with pytest.raises(SimmrError) as err:
            ev.add(EVERY_RULE)
        assert err.value.code == _abi.ESTATE
        ev.reset(TAXONOMY, GENOMES)   # the flag goes with the reset
        against_model(eng, [TRUTH], [EVERY_RULE], "after the reset", ev=ev)
    finally:
        ev.close()


def test_refusals_of_the_plan(eng):
    for text, word in ((truth_line(1, 0, "gStrain") + truth_line(2, 0, "gArch") + truth_line(1, 0, "gArch"), "different genomes"),
                       (truth_line(4, 1, "gArch") + truth_line(3, 1, "gArch") * 3, "more than two")):
        ev = eng.classify_eval_open(TAXONOMY, GENOMES)
        try:
            ev.truth_add(TRUTH.replace(b"\n1\t", b"\n11\t") + text)
            with pytest.raises(SimmrError) as err:
                ev.truth_plan()
            assert err.value.code == _abi.EINVAL and word in str(err.value)
            with pytest.raises(SimmrError) as err:
                ev.reads()
            assert err.value.code == _abi.ESTATE
        finally:
            ev.close()


@pytest.mark.parametrize("what", list(TREE_REFUSALS))
def test_refusals_of_the_reset(eng, what):
    rows, genomes, code = TREE_REFUSALS[what]
    with pytest.raises(SimmrError) as err:
        eng.classify_eval_open(tree_of(rows), genomes)
    assert err.value.code == CODES[code], str(err.value)


def test_the_state_order_and_short_capacities(eng):
    lib, h = eng.lib, C.c_void_p()
    assert lib.simmr_taxeval_create(eng._h, C.byref(h)) == 0
    try:
        n, ms = C.c_uint64(), C.c_float()
        for rc in (lib.simmr_taxeval_truth_add(h, None, 0), lib.simmr_taxeval_truth_plan(h, C.byref(n)), lib.simmr_taxeval_add(h, None, 0),
                   lib.simmr_taxeval_read(h, None, None, None), lib.simmr_taxeval_emit(h, None, None, None, None, None, 0),
                   lib.simmr_taxeval_taxa(h, None, None, None, None, 0), lib.simmr_taxeval_lineage(h, 1, None, None), lib.simmr_last_taxeval_ms(h, C.byref(ms))):
            assert rc == _abi.ESTATE   # before the reset
        cfg = _abi.TaxevalConfig(n_nodes=(1 << 26) + 1, n_genomes=0)
        assert lib.simmr_taxeval_reset(h, C.byref(cfg)) == _abi.EINVAL   # NULL arrays
        one = (C.c_uint32 * 1)(1)
        rank = (C.c_uint8 * 1)(0)
        cfg = _abi.TaxevalConfig((1 << 26) + 1, one, one, rank, 0, None, None)
        assert lib.simmr_taxeval_reset(h, C.byref(cfg)) == _abi.ERANGE   # (refused before an array is read)
        cfg = _abi.TaxevalConfig(1, one, one, rank, (1 << 24) + 1, (C.c_char_p * 1)(b"g"), one)
        assert lib.simmr_taxeval_reset(h, C.byref(cfg)) == _abi.ERANGE
        assert lib.simmr_taxeval_truth_add(h, None, 0) == _abi.ESTATE      # a refused reset leaves no tree
    finally:
        lib.simmr_taxeval_destroy(h)
    ev = eng.classify_eval_open(TAXONOMY, GENOMES)
    try:
        with pytest.raises(SimmrError) as err:
            ev.add(EVERY_RULE)   # before the plan
        assert err.value.code == _abi.ESTATE
        ev.truth_add(TRUTH)
        assert ev.truth_plan() == 6
        ev.add(EVERY_RULE)
        assert lib.simmr_taxeval_emit(ev._h, None, None, None, None, None, 5) == _abi.ERANGE
        assert lib.simmr_taxeval_taxa(ev._h, None, None, None, None, len(TAXONOMY[0]) - 1) == _abi.ERANGE
        assert lib.simmr_taxeval_emit(ev._h, None, None, None, None, None, 6) == 0 and lib.simmr_taxeval_taxa(ev._h, None, None, None, None, 1 << 40) == 0
        assert lib.simmr_taxeval_truth_add(ev._h, None, 5) == _abi.EINVAL and lib.simmr_taxeval_add(ev._h, None, (1 << 32)) in (_abi.EINVAL, _abi.ENOTSUP)
        same(ev, _taxeval.evaluate([TRUTH], [EVERY_RULE], TAXONOMY, GENOMES), "after the refused calls")
        assert ev.last_ms() > 0
        ev.truth_add(truth_line(99, 0, "gArch"))   # a truth add drops the plan
        with pytest.raises(SimmrError) as err:
            ev.add(EVERY_RULE)
        assert err.value.code == _abi.ESTATE
        assert ev.truth_plan() == 7
        ev.add(EVERY_RULE)
        same(ev, _taxeval.evaluate([TRUTH, truth_line(99, 0, "gArch")], [EVERY_RULE], TAXONOMY, GENOMES), "the second plan starts the candidate side over")
    finally:
        ev.close()


def test_the_lineage_of_every_node(eng):
    ev = eng.classify_eval_open(TAXONOMY, GENOMES)
    try:
        T = _taxeval.Tree(TAXONOMY, GENOMES)
        for taxid in T.taxid:
            assert ev.lineage(taxid) == T.lineage(taxid), taxid
        for none in (0, 4, 63, 2 ** 32 - 1):
            with pytest.raises(SimmrError) as err:
                ev.lineage(none)
            assert err.value.code == _abi.EINVAL
    finally:
        ev.close()


def test_a_second_reset_with_another_tree(eng):
    ev = eng.classify_eval_open(TAXONOMY, GENOMES)
    try:
        against_model(eng, [TRUTH], [EVERY_RULE], "the first tree", ev=ev)
        other = tree_of([(7, 0, "domain"), (9, 7, "species"), (8, 7, "genus"), (100, 8, "species"), (5, 5, "domain"), (6, 5, "species")])   # two roots
        genomes = [("b", 100), ("a", 9), ("c", 6)]
        ev.reset(other, genomes)
        truth = truth_line(3, 0, "a") + truth_line(1, 0, "b") + truth_line(2, 0, "c")
        calls = call(1, 100) + call(1, 9) + call(2, 100) + call(3, 8) + call(3, 61) + call(2, 5) + call(4, 7)
        m = against_model(eng, [truth], [calls], "the second tree", taxonomy=other, genomes=genomes, ev=ev)
        assert m.read()[0]["unknown_taxon"] == 1 and m.taxa()[3].sum() > 0 and m.tree.lca(m.tree.row[6], m.tree.row[100]) == _taxeval.NONE
        T = _taxeval.Tree(other, genomes)
        assert [ev.lineage(t) for t in T.taxid] == [T.lineage(t) for t in T.taxid]
        with pytest.raises(SimmrError):
            ev.reset(tree_of([(1, 2, 0), (2, 1, 0)]), [])   # a refused reset ...
        with pytest.raises(SimmrError) as err:
            ev.truth_plan()                                  # ... leaves no tree
        assert err.value.code == _abi.ESTATE
        ev.reset(TAXONOMY, GENOMES)
        against_model(eng, [TRUTH], [EVERY_RULE], "the first tree again", ev=ev)
    finally:
        ev.close()
