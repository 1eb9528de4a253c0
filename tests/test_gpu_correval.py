"""simmr_correval_* on the GPU against the plain model of tests/_correval.py for exact equality: every count, the cube, by_qual, by_pos
and every column of the entries; the invariants beside the model; the refusals.  The cases are built by hand and from a seeded generator."""
import random

import numpy as np
import pytest

from simmr_amd import SimmrError, _abi
from simmr_amd.engine import Engine
from tests import _correval as M
from tests._correval import cut_at, emitted, fastq_record, make_read, sam_record, true_read

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -22, -1
BASE_SUMS = ("kept", "damaged", "fixed", "left", "miscorrected", "ambiguous", "trimmed_error", "trimmed_clean", "extra")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def device(eng, truth_adds, read_adds, lpr=4):
    counts, cube, by_qual, by_pos, cols = eng.correction_eval(list(truth_adds), list(read_adds), lpr)
    return counts, cube, by_qual, by_pos, cols


def same(got, want, what):
    counts, cube, by_qual, by_pos, cols = got
    w_counts, w_cube, w_qual, w_pos, rows = want
    assert tuple(counts) == _abi.CORREVAL_COUNTS == M.COUNTS
    assert counts == w_counts, (what, {k: (counts[k], w_counts[k]) for k in counts if counts[k] != w_counts[k]})
    for name, g, w in (("cube", cube, w_cube), ("by_qual", by_qual, w_qual), ("by_pos", by_pos, w_pos)):
        w = np.array(w, dtype=np.uint64)
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:8], g[g != w][:8], w[g != w][:8])
    for j, name in enumerate(("key", "length", "before", "residual", "hits")):
        w = np.array([r[j] for r in rows], dtype=np.uint64 if j == 0 else np.uint32)
        assert cols[j].dtype == w.dtype and np.array_equal(cols[j], w), (what, name, cols[j][:8], w[:8])


def invariants(got, what):
    counts, cube, by_qual, by_pos, cols = got
    assert int(cube.sum()) == counts["compared"], what
    five = [counts[v] for v in M.VERDICTS]
    assert [int(x) for x in by_qual.sum(axis=0)] == five and [int(x) for x in by_pos.sum(axis=0)] == five, what
    assert counts["records"] == counts["unknown_read"] + counts["scored"], what
    assert counts["truth_lines"] == counts["truth_header"] + counts["truth_records"], what
    assert counts["missing"] + sum(counts[k] for k in ("clean_kept", "clean_damaged", "fixed_all", "improved", "unchanged", "worse")) == counts["truth_entries"], what


def against_model(eng, truth_adds, read_adds, what, lpr=4):
    want = M.score(truth_adds, read_adds, lpr)
    got = device(eng, truth_adds, read_adds, lpr)
    same(got, want, what)
    invariants(got, what)
    return got


# ---- the hand-built case ----------------------------------------------------------------------------------------------------------------
def hand_reads():
    rng = random.Random(20261021)
    R = []
    rid = 3
    for L in (1, 15, 16, 17, 31, 32, 33, 600):
        for rev in (False, True):
            for mate in (None, 0, 1):
                n_err = min(L, rng.choice((0, 1, 2, 5)))
                R.append(make_read(rng, rid, L, mate, rev, sorted(rng.sample(range(L), n_err))))
                rid += 1 if mate in (None, 1) else 0
    # qualities '!' and '~', and a truth QUAL of '*'
    R.append(make_read(rng, 1000, 20, None, False, (3, 4), qual="!" * 10 + "~" * 10))
    R.append(make_read(rng, 1001, 20, None, True, (0, 19), qual="*"))          # the first and the last base of a reverse read
    R.append(make_read(rng, 1002, 2, None, False, (0, 1)))                     # MD 0A0C0
    R.append(make_read(rng, 1003, 137, 1, False, (1, 3, 5, 7, 9, 11, 13)))     # "1X" seven times, then 123: its digits straddle byte 16 of MD
    R.append(make_read(rng, 1004, 300, 0, True, tuple(range(0, 300, 7))))      # an MD of more than 16 bytes, many rounds
    R.append(make_read(rng, 1005, 24, None, False, (5,), ref="ACGTNACGTACGTACGTACGTNNA"))   # N in o and t alike (a match), and an error
    r = make_read(rng, 1006, 12, None, True, ())
    r["ref"] = r["ref"][:4] + "N" + r["ref"][5:]                               # N in t only: MD letter N
    R.append(r)
    r = make_read(rng, 1007, 12, None, False, ())
    r["seq"] = r["seq"][:6] + "N" + r["seq"][7:]                               # N in o only
    R.append(r)
    R.append(make_read(rng, 10**18 - 1, 40, 1, True, (0, 39)))                 # the largest id: 18 digits, a key of 61 bits
    R.append(make_read(rng, 1008, 30, None, False, (2,)))                      # never in the corrected reads: missing
    return R


def corrupt(rng, r, p_fix=0.6, p_damage=0.03):
    """a corrector's output for read r, in the read's orientation: fixes some errors, damages some clean bases, lower-cases its changes"""
    e, t = list(emitted(r)), true_read(r)
    for i in range(len(e)):
        if e[i] != t[i] and t[i] in "ACGT" and rng.random() < p_fix:
            e[i] = t[i].lower()
        elif rng.random() < p_damage:
            e[i] = rng.choice("acgtn")
    return "".join(e)


def hand_case():
    rng = random.Random(7)
    R = hand_reads()
    truth = "@HD\tVN:1.6\n@SQ\tSN:c1\tLN:100000\n" + "".join(sam_record(r) for r in R[:20]) + "\n\n" + "".join(sam_record(r) for r in R[20:])
    truth += "77\t256\tc1\t5\t0\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:4\n"       # secondary: skipped
    truth += "78\t0\tc1\t5\t0\t2M1I1M\t*\t0\t0\tACGT\tIIII\tMD:Z:3\n"     # not one run: skipped
    truth += "79\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"                           # unmapped, SEQ *: skipped (its POS of 0 and missing MD are never looked at)
    truth += "80\t0\tc1\t5\t0\t4X\t*\t0\t0\tACGT\tIIII\tMD:Z:4"           # 4X is not <L>M: skipped; the last line lacks its '\n'
    by = {M.name_key(M.read_name(r)): r for r in R}
    recs = []
    for r in R[:-1]:
        recs.append(fastq_record(r, corrupt(rng, r)))
    r = by[M.name_key("1000")]
    recs.append(fastq_record(r, true_read(r)))                               # a record given twice: this one has residual 0
    recs.append(fastq_record(R[5], ""))                                      # trimmed to 0 bases: an empty line
    recs.append(fastq_record(R[7], emitted(R[7])[:-1]))                      # trimmed by one base
    recs.append(fastq_record(R[9], emitted(R[9]) + "A"))                     # longer by one
    recs.append(fastq_record(R[11], emitted(R[11])[:7].lower() + "N" + emitted(R[11])[8:]))   # lower case, and N in c
    recs.append(fastq_record(R[0], name="999999"))                           # an unknown id
    recs.append(fastq_record(R[0], name="read_17"))                          # a non-numeric name
    recs.append(fastq_record(R[0], name=str(2**61)))                         # 2^61 has 19 digits: no read name
    recs.append(fastq_record(R[13], true_read(R[13]), name=M.read_name(R[13]) + " length=%d\tx" % len(R[13]["seq"])))   # a name, a space, a comment
    recs.append(fastq_record(R[4], name=M.read_name(R[4]) + "\tcomment"))
    rng.shuffle(recs)
    reads = "".join(recs)
    return R, truth.encode(), reads[:-1].encode(), recs   # the last line lacks its '\n'


def record_ends(text: bytes, lpr):
    ends, n = [], 0
    for i, b in enumerate(text):
        if b == 10:
            n += 1
            if n % lpr == 0:
                ends.append(i + 1)
    return ends


def line_ends(text: bytes):
    return [i + 1 for i, b in enumerate(text) if b == 10]


def test_the_hand_built_case(eng):
    R, truth, reads, recs = hand_case()
    got = against_model(eng, [truth], [reads], "one add each")
    counts = got[0]
    assert counts["truth_skipped"] == 4 and counts["truth_header"] == 2 and counts["truth_entries"] == len(R)
    assert counts["missing"] >= 1 and counts["multiple"] >= 1 and counts["unknown_read"] == 3
    assert counts["trimmed_records"] == 2 and counts["longer_records"] == 1 and counts["extra"] == 1 and counts["ambiguous"] > 0
    assert got[3][511].sum() > 0   # the 600-base reads reach the last row of by_pos
    # any cut of either text, and any order of the records
    want = M.score([truth], [reads])
    for pieces in (2, 3, 7):
        t_adds, r_adds = cut_at(truth, line_ends(truth), pieces), cut_at(reads, record_ends(reads, 4), pieces)
        assert b"".join(t_adds) == truth and b"".join(r_adds) == reads and len(r_adds) > 1
        same(device(eng, t_adds, r_adds), want, "%d pieces" % pieces)
    rng = random.Random(11)
    for _ in range(2):
        order = recs[:]
        rng.shuffle(order)
        t_lines = truth.decode().split("\n")
        rng.shuffle(t_lines)
        shuffled = device(eng, ["\n".join(t_lines).encode()], ["".join(order).encode()])
        w = dict(want[0])
        assert shuffled[0] == w
        same(shuffled, want, "shuffled")


def test_uncorrected_and_true_reads(eng):
    rng = random.Random(5)
    R = []
    for i in range(60):
        L = rng.choice((1, 16, 33, 100, 151))
        R.append(make_read(rng, i, L, rng.choice((None, 0, 1)), bool(i & 1), sorted(rng.sample(range(L), min(L, rng.randrange(4))))))
    truth = "".join(sam_record(r) for r in R).encode()
    nm = sum(sum(a != b for a, b in zip(r["ref"], r["seq"])) for r in R)
    total = sum(len(r["seq"]) for r in R)
    got = against_model(eng, [truth], ["".join(fastq_record(r) for r in R).encode()], "the uncorrected reads")
    c = got[0]
    assert c["fixed"] == c["damaged"] == c["miscorrected"] == 0 and c["left"] == nm and c["kept"] == total - nm
    assert c["unchanged"] + c["clean_kept"] == len(R) and np.array_equal(got[4][2], got[4][3])   # residual == before
    assert sum(c[k] for k in BASE_SUMS) == total
    got = against_model(eng, [truth], ["".join(fastq_record(r, true_read(r)) for r in R).encode()], "the true reads")
    c = got[0]
    assert not got[4][3].any() and c["left"] == c["damaged"] == 0 and c["fixed"] == nm and c["fixed_all"] + c["clean_kept"] == len(R)


def test_per_record_sums(eng):
    """a record alone: the nine base sums add up to L + extra"""
    R, truth, _, _ = hand_case()
    rng = random.Random(3)
    for r in (R[2], R[45], R[47]):
        for bases in (corrupt(rng, r, 0.5, 0.2), corrupt(rng, r)[:len(r["seq"]) // 2], corrupt(rng, r) + "ACG"):
            got = against_model(eng, [truth], [fastq_record(r, bases).encode()], "one record")
            c = got[0]
            assert sum(c[k] for k in BASE_SUMS) == len(r["seq"]) + c["extra"] and c["extra"] == max(len(bases) - len(r["seq"]), 0)


def test_two_line_fasta(eng):
    R, truth, _, _ = hand_case()
    rng = random.Random(9)
    reads = "".join(fastq_record(r, corrupt(rng, r), lines_per_record=2) for r in R[:30]) + ">5\n\n" + ">nobody\nACGT"
    got = against_model(eng, [truth], [reads.encode()], "two-line FASTA", lpr=2)
    assert got[0]["records"] == 32 and got[0]["lines"] == 64


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
GOOD = "5\t0\tc1\t9\t60\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:1C2\n"
BAD_READS = {
    "three lines": "@5\nACGT\n+\n",
    "a missing +": "@5\nACGT\n-\nIIII\n",
    "a QUAL line of another length": "@5\nACGT\n+\nIII\n",
    "a first line without @": ">5\nACGT\n+\nIIII\n",
}
BAD_TRUTH = {
    "no MD": "5\t0\tc1\t9\t60\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:0\n",
    "an MD that does not add up": "5\t0\tc1\t9\t60\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:1C1\n",
    "an MD with a deletion": "5\t0\tc1\t9\t60\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:2^A2\n",
    "an MD with a lower-case letter": "5\t0\tc1\t9\t60\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:1c2\n",
    "an MD number of ten digits": "5\t0\tc1\t9\t60\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:0000000004\n",
    "a QUAL of another length": "5\t0\tc1\t9\t60\t4M\t*\t0\t0\tACGT\tIII\tMD:Z:4\n",
    "a QUAL byte outside": "5\t0\tc1\t9\t60\t4M\t*\t0\t0\tACGT\tII I\tMD:Z:4\n",
    "a QNAME that is no id": "r5\t0\tc1\t9\t60\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:4\n",
    "a POS of 0": "5\t0\tc1\t0\t60\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:4\n",
    "an id of 2^61 (19 digits)": "%d\t0\tc1\t9\t60\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:4\n" % 2**61,
    "ten fields": "5\t0\tc1\t9\t60\t4M\t*\t0\t0\tACGT\n",
    "one key twice": GOOD + GOOD,
}


@pytest.mark.parametrize("what", list(BAD_READS))
def test_malformed_reads_are_refused(eng, what):
    text = (fastq_record({"rid": 5, "mate": None, "rev": False, "seq": "ACGT", "qual": "IIII"}) + BAD_READS[what]).encode()
    with pytest.raises(M.Malformed):
        M.score([GOOD.encode()], [text])
    ev = eng.correction_eval_open()
    try:
        ev.truth_add(GOOD.encode())
        assert ev.truth_plan() == 1
        ev.add(text)
        for _ in range(2):  # sticky
            with pytest.raises(SimmrError) as err:
                ev.read()
            assert err.value.code == EINVAL, what
    finally:
        ev.close()


@pytest.mark.parametrize("what", list(BAD_TRUTH))
def test_malformed_truth_is_refused(eng, what):
    text = ("6\t16\tc1\t9\t60\t3M\t*\t0\t0\tACG\t*\tMD:Z:3\n" + BAD_TRUTH[what]).encode()
    with pytest.raises(M.Malformed):
        M.truth_of([text])
    ev = eng.correction_eval_open()
    try:
        ev.truth_add(text)
        with pytest.raises(SimmrError) as err:
            ev.truth_plan()
        assert err.value.code == EINVAL, what
        with pytest.raises(SimmrError) as err:
            ev.add(b"@5\nACGT\n+\nIIII\n")
        assert err.value.code == ESTATE, what
    finally:
        ev.close()


def test_states_and_arguments(eng):
    ev = eng.correction_eval_open()
    try:
        with pytest.raises(SimmrError) as err:
            ev.add(b"@5\nACGT\n+\nIIII\n")        # no plan
        assert err.value.code == ESTATE
        with pytest.raises(SimmrError) as err:
            ev.entries()
        assert err.value.code == ESTATE
        with pytest.raises(SimmrError) as err:
            ev.reset(3)
        assert err.value.code == EINVAL
        ev.reset(0)                                # the default: four lines
        assert ev.truth_plan() == 0                # an empty truth
        ev.add(b"@5\nACGT\n+\nIIII\n")
        counts, cube, _, _ = ev.read()
        assert counts["records"] == 1 and counts["unknown_read"] == 1 and counts["lines"] == 4 and not cube.any()
        ev.truth_add(GOOD.encode())                # drops the plan
        with pytest.raises(SimmrError) as err:
            ev.add(b"@5\nACGT\n+\nIIII\n")
        assert err.value.code == ESTATE
        assert ev.truth_plan() == 1 and ev.last_ms() >= 0.0
    finally:
        ev.close()
    h = _abi.C.c_void_p()
    assert eng.lib.simmr_correval_create(eng._h, _abi.C.byref(h)) == 0
    try:
        assert eng.lib.simmr_correval_truth_add(h, None, 0) == ESTATE       # before a reset
        assert eng.lib.simmr_correval_truth_plan(h, None) == ESTATE
        assert eng.lib.simmr_correval_read(h, None, None, None, None) == ESTATE
    finally:
        eng.lib.simmr_correval_destroy(h)
