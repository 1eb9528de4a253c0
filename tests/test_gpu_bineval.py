"""simmr_bineval_* on the GPU against the plain model of tests/_bineval.py for exact equality: every count, the per-genome table and
every column of the bins, the cells and the contigs; the sticky malformed answer; the same texts as one add each and, for a small
case, cut at every line end.  The cases are built by hand and from tests/_synth.py (the lengths and the shuffles)."""
import numpy as np
import pytest

from simmr_amd import SimmrError
from simmr_amd.engine import Engine
from tests import _bineval
from tests._bineval import bins_text, cut_at_every_line_end, truth_text
from tests._synth import splitmix64_words

pytestmark = pytest.mark.gpu

EINVAL, ERANGE, ENOTSUP, ESTATE = -22, -34, -95, -1
NONE = 0xffffffff
BINS = ("contigs", "bases", "none_bases", "first_record", "top_genome", "top_bases")
CELLS = ("bin", "genome", "contigs", "bases")
CONTIGS = ("genome", "length", "bin", "records")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def same(ev, model, what):
    counts, by = ev.read()
    want_counts, want_by = model.read()
    assert counts == want_counts, (what, {k: (counts[k], want_counts[k]) for k in counts if counts[k] != want_counts[k]})
    assert by.shape == want_by.shape and np.array_equal(by, want_by), (what, by, want_by)
    for fn, names in ((lambda o: o.bins(), BINS), (lambda o: o.cells(), CELLS), (lambda o: o.contigs(), CONTIGS)):
        for got, want, name in zip(fn(ev), fn(model), names):
            assert got.dtype == want.dtype and np.array_equal(got, want), (what, name, got, want)


def run(eng, truth_adds, bins_adds, label, genomes, hash_bits, model):
    ev = eng.binning_eval_open(genomes, hash_bits)
    try:
        for t in truth_adds:
            ev.truth_add(t)
        if model.malformed == "truth":
            with pytest.raises(SimmrError) as err:
                ev.truth_plan()
            assert err.value.code == EINVAL, label
            with pytest.raises(SimmrError) as err:  # sticky
                ev.truth_plan()
            assert err.value.code == EINVAL, label
            return
        assert ev.truth_plan() == len(model.t_genome), label
        for t in bins_adds:
            ev.add(t)
        if model.malformed:
            for _ in range(2):  # sticky
                with pytest.raises(SimmrError) as err:
                    ev.read()
                assert err.value.code == EINVAL, label
            return
        same(ev, model, label)
        same(ev, model, label + ", a second read")
    finally:
        ev.close()


def against_model(eng, truth_adds, bins_adds, label, genomes, hash_bits=64, every_line=False):
    model = _bineval.evaluate(truth_adds, bins_adds, genomes)
    run(eng, truth_adds, bins_adds, label, genomes, hash_bits, model)
    one_t, one_b = b"".join(bytes(t) for t in truth_adds), b"".join(bytes(t) for t in bins_adds)
    if all(bytes(t).endswith(b"\n") for t in list(truth_adds)[:-1] + list(bins_adds)[:-1]):
        assert _bineval.evaluate([one_t], [one_b], genomes).read()[0] == model.read()[0] or model.malformed
        run(eng, [one_t], [one_b], label + ", one add each", genomes, hash_bits, model)
        if every_line:
            run(eng, cut_at_every_line_end(one_t), cut_at_every_line_end(one_b), label + ", an add a line", genomes, hash_bits, model)
    return model


GENOMES = ["gA", "gB", "gC", "gD"]


def small():
    """twelve contigs of four genomes and of none, three bins, by hand"""
    truth = [(b"NODE_1_length_500_cov_8.1", 500, b"gA"), (b"NODE_2", 300, b"gA"), (b"NODE_3", 200, b"gB"), (b"k141_7", 900, b"gB"),
             (b"k141_71", 100, b"gC"), (b"k141_72", 100, b"gC"), (b"c7", 50, b"."), (b"c8", 75, b"."), (b"c9", 1000, b"gD"), (b"c10", 10, b"gA"),
             (b"c11", 0, b"gB"), (b"c12", 640, b"gC")]
    bins = [(b"NODE_1_length_500_cov_8.1", b"bin.2"), (b"NODE_2", b"bin.2"), (b"NODE_3", b"bin.2"), (b"k141_7", b"bin.1"), (b"k141_71", b"bin.1"),
            (b"k141_72", b"bin.10"), (b"c7", b"bin.10"), (b"c8", b"bin.2"), (b"c9", b"bin.1"), (b"c11", b"bin.10")]
    return truth, bins


def big(n=300, n_bins=40, seed=7):
    """about n contigs of 11 genomes and of none in n_bins bins, with unknown, repeated and unassigned contigs mixed in"""
    w = splitmix64_words(seed, 4 * n)
    genomes = [f"genome_{i:02d}" for i in range(11)]
    truth, bins = [], []
    for i in range(n):
        g = int(w[4 * i] % 12)
        truth.append((b"contig_%d" % (i * 7919 % 100003), int(w[4 * i + 1] % 50000), b"." if g == 11 else genomes[g].encode()))
    for i in range(n):
        r = int(w[4 * i + 2] % 100)
        name = truth[i][0]
        b = b"bin_%d" % (int(w[4 * i + 3] % n_bins) if r % 3 else int(w[4 * i] % 12))  # a third go to their genome's bin
        if r < 5:
            continue                              # unassigned
        bins.append((name, b))
        if r < 12:
            bins.append((name, b"bin_other"))     # repeated, the first wins
        if r > 95:
            bins.append((b"foreign_%d" % i, b))   # unknown
    return truth, bins, genomes


def test_the_small_case_in_every_cut(eng):
    truth, bins = small()
    m = against_model(eng, [truth_text(truth)], [bins_text(bins)], "small", GENOMES, every_line=True)
    c, by = m.read()
    assert c["bins"] == 3 and c["assigned"] == 10 and c["truth_none"] == 2 and c["cells"] == 9 and m.bin_names == [b"bin.2", b"bin.1", b"bin.10"]
    against_model(eng, [truth_text(truth[:5]), truth_text(truth[5:])], [bins_text(bins[:1]), bins_text(bins[1:7]), bins_text(bins[7:])], "small, cut", GENOMES)


def test_a_perfect_binning(eng):
    truth = [(b"c%d" % i, 100 + i, GENOMES[i % 4].encode()) for i in range(200)]
    bins = [(n, b"bin_" + g) for n, _, g in truth]
    c, by = against_model(eng, [truth_text(truth)], [bins_text(bins)], "perfect", GENOMES).read()
    assert c["sum_top_bases"] == c["sum_best_bases"] == c["assigned_bases"] == c["truth_bases"]
    assert c["pairs_cells"] == c["pairs_bins"] == c["pairs_genomes"] == 4 * (50 * 49 // 2)
    assert c["bins"] == c["cells"] == c["bins_c90_x5"] == c["bins_c50_x10"] == 4


def test_one_bin_for_everything_and_a_bin_per_contig(eng):
    truth = [(b"c%d" % i, 100 + i, GENOMES[i % 4].encode()) for i in range(300)]
    c, _ = against_model(eng, [truth_text(truth)], [bins_text([(n, b"all") for n, _, _ in truth])], "one bin", GENOMES).read()
    assert c["bins"] == 1 and c["cells"] == 4 and c["pairs_bins"] == 300 * 299 // 2
    c, _ = against_model(eng, [truth_text(truth)], [bins_text([(n, b"b_" + n) for n, _, _ in truth])], "a bin per contig", GENOMES).read()
    assert c["bins"] == c["cells"] == 300 and c["pairs_bins"] == c["pairs_cells"] == 0


def test_repeated_unknown_and_unassigned_contigs(eng):
    truth, bins = small()
    twice = bins[:4] + [(b"NODE_2", b"bin.1")] + bins[4:]
    m = against_model(eng, [truth_text(truth)], [bins_text(twice)], "a contig twice", GENOMES, every_line=True)
    assert m.read()[0]["repeated"] == 1 and m.contigs()[2][1] == 0 and m.contigs()[3][1] == 2
    unknown = [(b"nobody", b"bin.77")] + bins + [(b"NODE_", b"bin.1"), (b"NODE_22", b"bin.78")]
    m = against_model(eng, [truth_text(truth)], [bins_text(unknown)], "unknown contigs", GENOMES, every_line=True)
    c = m.read()[0]
    assert c["unknown_contig"] == 3 and c["bins"] == 3 and m.bins()[3][0] == 1, "an unknown contig's bin is no bin, and ordinals count it"
    c = against_model(eng, [truth_text(truth)], [bins_text(bins[:3])], "unassigned", GENOMES).read()[0]
    assert c["assigned"] == 3 and c["truth_records"] == 12
    c = against_model(eng, [truth_text(truth)], [], "no records", GENOMES).read()[0]
    assert c["assigned"] == c["bins"] == c["cells"] == 0
    against_model(eng, [], [bins_text(bins)], "no truth", GENOMES)


def test_none_contigs_and_ties(eng):
    truth = [(b"n1", 40, b"."), (b"n2", 60, b"."), (b"a1", 100, b"gA"), (b"b1", 100, b"gB"), (b"a2", 30, b"gA"), (b"c1", 30, b"gC"), (b"c2", 30, b"gC")]
    bins = [(b"n1", b"only_none"), (b"n2", b"mixed"), (b"a1", b"mixed"), (b"b1", b"mixed"), (b"a2", b"late"), (b"c1", b"late"), (b"c2", b"later")]
    m = against_model(eng, [truth_text(truth)], [bins_text(bins)], "none and ties", GENOMES, every_line=True)
    c, by = m.read()
    contigs, bases, none_bases, first, top, top_bases = m.bins()
    assert list(none_bases) == [40, 60, 0, 0] and top[0] == NONE and top_bases[0] == 0
    assert top[1] == 0 and top_bases[1] == 100, "gA and gB tie in `mixed`: the lowest row"
    assert int(by[2, 5]) == 2 and int(by[2, 6]) == 30, "gC has 30 bases in `late` and in `later`: the lowest bin row"
    assert int(by[3, 5]) == NONE and list(by[4]) == [2, 100, 2, 100, 0, 0, 0]
    # `only_none` has no top genome and is in no class.  `mixed`: top 100 of gA's 130 (76.9 %), 160 of its 260 bases foreign: in none.
    # `late`: top 30 of 130, in none.  `later`: all 30 bases are gC's, 30 of gC's 60 (50 %): c50 at both purities.
    assert [c[k] for k in ("bins_c90_x5", "bins_c70_x5", "bins_c50_x5", "bins_c90_x10", "bins_c70_x10", "bins_c50_x10")] == [0, 0, 1, 0, 0, 1]


def test_the_class_thresholds(eng):
    """genome g has 1000 truth bases; a bin holds `top` of them and `rest` of another genome: on and one base off every threshold"""
    cases = []
    for comp in (90, 70, 50):
        for top in (10 * comp - 1, 10 * comp):
            cases.append((top, 0))
    for rest, top in ((50, 950), (51, 949), (49, 951), (100, 900), (101, 899), (99, 901)):
        cases.append((top, rest))
    genomes = [f"g{i:02d}" for i in range(len(cases))] + ["other"]
    truth, bins = [(b"big_other", 10 ** 6, b"other")], []
    for i, (top, rest) in enumerate(cases):
        g = genomes[i].encode()
        truth += [(b"in_%d" % i, top, g), (b"out_%d" % i, 1000 - top, g), (b"rest_%d" % i, rest, b"other")]
        bins += [(b"in_%d" % i, b"bin%d" % i), (b"rest_%d" % i, b"bin%d" % i)]
    c = against_model(eng, [truth_text(truth)], [bins_text(bins)], "thresholds", genomes).read()[0]
    # from the construction.  The six pure bins: tops 899 | 900, 699 | 700, 499 | 500 of 1000: c90 has 1, c70 3, c50 5 of them.  The six
    # with rest: tops 950, 949, 951, 900, 899, 901, all c70 and c50, c90 but the 899; impurity 50/1000 (= 5 %), 51/1000, 49/1000,
    # 100/1000 (= 10 %), 101/1000, 99/1000: x5 holds 950 and 951, x10 all but the 899.
    assert [c[k] for k in ("bins_c90_x5", "bins_c70_x5", "bins_c50_x5", "bins_c90_x10", "bins_c70_x10", "bins_c50_x10")] == [1 + 2, 3 + 2, 5 + 2, 1 + 5, 3 + 5, 5 + 5]


def test_the_text_forms(eng):
    truth, bins = small()
    t, b = truth_text(truth), bins_text(bins)
    want = _bineval.evaluate([t], [b], GENOMES).read()
    head = b"@Version:0.9.0\n@SampleID:gsa\n\n@@SEQUENCEID\tBINID\n# a comment\n"
    m = against_model(eng, [b"#name\tlength\n\n" + t], [head + b], "the CAMI head", GENOMES, every_line=True)
    assert m.read()[0] == want[0]
    third = b"".join(line + b"\textra\t9\n" for line in b.split(b"\n") if line)
    assert against_model(eng, [t.replace(b"\n", b"\tmore\n")], [third], "further columns", GENOMES).read()[0] == want[0]
    m = against_model(eng, [truth_text(truth, b"\r\n")], [b"\r\n" + bins_text(bins, b"\r\n")], "CRLF", GENOMES, every_line=True)
    assert m.read()[0] == want[0]
    assert against_model(eng, [t[:-1]], [b[:-1]], "no last newline", GENOMES).read()[0] == want[0]
    assert against_model(eng, [t + b"\n\n"], [b"\n\n" + b + b"\n"], "empty lines", GENOMES).read()[0] == want[0]


MALFORMED_TRUTH = {
    "seven fields": b"c1\t100\t7\t5\t1\t0\t4\n",
    "one field": b"c1\n",
    "no number in field 2": b"c1\t1x0\t7\t5\t1\t0\t4\tgA\n",
    "an empty field 5": b"c1\t100\t7\t5\t\t0\t4\tgA\n",
    "a sign in field 7": b"c1\t100\t7\t5\t1\t0\t-4\tgA\n",
    "nineteen digits": b"c1\t1000000000000000000\t7\t5\t1\t0\t4\tgA\n",
    "a foreign genome": b"c1\t100\t7\t5\t1\t0\t4\tgZ\n",
    "a genome's prefix": b"c1\t100\t7\t5\t1\t0\t4\tg\n",
    "an empty genome": b"c1\t100\t7\t5\t1\t0\t4\t\n",
    "a genome field of 255 bytes": b"c1\t100\t7\t5\t1\t0\t4\t" + b"g" * 255 + b"\n",
    "a genome field of 256 bytes": b"c1\t100\t7\t5\t1\t0\t4\t" + b"g" * 256 + b"\n",
    "a genome field of 257 bytes that begins with '.'": b"c1\t100\t7\t5\t1\t0\t4\t." + b"g" * 256 + b"\n",
    "a genome field of 258 bytes that begins with a genome": b"c1\t100\t7\t5\t1\t0\t4\tgA" + b"g" * 256 + b"\n",
    "a genome field of 600 bytes": b"c1\t100\t7\t5\t1\t0\t4\t" + b"g" * 600 + b"\n",
    "an empty name": b"\t100\t7\t5\t1\t0\t4\tgA\n",
    "a blank in the name": b"c 1\t100\t7\t5\t1\t0\t4\tgA\n",
    "a control byte in the name": b"c\x011\t100\t7\t5\t1\t0\t4\tgA\n",
    "255 bytes": b"c" * 255 + b"\t100\t7\t5\t1\t0\t4\tgA\n",
    "a name twice": b"c2\t100\t7\t5\t1\t0\t4\tgA\n",
}
MALFORMED_CAND = {
    "no second field": b"c2\n",
    "an empty bin": b"c2\t\n",
    "an empty contig": b"\tbin\n",
    "a blank in the bin": b"c2\tbin 1\n",
    "a bin of 255 bytes": b"c2\t" + b"b" * 255 + b"\n",
    "a contig of 255 bytes": b"c" * 255 + b"\tbin\n",
    "a '\\r' that ends the text": b"c2\tbin\r",
}


@pytest.mark.parametrize("which", sorted(MALFORMED_TRUTH))
def test_a_malformed_truth(eng, which):
    good = truth_text([(b"c2", 10, b"gA"), (b"c3", 10, b".")])
    m = against_model(eng, [good + MALFORMED_TRUTH[which] + good.replace(b"c", b"d")], [b"c2\tb\n"], which, GENOMES)
    assert m.malformed == "truth"
    if which == "a name twice":  # across two adds too, and far apart
        filler = truth_text([(b"f%d" % i, 1, b"gB") for i in range(600)])
        assert against_model(eng, [good, filler, MALFORMED_TRUTH[which]], [], which + ", across adds", GENOMES, hash_bits=4).malformed == "truth"


@pytest.mark.parametrize("which", sorted(MALFORMED_CAND))
def test_a_malformed_candidate(eng, which):
    good = truth_text([(b"c2", 10, b"gA"), (b"c3", 10, b".")])
    m = against_model(eng, [good], [b"c3\tb\n" + MALFORMED_CAND[which]], which, GENOMES)
    assert m.malformed == "candidate"
    # the next plan empties the candidate side, the error with it
    ev = eng.binning_eval_open(GENOMES)
    try:
        ev.truth_add(good)
        ev.truth_plan()
        ev.add(MALFORMED_CAND[which])
        with pytest.raises(SimmrError):
            ev.read()
        ev.truth_plan()
        ev.add(b"c3\tb\n")
        assert ev.read()[0]["assigned"] == 1
    finally:
        ev.close()


def test_names_at_their_limits(eng):
    long_a, long_b = b"x" * 253 + b"a", b"x" * 253 + b"b"
    truth = [(b"c", 1, b"gA"), (b"cc", 2, b"gA"), (b"ccc", 4, b"gB"), (long_a, 8, b"gB"), (long_b, 16, b"gC"), (b"x" * 253, 32, b"gC"), (b"\xc3\xa9~!", 64, b"gD")]
    bins = [(b"ccc", b"B"), (b"c", b"BB"), (b"cc", b"B" * 254), (long_b, b"B" * 253 + b"C"), (long_a, b"B" * 254), (b"x" * 253, b"b"), (b"x" * 252, b"b"),
            (b"\xc3\xa9~!", b"\xc3\xa9")]
    for bits in (64, 0):
        m = against_model(eng, [truth_text(truth)], [bins_text(bins)], f"name limits, {bits} bits", GENOMES, hash_bits=bits, every_line=bits == 64)
        assert m.read()[0]["bins"] == 6 and m.read()[0]["unknown_contig"] == 1


@pytest.fixture(scope="module")
def big_case():
    truth, bins, genomes = big()
    t, b = truth_text(truth), bins_text(bins)
    return t, b, genomes, _bineval.evaluate([t], [b], genomes)


@pytest.mark.parametrize("hash_bits", [64, 16, 4, 0])
def test_hash_bits_give_the_same_answers(eng, big_case, hash_bits):
    t, b, genomes, model = big_case
    c = model.read()[0]
    assert c["truth_records"] == 300 and 30 < c["bins"] <= 53 and min(c["unknown_contig"], c["repeated"], c["truth_none"]) > 0
    assert c["assigned"] < 300
    run(eng, [t], [b], f"{hash_bits} bits", genomes, hash_bits, model)
    cut_t, cut_b = len(t) // 3, len(b) // 2
    cut_t, cut_b = t.index(b"\n", cut_t) + 1, b.index(b"\n", cut_b) + 1
    run(eng, [t[:cut_t], t[cut_t:]], [b[:cut_b], b[cut_b:]], f"{hash_bits} bits, two adds", genomes, hash_bits, model)


def test_renamed_bins_and_allowed_reorderings_give_identical_tables(eng, big_case):
    t, b, genomes, model = big_case
    lines = [ln.split(b"\t") for ln in b.split(b"\n") if ln]
    renamed = bins_text([(c, b"renamed:" + bn[::-1]) for c, bn in lines])
    run(eng, [t], [renamed], "renamed", genomes, 64, model)
    # every record that is neither a bin's first appearance nor a contig's first record moves to the end, reversed
    seen_bins, seen_contigs, keep, move = set(), set(), [], []
    for c, bn in lines:
        first = bn not in seen_bins or c not in seen_contigs
        seen_bins.add(bn)
        seen_contigs.add(c)
        (keep if first else move).append((c, bn))
    assert move
    m2 = _bineval.evaluate([t], [bins_text(keep + move[::-1])], genomes)
    assert m2.read()[0] == model.read()[0] and np.array_equal(m2.read()[1], model.read()[1])
    for got, want in zip(m2.cells() + m2.contigs()[:3], model.cells() + model.contigs()[:3]):
        assert np.array_equal(got, want)
    run(eng, [t], [bins_text(keep + move[::-1])], "reordered", genomes, 64, m2)


def test_the_states(eng):
    truth, bins = small()
    t, b = truth_text(truth), bins_text(bins)
    lib, C = eng.lib, __import__("ctypes")
    h = C.c_void_p()
    assert lib.simmr_bineval_create(eng._h, C.byref(h)) == 0
    try:
        assert lib.simmr_bineval_truth_add(h, None, 0) == ESTATE and lib.simmr_bineval_truth_plan(h, None) == ESTATE
        assert lib.simmr_bineval_read(h, None, None) == ESTATE
    finally:
        lib.simmr_bineval_destroy(h)
    with pytest.raises(SimmrError) as err:
        eng.binning_eval_open(GENOMES, hash_bits=65)
    assert err.value.code == EINVAL
    with pytest.raises(SimmrError) as err:
        eng.binning_eval_open(["gA", "gA"])
    assert err.value.code == EINVAL
    ev = eng.binning_eval_open(GENOMES)
    try:
        for call in (lambda: ev.add(b), ev.read, ev.bins):
            with pytest.raises(SimmrError) as err:
                call()
            assert err.value.code == ESTATE
        ev.truth_add(t)
        assert ev.truth_plan() == 12
        with pytest.raises(SimmrError) as err:
            ev.bins()  # no read yet
        assert err.value.code == ESTATE
        ev.add(b)
        first = ev.read()
        n = C.c_uint64(99)
        assert lib.simmr_bineval_bins(ev._h, None, None, None, None, None, None, 0, C.byref(n)) == ERANGE and n.value == 3
        assert lib.simmr_bineval_cells(ev._h, None, None, None, None, 0, C.byref(n)) == ERANGE and n.value == 9
        assert lib.simmr_bineval_contigs(ev._h, None, None, None, None, 11, C.byref(n)) == ERANGE and n.value == 12
        import torch
        guard = torch.full((3,), 7, dtype=torch.int32, device=eng.device)
        assert lib.simmr_bineval_bins(ev._h, C.c_void_p(guard.data_ptr()), None, None, None, None, None, 2, None) == ERANGE
        assert guard.cpu().tolist() == [7, 7, 7], "nothing is written on short capacity"
        second = ev.read()
        assert first[0] == second[0] and np.array_equal(first[1], second[1])
        ev.add(b"c10\tbin.new\n")  # an add after a read is scored by the next read
        with pytest.raises(SimmrError) as err:
            ev.cells()
        assert err.value.code == ESTATE
        third = ev.read()[0]
        assert third["assigned"] == first[0]["assigned"] + 1 and third["bins"] == 4
        ev.truth_add(b"")  # a truth add drops the plan
        with pytest.raises(SimmrError) as err:
            ev.add(b)
        assert err.value.code == ESTATE
        assert ev.truth_plan() == 12
        assert ev.read()[0]["records"] == 0, "the plan empties the candidate side"
        ms, sort_ms = ev.ms()
        assert ms > 0 and sort_ms >= 0
    finally:
        ev.close()
