"""simmr_asmeval_* on the GPU against the plain model of tests/_asmeval.py for exact equality: every count, the per-genome table,
the entry columns key / genome / mult / hits and the six contig columns.  A synthetic community of three genomes and an "assembly"
cut from it with errors, a chimera, a duplicate and a foreign contig; cuts of both texts into adds; every contig reverse-
complemented; k = 15, 17, 31; the table against the plain search; the malformed texts and every status code; a second plan."""
import numpy as np
import pytest

from simmr_amd import SimmrError
from simmr_amd.engine import Engine
from tests import _asmeval
from tests._asmeval import fasta, revcomp_bytes
from tests._synth import synthetic_contigs

pytestmark = pytest.mark.gpu

EINVAL, ERANGE, ENOTSUP, ESTATE = -22, -34, -95, -1


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def same(ev, model, what):
    """every table and column of the device object equals the model's"""
    counts, by = ev.read()
    want_counts, want_by = model.read()
    assert counts == want_counts, (what, {k: (counts[k], want_counts[k]) for k in counts if counts[k] != want_counts[k]})
    assert by.shape == want_by.shape and np.array_equal(by, want_by), (what, by, want_by)
    for got, want, name in zip(ev.entries(), model.entries(), ("key", "genome", "mult", "hits")):
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, name)
    for got, want, name in zip(ev.contigs(), model.contigs(), ("length", "kmers", "found", "shared", "top_genome", "top_kmers")):
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, name, got, want)


def against_model(eng, truth_pieces, contig_pieces, what, genomes, k=31, plain_search=False, model=None):
    model = model or _asmeval.evaluate(truth_pieces, contig_pieces, genomes, k)
    ev = eng.assembly_eval_open(genomes, k, plain_search)
    try:
        for t in truth_pieces:
            ev.truth_add(t)
        assert ev.truth_plan() == len(model.order), what
        for t in contig_pieces:
            ev.add(t)
        same(ev, model, what)
    finally:
        ev.close()
    return model


GENOMES = ["gA", "gB", "gC"]


def community():
    """(truth records, contig records): three genomes of a few kbp, B carrying 300 bases of A"""
    a, b, c, foreign = (x.tobytes() for x in synthetic_contigs([3000, 2500, 2100, 700], 20260101))
    b = b[:1000] + a[500:800] + b[1300:]
    truth = [(b"gA|s1:0-1400 depth_sum=9", a[:1400]), (b"gA|s1:1600-3000 depth_sum=7", a[1600:]), (b"gB|s1:0-2500 depth_sum=11", b),
             (b"gC|s1:0-900 depth_sum=1", c[:900]), (b"gC|s2:0-1100 depth_sum=2", c[1000:])]
    sub = bytearray(a[100:900])
    sub[400] = ord("A") if sub[400] != ord("A") else ord("C")
    contigs = [(b"c_exact", a[:1400]), (b"c_sub", bytes(sub)), (b"c_chimera", b[100:400] + c[200:500]), (b"c_dup", c[1200:1800]), (b"c_dup2", c[1200:1800]),
               (b"c_foreign", foreign), (b"c_short", a[:20]), (b"c_n", b[1500:1700] + b"N" + b[1701:1900].lower()), (b"c_shared", a[520:780]),
               (b"c_rc", revcomp_bytes(c[100:700])), (b"c_empty", b"")]
    return truth, contigs


def test_the_community_in_one_add_and_one_add_per_record(eng):
    truth, contigs = community()
    m = against_model(eng, [fasta(truth)], [fasta(contigs)], "one add each", GENOMES)
    c, by = m.read()
    assert min(c["contigs_short"], c["contigs_novel"], c["contigs_pure"], c["contigs_mixed"], c["contigs_shared_only"], c["shared"], c["novel"],
               c["invalid"], c["truth_shared_distinct"]) > 0 and by[:, 2].sum() > 0
    m2 = against_model(eng, [fasta([r]) for r in truth], [fasta([r]) for r in contigs], "an add per record", GENOMES)
    assert m2.read()[0] == c
    against_model(eng, [fasta(truth[:2], width=7), fasta(truth[2:], eol=b"\r\n")], [fasta(contigs[:5], width=1), fasta(contigs[5:], width=100000)],
                  "other cuts, widths and line ends", GENOMES, model=m)


def test_every_contig_reverse_complemented_gives_the_same_tables(eng):
    truth, contigs = community()
    m = _asmeval.evaluate([fasta(truth)], [fasta(contigs)], GENOMES)
    against_model(eng, [fasta(truth)], [fasta([(n, revcomp_bytes(s)) for n, s in contigs])], "reverse complements", GENOMES, model=m)


@pytest.mark.parametrize("k", [15, 17, 31])
def test_k(eng, k):
    truth, contigs = community()
    against_model(eng, [fasta(truth)], [fasta(contigs)], f"k = {k}", GENOMES, k=k)
    against_model(eng, [fasta(truth)], [fasta(contigs)], f"k = {k}, the plain search", GENOMES, k=k, plain_search=True)


def test_empty_texts(eng):
    truth, contigs = community()
    against_model(eng, [b""], [b""], "empty", GENOMES)
    against_model(eng, [], [fasta(contigs)], "an empty truth: everything novel", GENOMES)
    against_model(eng, [fasta(truth)], [], "an empty candidate", GENOMES)
    against_model(eng, [b"\n\n"], [b"\n\r\n"], "empty lines alone", GENOMES)
    against_model(eng, [b">gA|x\n"], [b">c\n>d"], "headers alone", GENOMES)


def test_a_second_plan_after_more_truth_adds(eng):
    truth, contigs = community()
    ev = eng.assembly_eval_open(GENOMES, 21)
    try:
        ev.truth_add(fasta(truth[:2]))
        ev.truth_plan()
        ev.add(fasta(contigs))
        same(ev, _asmeval.evaluate([fasta(truth[:2])], [fasta(contigs)], GENOMES, 21), "the first plan")
        ev.truth_add(fasta(truth[2:]))
        with pytest.raises(SimmrError) as err:
            ev.add(fasta(contigs))
        assert err.value.code == ESTATE
        ev.truth_plan()
        for r in contigs:
            ev.add(fasta([r]))
        same(ev, _asmeval.evaluate([fasta(truth)], [fasta(contigs)], GENOMES, 21), "the second plan")
        assert ev.ms()[0] > 0
    finally:
        ev.close()


def test_malformed_texts_and_every_status_code(eng):
    truth, contigs = community()
    for k in (13, 16, 33, 0):
        with pytest.raises(SimmrError) as err:
            eng.assembly_eval_open(GENOMES, k)
        assert err.value.code == EINVAL
    with pytest.raises(SimmrError) as err:
        eng.assembly_eval_open(["gA", "gA"])
    assert err.value.code == EINVAL
    with pytest.raises(SimmrError) as err:
        eng.assembly_eval_open(["g A"])
    assert err.value.code == ENOTSUP
    for bad in (b"ACGT\n>gA|x\nACGT\n", b">gA\nACGT\n", b">gA x|y\nACGT\n", b">gZ|x\nACGT\n", b">|x\nACGT\n"):
        ev = eng.assembly_eval_open(GENOMES)
        try:
            ev.truth_add(bad)
            with pytest.raises(SimmrError) as err:
                ev.truth_plan()
            assert err.value.code == EINVAL, bad
            with pytest.raises(SimmrError) as err:
                ev.read()
            assert err.value.code == EINVAL, bad
        finally:
            ev.close()
    ev = eng.assembly_eval_open(GENOMES)
    try:
        with pytest.raises(SimmrError) as err:
            ev.add(fasta(contigs))
        assert err.value.code == ESTATE
        with pytest.raises(SimmrError) as err:
            ev.entries()
        assert err.value.code == ESTATE
        ev.truth_add(fasta(truth))
        n = ev.truth_plan()
        ev.add(fasta(contigs))
        import ctypes as C
        assert ev.lib.simmr_asmeval_emit(ev._h, None, None, None, None, n - 1) == ERANGE
        assert ev.lib.simmr_asmeval_contigs(ev._h, None, None, None, None, None, None, len(contigs) - 1, None) == ERANGE
        assert ev.lib.simmr_asmeval_truth_add(ev._h, None, 5) == EINVAL
        assert ev.lib.simmr_asmeval_truth_add(ev._h, C.c_void_p(8), 0x80000000) == ENOTSUP
        ev.truth_plan()
        ev.add(b"ACGT\n>c\nACGT\n")  # sticky on the candidate side
        with pytest.raises(SimmrError) as err:
            ev.read()
        assert err.value.code == EINVAL
    finally:
        ev.close()


def test_the_one_call_form(eng):
    truth, contigs = community()
    counts, by, entries, cols = eng.assembly_eval(fasta(truth), [fasta(contigs[:4]), fasta(contigs[4:])], GENOMES, k=17)
    m = _asmeval.evaluate([fasta(truth)], [fasta(contigs)], GENOMES, 17)
    assert (counts, by.tolist()) == (m.read()[0], m.read()[1].tolist())
    assert all(np.array_equal(a, b) for a, b in zip(entries, m.entries())) and all(np.array_equal(a, b) for a, b in zip(cols, m.contigs()))
