"""simmr_asmmap_* on the GPU against the plain model of tests/_asmmap.py for exact equality: every count, the per-genome table, the
anchor index, the nine block columns and the six contig columns.  Every hand-written case of tests/test_asmmap_host.py; a synthetic
community with a chimera, an inversion, a relocation, strays and repeats at k = 15 and 31; both texts cut into one add per record;
every contig reverse-complemented (the invariances); the malformed texts and every status code; capacities; a second read; a second
plan."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import SimmrError
from simmr_amd.engine import Engine
from tests import _asmmap
from tests._asmmap import fasta, revcomp_bytes
from tests._synth import synthetic_contigs
from tests.test_asmmap_host import CASES, G2, P

pytestmark = pytest.mark.gpu

EINVAL, ERANGE, ENOTSUP, ESTATE = -22, -34, -95, -1
GENOMES = ["gA", "gB", "gC"]


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
    for got, want, name in zip(ev.anchors(), model.anchors(), ("key", "t", "p", "o")):
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, name)
    for got, want, name in zip(ev.blocks(), model.blocks(), _asmmap.BLOCK_COLS):
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, name, got, want)
    for got, want, name in zip(ev.contigs(), model.contigs(), ("length", "hits", "blocks", "first_block", "block_bases", "worst_join")):
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, name, got, want)


def against_model(eng, truth_pieces, contig_pieces, what, genomes, model=None, **params):
    model = model or _asmmap.evaluate(truth_pieces, contig_pieces, genomes, **params)
    ev = eng.assembly_map_open(genomes, **params)
    try:
        for t in truth_pieces:
            ev.truth_add(t)
        assert ev.truth_plan() == len(model.anchor), what
        for t in contig_pieces:
            ev.add(t)
        same(ev, model, what)
    finally:
        ev.close()
    return model


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_hand_written_cases(eng, name):
    truth, contigs = CASES[name]
    against_model(eng, [fasta(truth)], [fasta(contigs)], name, G2, **P)


def community():
    """(truth records, contig records): three genomes of a few kbp, B carrying 300 bases of A (repeats)"""
    a, b, c, foreign = (x.tobytes() for x in synthetic_contigs([3000, 2500, 2100, 700], 20260101))
    b = b[:1000] + a[500:800] + b[1300:]
    truth = [(b"gA|s1:0-1400 depth_sum=9", a[:1400]), (b"gA|s1:1600-3000 depth_sum=7", a[1600:]), (b"gB|s1:0-2500 depth_sum=11", b),
             (b"gC|s1:0-900 depth_sum=1", c[:900]), (b"gC|s2:0-1100 depth_sum=2", c[1000:])]
    sub = bytearray(a[100:900])
    sub[400] = ord("A") if sub[400] != ord("A") else ord("C")
    contigs = [(b"c_exact", a[:1400]), (b"c_sub", bytes(sub)), (b"c_chimera", b[100:400] + c[200:500]), (b"c_bridge", a[1000:1400] + a[1600:2000]),
               (b"c_inv", c[1000:1300] + revcomp_bytes(c[1300:1600]) + c[1600:1900]), (b"c_reloc", b[0:300] + b[1800:2100]), (b"c_local", b[1400:1700] + b[1800:2100]),
               (b"c_stray", c[100:400] + a[2000:2040] + c[440:800]), (b"c_foreign", foreign), (b"c_short", a[:20]),
               (b"c_n", b[1500:1700] + b"N" + b[1701:1900].lower()), (b"c_shared", a[520:780]), (b"c_rc", revcomp_bytes(c[100:700])), (b"c_empty", b"")]
    return truth, contigs


def test_the_community_in_one_add_and_one_add_per_record(eng):
    truth, contigs = community()
    m = against_model(eng, [fasta(truth)], [fasta(contigs)], "one add each", GENOMES)
    c, by = m.read()
    assert min(c["breaks_inter_genome"], c["breaks_inter_record"], c["breaks_inversion"], c["breaks_relocation"], c["breaks_local"], c["stray_hits"],
               c["repeat_hits"], c["truth_repeats"], c["contigs_unplaced"], c["contigs_clean"], c["contigs_local_only"], c["contigs_misassembled"], c["invalid"]) > 0
    m2 = against_model(eng, [fasta([r]) for r in truth], [fasta([r]) for r in contigs], "an add per record", GENOMES)
    assert _asmmap.invariants(m2) == _asmmap.invariants(m) and [x.tolist() for x in m2.blocks()] == [x.tolist() for x in m.blocks()]
    against_model(eng, [fasta(truth[:2], width=7), fasta(truth[2:], eol=b"\r\n")], [fasta(contigs[:5], width=1), fasta(contigs[5:], width=100000)],
                  "other cuts, widths and line ends", GENOMES, model=m)


@pytest.mark.parametrize("k", [15, 31])
def test_every_contig_reverse_complemented_gives_the_same_tables(eng, k):
    truth, contigs = community()
    m = against_model(eng, [fasta(truth)], [fasta(contigs)], f"k = {k}", GENOMES, k=k)
    rc = against_model(eng, [fasta(truth)], [fasta([(n, revcomp_bytes(s)) for n, s in contigs])], f"reverse complements, k = {k}", GENOMES, k=k)
    assert _asmmap.invariants(rc) == _asmmap.invariants(m)


def test_empty_texts(eng):
    truth, contigs = community()
    against_model(eng, [b""], [b""], "empty", GENOMES)
    against_model(eng, [], [fasta(contigs)], "an empty truth: nothing placed", GENOMES)
    against_model(eng, [fasta(truth)], [], "an empty candidate", GENOMES)
    against_model(eng, [b"\n\n"], [b"\n\r\n"], "empty lines alone", GENOMES)
    against_model(eng, [b">gA|x\n"], [b">c\n>d"], "headers alone", GENOMES)
    against_model(eng, [fasta([truth[2], (b"gB|again", truth[2][1])])], [fasta(contigs)], "repeats alone: no anchor", GENOMES)


def test_a_second_read_and_a_plan_that_empties_the_candidate_side(eng):
    truth, contigs = community()
    ev = eng.assembly_map_open(GENOMES, 21)
    try:
        ev.truth_add(fasta(truth[:2]))
        ev.truth_plan()
        ev.add(fasta(contigs))
        first = _asmmap.evaluate([fasta(truth[:2])], [fasta(contigs)], GENOMES, 21)
        same(ev, first, "the first plan")
        same(ev, first, "a second read")
        ev.truth_add(fasta(truth[2:]))
        with pytest.raises(SimmrError) as err:
            ev.add(fasta(contigs))
        assert err.value.code == ESTATE
        counts, by = ev.read()   # the truth add has dropped the plan: the truth's sums since the reset, nothing of a plan or of the candidates
        assert counts["truth_records"] == len(truth) and counts["truth_kmers"] > 0 and not by.any()
        assert not any(counts[n] for n in _asmmap.COUNTS[4:]), counts
        ev.truth_plan()
        same(ev, _asmmap.evaluate([fasta(truth)], [], GENOMES, 21), "the plan has emptied the candidate side")
        for r in contigs:
            ev.add(fasta([r]))
        same(ev, _asmmap.evaluate([fasta(truth)], [fasta(contigs)], GENOMES, 21), "the second plan")
        assert ev.ms() > 0
    finally:
        ev.close()


def test_malformed_texts_and_every_status_code(eng):
    truth, contigs = community()
    for k in (13, 16, 33, 0):
        with pytest.raises(SimmrError) as err:
            eng.assembly_map_open(GENOMES, k)
        assert err.value.code == EINVAL
    for params in (dict(band=1001), dict(min_anchors=0), dict(relocation=2 ** 31, band=0), dict(band=65, relocation=64)):
        with pytest.raises(SimmrError) as err:
            eng.assembly_map_open(GENOMES, **params)
        assert err.value.code == EINVAL, params
    eng.assembly_map_open(GENOMES, band=64, relocation=64, min_anchors=1).close()
    with pytest.raises(SimmrError) as err:
        eng.assembly_map_open(["gA", "gA"])
    assert err.value.code == EINVAL
    with pytest.raises(SimmrError) as err:
        eng.assembly_map_open(["g A"])
    assert err.value.code == ENOTSUP
    for bad in (b"ACGT\n>gA|x\nACGT\n", b">gA\nACGT\n", b">gA x|y\nACGT\n", b">gZ|x\nACGT\n", b">|x\nACGT\n"):
        ev = eng.assembly_map_open(GENOMES)
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
    ev = eng.assembly_map_open(GENOMES)
    try:
        with pytest.raises(SimmrError) as err:
            ev.add(fasta(contigs))
        assert err.value.code == ESTATE
        for call in (ev.anchors, ev.blocks, ev.contigs):
            with pytest.raises(SimmrError) as err:
                call()
            assert err.value.code == ESTATE
        ev.truth_add(fasta(truth))
        n = ev.truth_plan()
        ev.add(fasta(contigs))
        nb, nc = C.c_uint64(), C.c_uint64()
        assert ev.lib.simmr_asmmap_anchors(ev._h, None, None, None, None, n - 1) == ERANGE
        assert ev.lib.simmr_asmmap_blocks(ev._h, None, 0, C.byref(nb)) == ERANGE and nb.value == ev.n_blocks() > 1
        assert ev.lib.simmr_asmmap_blocks(ev._h, None, nb.value - 1, None) == ERANGE and ev.lib.simmr_asmmap_blocks(ev._h, None, nb.value, None) == 0
        assert ev.lib.simmr_asmmap_contigs(ev._h, None, None, None, None, None, None, 0, C.byref(nc)) == ERANGE and nc.value == len(contigs)
        assert ev.lib.simmr_asmmap_contigs(ev._h, None, None, None, None, None, None, len(contigs) - 1, None) == ERANGE
        assert ev.lib.simmr_asmmap_truth_add(ev._h, None, 5) == EINVAL
        assert ev.lib.simmr_asmmap_truth_add(ev._h, C.c_void_p(8), 0x80000000) == ENOTSUP
        ev.truth_plan()
        ev.add(b"ACGT\n>c\nACGT\n")  # sticky on the candidate side
        with pytest.raises(SimmrError) as err:
            ev.read()
        assert err.value.code == EINVAL
    finally:
        ev.close()


def test_the_one_call_form(eng):
    truth, contigs = community()
    counts, by, cols, blocks = eng.assembly_map(fasta(truth), [fasta(contigs[:4]), fasta(contigs[4:])], GENOMES, k=17, band=32, relocation=500, min_anchors=8)
    m = _asmmap.evaluate([fasta(truth)], [fasta(contigs)], GENOMES, 17, 32, 500, 8)
    assert (counts, by.tolist()) == (m.read()[0], m.read()[1].tolist())
    assert all(np.array_equal(a, b) for a, b in zip(blocks, m.blocks())) and all(np.array_equal(a, b) for a, b in zip(cols, m.contigs()))
