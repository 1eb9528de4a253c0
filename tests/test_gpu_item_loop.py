"""The item loop of k_emit_philox against the CPU oracle, bit for bit, where its per-read record decides the result.

What an item needs of its read — where its bases and qualities go, which way the read runs, how many of the item's
sixteen bases are live, where its plane word lies — comes out of the 32-byte record the block's prologue writes
(kernels.hip: PhRec).  The cases here are the smallest at which a wrong record field shows: two full blocks and a
partial one of pairs in both layouts, read lengths on both sides of every item boundary, the TEXT and COPY_ONLY forms
of the same loop, and blocks with more items than the LDS item map holds, where an item finds its read by binary
search or by walking."""
import numpy as np
import pytest

from simmr_amd import MinimalLongErrorProfile, MinimalShortErrorProfile, _abi
from tests import _fastq, _oracle, _synth
from tests.test_gpu_blockloop import assert_counters, expected_counters
from tests.test_gpu_cli import FMT
from tests.test_gpu_parity import COLS, assert_same
from tests.test_gpu_slots import check_raw_layout

pytestmark = pytest.mark.gpu

PAIRS = 128 + 128 + 37  # kernels.hip: PHILOX_UNITS = 128 pairs per block
MAP_ITEMS = 4096        # kernels.hip: PHILOX_MAP_ITEMS
EDGE_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 150, 160, 161)
G_MULTI, G_ONE = 1, 0


@pytest.fixture(scope="module")
def genomes(engine):
    multi = _synth.synthetic_contigs([200_000, 90_001, 30_017, 70_000, 123_457], 7)
    one = _synth.synthetic_contigs([400_000], 3)
    engine.stage_genome(G_MULTI, multi)
    engine.stage_genome(G_ONE, one)
    return {G_MULTI: _oracle.HostGenome(multi), G_ONE: _oracle.HostGenome(one)}


def run_pairs(eng, lib, genomes, prof, pairs, seed, slot, max_len=1024, gidx=G_MULTI):
    """one paired run in the layout `slot` against the oracle: every column, seq_off and the run counters"""
    eng.set_read_slots(slot)
    try:
        eng.counters_reset()
        dev = eng.simulate_pe_reads_from_genome(gidx, prof, 2 * pairs, seed, qual_offset=33)
        cnt = eng.counters()
    finally:
        eng.set_read_slots(0)
    assert dev.n_reads == 2 * pairs and dev.slot_bytes == slot
    if slot:
        check_raw_layout(dev)  # padding bytes 0, a reverse mate's bases right-aligned
    o = _oracle.simulate_pe(lib, genomes[gidx], prof, 2 * pairs, seed, qual_offset=33, max_len=max_len).trimmed()
    assert_same(dev.to_host(), o)
    o["genome"][:] = gidx
    # (CNT_OUTER_REJECTS is the plan kernel's and cannot be had from the oracle's arrays: tests/test_gpu_blockloop.py)
    assert_counters(cnt, expected_counters(lib, o, genomes, 33))
    return o


@pytest.mark.parametrize("slot", [16, 0], ids=["slot16", "compact"])
def test_pairs_two_full_blocks_and_a_partial_one(engine, oracle, genomes, slot):
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
    o = run_pairs(engine, oracle, genomes, prof, PAIRS, 42, slot)
    assert len(np.unique(o["contig"])) > 1


@pytest.mark.parametrize("slot", [16, 0], ids=["slot16", "compact"])
def test_pair_lengths_around_the_item_boundaries(engine, oracle, genomes, slot):
    """a plan of 150 pairs (a full block and a partial one) around each length: the drawn inserts cut the mates to
    lengths on both sides of it, down to reads without a base"""
    seen = set()
    for L in EDGE_LENGTHS:
        prof = MinimalShortErrorProfile(read_length=L, insert_size=max(L + L // 2, 2), rng_mode=_abi.RNG_PHILOX_FULL).pod()
        o = run_pairs(engine, oracle, genomes, prof, 150, 5 + L, slot)
        seen |= set(np.diff(o["seq_off"].astype(np.int64)).tolist())
    assert set(EDGE_LENGTHS) <= seen, f"no pair has a mate of length {sorted(set(EDGE_LENGTHS) - seen)}: choose other seeds"


@pytest.fixture(scope="module")
def short_long_reads(oracle, genomes):
    """unpaired reads with per-read lengths on both sides of every item boundary, in one plan"""
    lp = MinimalLongErrorProfile(gamma_mean=80.0, gamma_std=70.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX,
                                 mean_phred_score=20).pod()
    idx, reads = [G_MULTI, G_ONE], [3000, 2000]
    o = _oracle.simulate_long(oracle, [genomes[g] for g in idx], reads, lp, 11, qual_offset=33).trimmed()
    o["genome"] = np.array(idx, dtype=np.uint32)[o["genome"]]
    return lp, idx, reads, o


def run_long(eng, lib, genomes, lp, idx, reads, seed, slot, o):
    eng.set_read_slots(slot)
    try:
        eng.counters_reset()
        dev = eng.simulate_long_reads(idx, reads, lp, seed, qual_offset=33)
        cnt = eng.counters()
    finally:
        eng.set_read_slots(0)
    assert dev.slot_bytes == slot
    if slot:
        check_raw_layout(dev)
    assert_same(dev.to_host(), o, cols=COLS + ("genome",))
    assert_counters(cnt, expected_counters(lib, o, genomes, 33))


@pytest.mark.parametrize("slot", [16, 0], ids=["slot16", "compact"])
def test_unpaired_lengths_around_the_item_boundaries(engine, oracle, genomes, short_long_reads, slot):
    lp, idx, reads, o = short_long_reads
    lengths = set(np.diff(o["seq_off"].astype(np.int64)).tolist())
    assert set(EDGE_LENGTHS) <= lengths, f"the plan lacks lengths {sorted(set(EDGE_LENGTHS) - lengths)}: choose another seed"
    run_long(engine, oracle, genomes, lp, idx, reads, 11, slot, o)


def test_text_form_of_the_same_pairs(engine, oracle, genomes):
    """k_emit_philox<.., TEXT>: the FASTQ text straight from the plan is the text of the oracle's columns"""
    names = [(G_MULTI, "multi", ["a", "b b", "c", "d" * 30, "e"])]
    for L, pairs in ((150, PAIRS), (33, 150)):
        prof = MinimalShortErrorProfile(read_length=L, insert_size=2 * L, rng_mode=_abi.RNG_PHILOX_FULL).pod()
        o = _oracle.simulate_pe(oracle, genomes[G_MULTI], prof, 2 * pairs, 42, qual_offset=33).trimmed()
        o["genome"][:] = G_MULTI
        assert engine.pe_plan(G_MULTI, prof, 2 * pairs, 42).n_reads == 2 * pairs
        got = engine.fastq_direct(FMT, names, 0).cpu().numpy().tobytes()
        _fastq.assert_same_text(got, _fastq.expected_text(o, names, FMT, True), f"L = {L}: ")


def test_copy_only_form_of_the_same_loop(engine, oracle, genomes):
    """k_emit_philox<.., COPY_ONLY>: custom-short pairs, whose bases this loop copies (another kernel draws the qualities)"""
    from simmr_amd import CustomShortErrorProfile
    from tests import _model
    keep = CustomShortErrorProfile(_model.synthetic_short_model(n_positions=120, seed=42))
    dev = engine.simulate_pe_reads_from_genome(G_MULTI, keep.pod(), 2 * PAIRS, 9, qual_offset=33)
    o = _oracle.simulate_pe(oracle, genomes[G_MULTI], keep.pod(), 2 * PAIRS, 9, qual_offset=33).trimmed()
    assert_same(dev.to_host(), o)


@pytest.mark.parametrize("slot", [16, 0], ids=["slot16", "compact"])
@pytest.mark.parametrize("L,form", [(333, "search"), (1100, "walk")])
def test_pairs_with_more_items_than_the_map(engine, oracle, genomes, slot, L, form):
    """256 reads of about L / 16 items are more than the item map holds; 64 items per read and more are walked"""
    prof = MinimalShortErrorProfile(read_length=L, insert_size=L + 200, rng_mode=_abi.RNG_PHILOX_FULL).pod()
    o = run_pairs(engine, oracle, genomes, prof, 128 + 37, 7, slot, max_len=2048, gidx=G_ONE)
    first_block = int(((np.diff(o["seq_off"].astype(np.int64)) + 15) // 16)[:256].sum())  # (128 pairs per block)
    assert first_block > MAP_ITEMS and (first_block >= 64 * 256) == (form == "walk")


@pytest.mark.parametrize("slot", [16, 0], ids=["slot16", "compact"])
@pytest.mark.parametrize("mean,std,form", [(600.0, 250.0, "search"), (5000.0, 1500.0, "walk")])
def test_long_reads_with_more_items_than_the_map(engine, oracle, genomes, slot, mean, std, form):
    lp = MinimalLongErrorProfile(gamma_mean=mean, gamma_std=std, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX,
                                 mean_phred_score=20).pod()
    idx, reads = [G_MULTI, G_ONE], [200, 121]
    o = _oracle.simulate_long(oracle, [genomes[g] for g in idx], reads, lp, 3, qual_offset=33).trimmed()
    o["genome"] = np.array(idx, dtype=np.uint32)[o["genome"]]
    g = (np.diff(o["seq_off"].astype(np.int64)) + 15) // 16
    first_block = int(g[:128].sum())  # (128 reads per block, unpaired)
    assert first_block > MAP_ITEMS and (first_block >= 64 * 128) == (form == "walk")
    run_long(engine, oracle, genomes, lp, idx, reads, 3, slot, o)
