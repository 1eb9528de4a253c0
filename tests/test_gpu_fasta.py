"""FASTA record bodies normalised and packed on the device (simmr_stage_fasta) against the host restatement of
needletail 0.4.1 normalize(false) as genome.rs:93-137 applies it (simmr_amd/host: simmr_host_normalize, itself
pinned by the reference's genome_tests.rs fixture in tests/test_host_cpp.py)."""
import ctypes as C
import itertools
from pathlib import Path

import numpy as np
import pytest

from tests import _fasta, _oracle

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def host_normalize(raw: bytes) -> bytes:
    lib = C.CDLL(str(ROOT / "simmr_amd" / "host" / "libsimmr_host.so"))
    lib.simmr_host_normalize.restype = C.c_void_p
    lib.simmr_host_normalize.argtypes = [C.c_char_p, C.c_uint64]
    lib.simmr_host_free.argtypes = [C.c_void_p]
    p = lib.simmr_host_normalize(raw, len(raw))
    try:
        return C.string_at(p)
    finally:
        lib.simmr_host_free(p)


def bodies():
    rng = np.random.default_rng(12)
    alphabet = np.frombuffer(b"ACGTacgtNnUu-.~RYKMSWBDHVX*\t \r", dtype=np.uint8)

    def body(n, width, crlf=False):
        seq = alphabet[rng.choice(alphabet.size, n, p=np.r_[np.full(8, 0.11), np.full(alphabet.size - 8, 0.12 / (alphabet.size - 8))])]
        out = bytearray()
        for i in range(0, n, width):
            out += seq[i:i + width].tobytes() + (b"\r\n" if crlf else b"\n")
        return bytes(out)
    return [body(70_001, 80), b"", body(15, 60), b"\n\n  \n", body(3_000, 7, crlf=True), body(1_048_576, 61), b"ACGT", body(1023, 1023),
            body(1024, 1 << 20), body(1025, 60)]


@pytest.mark.parametrize("contiguous", [False, True])
def test_stage_fasta_equals_host_normalize(engine, contiguous):
    raw = bodies()
    want = [host_normalize(b) for b in raw]
    min_size = 0 if contiguous else 14
    counts, n_staged = engine.stage_fasta(20, raw, contiguous=contiguous, min_size=min_size)
    assert counts == [len(w) for w in want]
    if contiguous:
        assert n_staged == 1
        whole = b"".join(w + b"N" for w in want)  # genome.rs:121-137
        n_contigs, size = engine.genome_info(20)
        assert n_contigs == 1 and size == sum(len(w) for w in want)  # Seq.size does not count the separators
        assert engine.unstage(20, 0, 0, len(whole)).tobytes() == whole
    else:
        kept = [w for w in want if len(w) > min_size]  # main.rs:117-162
        assert n_staged == len(kept) and len(kept) < len(want)
        n_contigs, size = engine.genome_info(20)
        assert n_contigs == len(kept) and size == sum(len(w) for w in kept)
        for c, w in enumerate(kept):
            assert engine.unstage(20, c, 0, len(w)).tobytes() == w, c


def test_stage_fasta_then_simulate(engine, oracle):
    """A genome staged from raw FASTA bytes simulates the same reads as the same genome staged from the host-normalised text."""
    from simmr_amd import MinimalShortErrorProfile
    from tests import _oracle
    raw = bodies()[:1] + bodies()[5:6]
    norm = [np.frombuffer(host_normalize(b), dtype=np.uint8) for b in raw]
    engine.stage_fasta(20, raw)
    engine.stage_genome(21, norm)
    prof = MinimalShortErrorProfile().pod()
    a = engine.simulate_pe_reads_from_genome(20, prof, 3000, 5, qual_offset=33).to_host()
    b = engine.simulate_pe_reads_from_genome(21, prof, 3000, 5, qual_offset=33).to_host()
    for col in ("seq", "qual", "seq_off", "start", "end", "contig", "flags"):
        assert np.array_equal(a[col], b[col]), col
    o = _oracle.simulate_pe(oracle, _oracle.HostGenome(norm), prof, 3000, 5, qual_offset=33).trimmed()
    assert np.array_equal(a["seq"], o["seq"]) and np.array_equal(a["qual"], o["qual"])


def test_stage_fasta_nothing_left(engine):
    from simmr_amd import SimmrError, PerfectShortErrorProfile
    counts, n_staged = engine.stage_fasta(22, [b"ACGT\nAC\n", b"\n"], min_size=100)
    assert counts == [6, 0] and n_staged == 0
    with pytest.raises(SimmrError):  # the slot is not staged
        engine.pe_plan(22, PerfectShortErrorProfile().pod(), 10, 1)


# ---- staging at its tile, word and record edges -----------------------------------------------------------------------------
# Every case below is held to tests/_fasta.py — the 256-entry table of the rule and the layout of genome.rs:117-148 — in
# three ways: the bases counted per record and the number of sequences staged, genome_info, and every staged sequence read
# back whole through k_unpack.  check_reads() reads the planes a second time, through the emit kernels' windows.
COLS, assert_equal = _fasta.COLS, _fasta.assert_equal
SHORT = dict(read_length=20, insert_size=20)  # minimum_genome_size() == 60
_slots = itertools.count()


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from simmr_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def tiny():
    """(e) the bodies and, per setting, what they must stage as: computed once, left unchanged"""
    raw = _fasta.tiny_record_bodies(np.random.default_rng(5))
    return raw, {key: _fasta.layout(raw, *key) for key in ((True, 0), (False, 14), (False, 0))}


def check_staged(eng, slot, want, what):
    from simmr_amd import SimmrError
    assert eng.genome_info(slot) == (len(want.contigs), sum(want.sizes)), what
    for c, w in enumerate(want.contigs):
        assert_equal(eng.unstage(slot, c, 0, w.size), w, f"{what}: staged sequence {c}")
        with pytest.raises(SimmrError):  # ... and it ends there
            eng.unstage(slot, c, w.size, 1)


def stage_and_check(eng, slot, raw, contiguous, min_size=0, want=None, what=""):
    want = want or _fasta.layout(raw, contiguous, min_size)
    counts, n_staged = eng.stage_fasta(slot, raw, contiguous=contiguous, min_size=min_size)
    assert_equal(counts, want.counts, f"{what}: bases per record")
    assert n_staged == want.n_staged, what
    check_staged(eng, slot, want, what)
    return want


def check_reads(eng, oracle, slot, want, pairs, seed, what):
    """perfect-short pairs drawn from `slot`, and from a second slot that holds the expected sequences staged as text: both
    equal to the oracle's on the expected sequences, in every column.  Returns the reads of `slot`."""
    from simmr_amd import PerfectShortErrorProfile
    ref = next(_slots)
    eng.stage_genome(ref, want.contigs, want.sizes)
    prof = PerfectShortErrorProfile(**SHORT).pod()
    o = _oracle.simulate_pe(oracle, _oracle.HostGenome(want.contigs, want.sizes), prof, 2 * pairs, seed, qual_offset=33, max_len=32).trimmed()
    a = eng.simulate_pe_reads_from_genome(slot, prof, 2 * pairs, seed, qual_offset=33).to_host()
    b = eng.simulate_pe_reads_from_genome(ref, prof, 2 * pairs, seed, qual_offset=33).to_host()
    assert a["start"].size == 2 * pairs
    for col in COLS:
        assert_equal(a[col], o[col], f"{what}: reads of the FASTA slot, {col}")
        assert_equal(b[col], o[col], f"{what}: reads of the text slot, {col}")
    return a


def check_long_reads(eng, oracle, slot, want, n, seed, what):
    """perfect-long reads of about 300 bases that start anywhere in the sequence; returns them"""
    from simmr_amd import PerfectLongErrorProfile, _abi
    prof = PerfectLongErrorProfile(gamma_mean=300.0, gamma_std=10.0, length_mode=_abi.LEN_PER_READ, uniform_start=True).pod()
    d = eng.simulate_long_reads([slot], [n], prof, seed, qual_offset=33).to_host()
    o = _oracle.simulate_long(oracle, [_oracle.HostGenome(want.contigs, want.sizes)], [n], prof, seed, qual_offset=33).trimmed()
    assert d["start"].size == n
    for col in COLS:
        assert_equal(d[col], o[col], f"{what}: long reads, {col}")
    return d


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contiguous", [False, True])
def test_every_byte_value(eng, contiguous):
    lined, bare = _fasta.every_byte_value(np.random.default_rng(1))
    assert set(lined) == set(range(256)) and set(bare) == set(range(256)) - set(_fasta.WHITESPACE)
    for name, raw in (("lines of 61", [lined]), ("no whitespace", [bare]), ("both", [lined, bare])):
        want = stage_and_check(eng, next(_slots), raw, contiguous, what=f"every byte value, {name}")
        assert want.counts[-1] == len(bare)  # nothing but the four whitespace values is dropped


# ---- (b) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contiguous", [False, True])
def test_tile_loop(eng, oracle, n_cu, contiguous):
    """Both FASTA kernels launch min(n_tiles, 16 * n_cu) workgroups: here every workgroup takes a second tile and some a
    third, across the end of a record and into records of one to three tiles."""
    raw = _fasta.tile_loop_bodies(np.random.default_rng(2), n_cu)
    tiles = _fasta.n_tiles(raw)
    assert tiles > 2 * 16 * n_cu, f"{tiles} tiles on {16 * n_cu} workgroups: not two trips, resize this test"
    assert -(-len(raw[0]) // _fasta.TILE) > 16 * n_cu
    slot = next(_slots)
    want = stage_and_check(eng, slot, raw, contiguous, 0 if contiguous else 60, what="tile loop")
    assert want.n_staged == (1 if contiguous else len(raw))
    check_reads(eng, oracle, slot, want, 2000, 7, "tile loop")


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contiguous", [False, True])
def test_tiles_that_keep_nothing(eng, contiguous):
    raw = _fasta.empty_tile_bodies(np.random.default_rng(3))
    gaps = np.frombuffer(raw[1], dtype=np.uint8).reshape(-1)
    kept = [int((~_fasta.DROPPED[gaps[t:t + _fasta.TILE]]).sum()) for t in range(0, gaps.size, _fasta.TILE)]
    assert [k == 0 for k in kept] == [True, True, False, True, True, False, False, False, True, True], kept
    assert [len(b) for b in raw[3:]] == [1024, 2048, 1025] and not any(_fasta.DROPPED[b[-1]] for b in raw[3:])
    want = stage_and_check(eng, next(_slots), raw, contiguous, what="tiles that keep nothing")
    assert want.counts[1] == 1705 and want.counts[3:] == [1024, 2048, 1025]


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "descending", "every phase"])
def test_kept_counts_per_tile(eng, order):
    rng = np.random.default_rng(4)
    if order == "every phase":
        body, met = _fasta.kept_count_phases_body(rng)
        assert met == {(k, p) for k in _fasta.KEPT_COUNTS for p in range(32)}
    else:
        body = _fasta.kept_count_body(rng, reverse=order == "descending")
        assert len(body) == len(_fasta.KEPT_COUNTS) * _fasta.TILE
    for contiguous in (False, True):
        want = stage_and_check(eng, next(_slots), [b"ACGTN", body, b"-acgt"], contiguous, what=f"kept counts, {order}")
        assert want.counts[1] >= sum(_fasta.KEPT_COUNTS)


# ---- (e) ----------------------------------------------------------------------------------------------------------------------
def test_many_tiny_records_contiguous(eng, oracle, tiny):
    """Several records, their separators and the next tile's head in one 16-base code word and one 32-base mask word."""
    raw, wants = tiny
    want = wants[(True, 0)]
    seps = _fasta.separators(want.counts)
    assert np.diff(seps).min() == 1 and np.bincount(seps >> 5).max() >= 3 and np.bincount(seps >> 4).max() >= 2
    slot = next(_slots)
    stage_and_check(eng, slot, raw, True, want=want, what="tiny records")
    got = eng.unstage(slot, 0, 0, want.contigs[0].size)
    assert (got[seps] == ord("N")).all() and seps[-1] == got.size - 1
    pure = np.concatenate([np.arange(s - c, s) for i, (s, c) in enumerate(zip(seps, want.counts)) if i % 3 == 0])
    assert np.isin(got[pure], _fasta.ACGT).all()  # ... and nowhere else in the records written as pure ACGT
    check_reads(eng, oracle, slot, want, 3000, 8, "tiny records")
    d = check_long_reads(eng, oracle, slot, want, 200, 9, "tiny records")
    lo, hi = np.minimum(d["start"], d["end"]), np.maximum(d["start"], d["end"])
    crossed = np.searchsorted(seps, hi) - np.searchsorted(seps, lo)
    assert crossed.min() >= 5 and (hi - lo).min() >= 200


@pytest.mark.parametrize("min_size", [14, 0])
def test_many_tiny_records_min_size(eng, tiny, min_size):
    """main.rs:124 keeps a record with more than min_size bases: one of exactly min_size is absent, one of min_size + 1 is there."""
    raw, wants = tiny
    want = wants[(False, min_size)]
    assert min_size in want.counts and min_size + 1 in want.counts
    assert want.n_staged == sum(c > min_size for c in want.counts) and min(want.sizes) == min_size + 1
    stage_and_check(eng, next(_slots), raw, False, min_size, want=want, what=f"tiny records, min_size {min_size}")


# ---- (f) ----------------------------------------------------------------------------------------------------------------------
CONTIGUOUS_EDGES = {
    "first record empty": [b"", b"ACGTNacgt\n", b"GG-TT\n"],
    "two adjacent empty records": [b"ACGTAC\n", b"", b"\n", b"TTGA.CA\nAC\n"],
    "last record empty": [b"ACGTNacgt\nAC\n", b"GGTT~", b"\r\n"],
    "all records empty": [b""] * 5,
    "one empty record": [b""],
    "all records blank": [b"\n", b" \t\r\n", b"", b"\n\n"],
}


@pytest.mark.parametrize("name", list(CONTIGUOUS_EDGES))
def test_contiguous_edges(eng, name):
    raw = CONTIGUOUS_EDGES[name]
    slot = next(_slots)
    want = stage_and_check(eng, slot, raw, True, what=name)
    if name.startswith(("all records", "one empty")):  # a genome of separators only
        assert (_fasta.n_tiles(raw) == 0) == ("empty" in name)  # ... and, of empty records, one without a tile
        assert want.n_staged == 1 and want.sizes == [0]
        assert eng.unstage(slot, 0, 0, len(raw)).tobytes() == b"N" * len(raw)


def pure_acgt_bodies():
    rng = np.random.default_rng(6)
    return [_fasta.wrap(_fasta.bases(rng, n, _fasta.ACGT), 25) for n in (70, 64, 100, 33, 65, 128, 16)]


def test_contiguous_pure_acgt(eng, oracle):
    """The only exceptions are the separators: has_exc comes from k_fasta_separators alone."""
    slot = next(_slots)
    want = stage_and_check(eng, slot, pure_acgt_bodies(), True, what="pure ACGT, contiguous")
    seq, seps = want.contigs[0], _fasta.separators(want.counts)
    assert np.array_equal(np.flatnonzero(~np.isin(seq, _fasta.ACGT)), seps)
    a = check_reads(eng, oracle, slot, want, 2000, 10, "pure ACGT, contiguous")
    assert (a["seq"] == ord("N")).any()  # reads across the separators


def test_not_contiguous_pure_acgt(eng, oracle):
    """No exception anywhere: the readers are given no mask plane (has_exc == 0) and must not need one."""
    slot = next(_slots)
    want = stage_and_check(eng, slot, pure_acgt_bodies(), False, 60, what="pure ACGT, records")
    assert want.sizes == [70, 64, 100, 65, 128]
    a = check_reads(eng, oracle, slot, want, 2000, 10, "pure ACGT, records")
    assert np.isin(a["seq"], _fasta.ACGT).all()


# ---- (g) ----------------------------------------------------------------------------------------------------------------------
def test_restaging_one_slot(eng, oracle, tiny):
    """Exception-rich, then smaller and pure ACGT, then the first again, in one slot: the planes are zeroed anew and
    has_exc follows the genome that is staged."""
    raw, wants = tiny
    rich = wants[(True, 0)]
    plain_raw = [_fasta.wrap(_fasta.bases(np.random.default_rng(7), 3000, _fasta.ACGT), 70)]
    slot = next(_slots)
    for step, (bodies, contiguous, want) in enumerate([(raw, True, rich), (plain_raw, False, None), (raw, True, rich)]):
        want = stage_and_check(eng, slot, bodies, contiguous, want=want, what=f"restaging, step {step}")
        a = check_reads(eng, oracle, slot, want, 500, 11 + step, f"restaging, step {step}")
        if step == 1:
            assert want.sizes == [3000]
            assert np.isin(eng.unstage(slot, 0, 0, 3000), _fasta.ACGT).all() and np.isin(a["seq"], _fasta.ACGT).all()
        else:
            assert (a["seq"] == ord("N")).any() and (a["seq"] == ord("-")).any()
