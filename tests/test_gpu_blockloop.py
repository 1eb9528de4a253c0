"""The block loop of the emit kernels against the CPU oracle, bit for bit.

Every other comparison with the oracle runs at a size where a workgroup of k_emit_philox handles exactly one block of
128 units, so the code that runs when a workgroup takes its second or twelfth block — the barrier that frees the read
records, the scans and the LDS item map of the new block, the counters a lane carries from block to block — was checked by
the full-size property tests alone, which an error that a whole run and its shards make alike passes.  Here a second
engine launches ONE workgroup per CU (SIMMR_PHILOX_WGS_PER_CU=1, SIMMR_GRID_MULT=1: engine.hip, the grid lines that
tests/test_host.py::test_block_loop_tests_are_sized_from_the_kernels_constants pins), every run has more than three blocks
per workgroup plus a partial last one, and every column and every run counter is the oracle's.

CNT_OUTER_REJECTS is the plan kernels' (nothing of the emit loop feeds it) and cannot be had from the oracle's arrays:
tests/test_gpu_shapes.py::test_results_do_not_depend_on_the_grid compares it between grids.

Each case is named after the instantiation of engine.hip's philox_kernel / philox_text_kernel it is meant to reach."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import (MinimalLongErrorProfile, MinimalShortErrorProfile, PerfectLongErrorProfile,
                       PerfectShortErrorProfile, _abi)
from tests import _fastq, _oracle, _synth
from tests.test_gpu_cli import FMT  # (every field of the header template)
from tests.test_gpu_parity import COLS, assert_same

pytestmark = pytest.mark.gpu

UNITS = 128          # kernels.hip: PHILOX_UNITS
TRIPS = 3
PERFECT_GROUP = 256  # kernels.hip: reads per workgroup iteration of k_emit_perfect_pe
LANES_WG = 512       # kernels.hip: reads per workgroup iteration of k_emit_lanes
# k_emit_lanes' grid is n_cu * per_cu * SIMMR_GRID_MULT with per_cu from hipOccupancyMaxActiveBlocksPerMultiprocessor: a
# workgroup is 8 waves with 512 * 136 = 69 632 bytes of LDS (RING_PITCH), so the CU's 160 KB hold two, and the four waves
# per SIMD that tests/test_resource_guard.py holds the kernel to are two workgroups as well
LANES_PER_CU_MAX = 2
THREADS = 16
NAMES = {0: (0, "g", ["the only sequence of genome zero"]),
         1: (1, "genome-with-exceptions", ["x", "second one"]),
         2: (2, "70c", ["c%d" % i + "_" * (i % 9) for i in range(70)])}


def _engine_with(env):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from simmr_amd.engine import Engine
    mp = pytest.MonkeyPatch()
    try:
        for k, v in env.items():
            mp.setenv(k, v)  # (read once, at engine creation)
        return Engine(0)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def genomes():
    rng = np.random.default_rng(21)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    seq = acgt[rng.integers(0, 4, 300_000)].copy()
    seq[rng.integers(0, 300_000, 30_000)] = ord("N")
    seq[rng.integers(0, 300_000, 5_000)] = ord("-")
    seq[120_000:120_700] = ord("N")
    many = _synth.synthetic_contigs([6000 + 37 * i for i in range(70)], 11)
    return {0: _oracle.HostGenome(_synth.synthetic_contigs([1_000_000], 1)),
            1: _oracle.HostGenome([seq, seq[:90_001].copy()]),
            2: _oracle.HostGenome(many)}


def _stage(eng, genomes):
    for idx, g in genomes.items():
        eng.stage_genome(idx, g.contigs)


@pytest.fixture(scope="module")
def loop(genomes):
    """one workgroup of the item kernel per CU, and the smallest grids of the other emit kernels"""
    eng = _engine_with({"SIMMR_PHILOX_WGS_PER_CU": "1", "SIMMR_GRID_MULT": "1"})
    _stage(eng, genomes)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def loop_lines(genomes):
    """the same grids with the whole-line text kernel wherever it applies (SIMMR_TEXT_FORM=2, text_lines.hip)"""
    eng = _engine_with({"SIMMR_PHILOX_WGS_PER_CU": "1", "SIMMR_GRID_MULT": "1", "SIMMR_TEXT_FORM": "2"})
    _stage(eng, genomes)
    yield eng
    eng.close()


def units_for(n_cu):
    return UNITS * TRIPS * n_cu + 77


def assert_loops(units, n_cu, trips=TRIPS, per_block=UNITS, wgs_per_cu=1):
    """the premise: with `wgs_per_cu * n_cu` workgroups, some workgroup takes more than `trips` blocks"""
    blocks = -(-units // per_block)
    assert blocks > trips * wgs_per_cu * n_cu, f"{blocks} blocks on {wgs_per_cu * n_cu} workgroups: not {trips} trips, resize this test"
    return blocks


_comp = None


def complement_lut(lib):
    global _comp
    if _comp is None:
        _comp = np.array([lib.orc_complement(b) for b in range(256)], dtype=np.uint8)
    return _comp


def count_substitutions(lib, o, genomes, chunk=20_000):
    """bases of the reads that differ from the genome: forward reads against their slice, reverse-complemented ones after
    undoing the reverse complement (start > end for a pair's second mate, simulate.rs:295-296)"""
    comp = complement_lut(lib)
    n = len(o["start"])
    st, en = o["start"].astype(np.int64), o["end"].astype(np.int64)
    lo, L = np.minimum(st, en), np.abs(en - st)
    off = o["seq_off"].astype(np.int64)
    assert np.array_equal(np.diff(off), L)
    rev = (o["flags"] & _abi.FLAG_REVCOMP) != 0
    flat, base, at = [], {}, 0
    for g in sorted(set(int(x) for x in np.unique(o["genome"]))):
        bases = []
        for c in genomes[g].contigs:
            bases.append(at)
            flat.append(c)
            at += c.size
        base[g] = np.array(bases, dtype=np.int64)
    flat = np.concatenate(flat)
    cb = np.zeros(n, dtype=np.int64)
    for g, b in base.items():
        m = o["genome"] == g
        cb[m] = b[o["contig"][m]]
    mism = 0
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        Lc = L[a:b]
        within = np.arange(int(off[b] - off[a]), dtype=np.int64) - np.repeat(off[a:b] - off[a], Lc)
        r_rev = np.repeat(rev[a:b], Lc)
        src = np.repeat(cb[a:b] + lo[a:b], Lc) + np.where(r_rev, np.repeat(Lc, Lc) - 1 - within, within)
        ref = flat[src]
        ref = np.where(r_rev, comp[ref], ref)
        mism += int((o["seq"][off[a]:off[b]] != ref).sum())
    return mism


def expected_counters(lib, o, genomes, qual_offset):
    """seven of the eight run counters from the oracle's arrays (CNT_OUTER_REJECTS: see the module's docstring)"""
    fl = o["flags"]
    acgt = np.zeros(256, dtype=bool)
    acgt[[65, 67, 71, 84]] = True
    return {_abi.CNT_READS: len(o["start"]), _abi.CNT_BASES: int(o["seq_off"][-1]),
            _abi.CNT_ACGT_BASES: int(acgt[o["seq"]].sum()),
            _abi.CNT_SUBSTITUTIONS: count_substitutions(lib, o, genomes),
            _abi.CNT_REDRAWN: int(((fl & _abi.FLAG_REDRAWN) != 0).sum()),
            _abi.CNT_SEED_SUBST: int(((fl & _abi.FLAG_QSEED_SUBST) != 0).sum() + ((fl & _abi.FLAG_MSEED_SUBST) != 0).sum()),
            _abi.CNT_QUAL_SUM: int(((o["qual"].astype(np.int64) - qual_offset) % 256).sum())}


CNT_NAMES = {getattr(_abi, k): k for k in dir(_abi) if k.startswith("CNT_")}


def assert_counters(got, want, what=""):
    print(what, "counters:", {CNT_NAMES[k]: (int(got[k]), v) for k, v in want.items()})
    for k, v in want.items():
        assert int(got[k]) == v, f"{what}{CNT_NAMES[k]}: device {int(got[k])}, from the oracle's arrays {v}"


def check_pe(eng, lib, genomes, gidx, prof, n_cu, *, first, read_id_base, qual_offset=33, seed=42, max_len=1024, slot=0,
             pairs=None, per_block=UNITS, wgs_per_cu=1, trips=TRIPS, skip_counters=()):
    pairs = units_for(n_cu) if pairs is None else pairs
    assert_loops(pairs, n_cu, trips, per_block, wgs_per_cu)
    total = 2 * (first + pairs) + (5 if first else 0)  # a shard in the middle of a longer run, or the whole run
    eng.set_read_slots(slot)
    try:
        eng.counters_reset()
        dev = eng.simulate_pe_reads_from_genome(gidx, prof, total, seed, first=first, count=pairs, read_id_base=read_id_base,
                                                qual_offset=qual_offset)
        cnt = eng.counters()
    finally:
        eng.set_read_slots(0)
    assert dev.n_reads == 2 * pairs
    if slot:
        from tests.test_gpu_slots import check_raw_layout
        check_raw_layout(dev)
    o = _oracle.simulate_pe(lib, genomes[gidx], prof, total, seed, first=first, count=pairs, read_id_base=read_id_base,
                            qual_offset=qual_offset, max_len=max_len, threads=THREADS).trimmed()
    assert_same(dev.to_host(), o)
    o["genome"][:] = gidx
    want = expected_counters(lib, o, genomes, qual_offset)
    for k in skip_counters:
        del want[k]
    assert_counters(cnt, want)
    return o


def qmax1(lib, kind, mean_phred):
    """engine.hip's philox_qmax1 (the largest Phred a level-1 cell of the quality table answers) from the oracle's own
    statement of the table, oracle/philox.c: column k answers A in T of its 16384 cells and B in the rest"""
    t1 = (C.c_uint64 * 1024)()
    t2 = (C.c_uint32 * 1024)()
    lib.orc_philox_tables.restype = C.c_uint32
    lib.orc_philox_tables.argtypes = [C.c_uint32, C.c_uint8, C.c_void_p, C.c_void_p]
    lib.orc_philox_tables(kind, mean_phred, t1, t2)
    q = 0
    for e in t1:
        T, A, B = e & 0xffff, (e >> 16) & 0xffff, (e >> 32) & 0xffff
        for n_cells, oc in ((T, A), (16384 - T, B)):
            if n_cells > 0 and oc != 1024:  # (1024: the escape, ORC_PHILOX_ESC)
                q = max(q, oc & 255)
    return q


# ---- 1, 2: <EXC=0, CACHED, ESCQ, COARSE>, compact and SLOT: the benchmark's kernel ---------------------------------------
@pytest.mark.parametrize("first", [0, 7], ids=["whole", "shard"])
def test_philox_full_cached(loop, oracle, genomes, n_cu, first):
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
    check_pe(loop, oracle, genomes, 0, prof, n_cu, first=first, read_id_base=11 if first else 0)


def test_philox_full_cached_slot16(loop, oracle, genomes, n_cu):
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
    check_pe(loop, oracle, genomes, 0, prof, n_cu, first=7, read_id_base=11, slot=16)


# ---- 3: <EXC=1, CACHED, ESCQ, COARSE>, the plan from the reference's streams ----------------------------------------------
def test_philox_exceptions_cached(loop, oracle, genomes, n_cu):
    prof = MinimalShortErrorProfile(mean_phred_score=8, rng_mode=_abi.RNG_PHILOX).pod()
    check_pe(loop, oracle, genomes, 1, prof, n_cu, first=3, read_id_base=5)


# ---- 4: not CACHED: more contigs than PHILOX_CBASE, and several genomes in one plan ----------------------------------------
def test_philox_many_contigs_not_cached(loop, oracle, genomes, n_cu):
    assert len(genomes[2].contigs) > 64
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX).pod()
    o = check_pe(loop, oracle, genomes, 2, prof, n_cu, first=9, read_id_base=1)
    assert int(o["contig"].max()) >= 64  # (the cached form would have read cbase[contig & 63])


def multi_plan(lib, genomes, n_cu):
    """[genome 2, genome 0 with no reads, genome 1 (exception bases)]: the oracle's per-genome runs, concatenated"""
    pairs = units_for(n_cu)
    p0 = pairs // 2 + 5
    assert p0 % UNITS != 0 and (p0 // UNITS) > n_cu  # u_genome changes inside a block, and not in a workgroup's first
    idx, reads = [2, 0, 1], [2 * p0 + 1, 0, 2 * (pairs - p0)]
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
    parts, base = [], 0
    for g, n in zip(idx, reads):
        p = _oracle.simulate_pe(lib, genomes[g], prof, n, 9, read_id_base=base, qual_offset=33, threads=THREADS).trimmed()
        p["genome"][:] = g
        parts.append(p)
        base += n // 2
    o = {c: np.concatenate([p[c] for p in parts]) for c in ("start", "end", "contig", "genome", "read_id", "flags", "qual", "seq")}
    lens = np.concatenate([np.diff(p["seq_off"].astype(np.int64)) for p in parts])
    o["seq_off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return idx, reads, prof, pairs, o


def test_philox_three_genomes_in_one_plan(loop, oracle, genomes, n_cu):
    idx, reads, prof, pairs, o = multi_plan(oracle, genomes, n_cu)
    assert_loops(pairs, n_cu)
    loop.counters_reset()
    dev = loop.simulate_pe_reads_multi(idx, reads, prof, 9, qual_offset=33)
    cnt = loop.counters()
    assert dev.n_reads == 2 * pairs
    assert_same(dev.to_host(), o, cols=COLS + ("genome",))
    assert_counters(cnt, expected_counters(oracle, o, genomes, 33))


# ---- 5: the flag-bit form, ESCQ = false -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean_phred,qual_offset", [(30, 100), (240, 33)], ids=["offset-100", "phred-240-wraps"])
def test_philox_flag_bit_form(loop, oracle, genomes, n_cu, mean_phred, qual_offset):
    """engine.hip selects ESCQ = false when qual_offset + philox_qmax1 > 127.  The Python mirror of the profile does not
    carry philox_qmax1, so it is computed from the oracle's statement of the table (qmax1 above) and the precondition is
    asserted.  Mean Phred 240 with offset 33 also wraps most encoded qualities (q + 33 is a u8 add, util.rs:46-50)."""
    assert qual_offset + qmax1(oracle, _abi.MINIMAL_SHORT, mean_phred) > 127
    prof = MinimalShortErrorProfile(mean_phred_score=mean_phred, rng_mode=_abi.RNG_PHILOX).pod()
    o = check_pe(loop, oracle, genomes, 1, prof, n_cu, first=5, read_id_base=2, qual_offset=qual_offset)
    if mean_phred == 240:
        assert (o["qual"] < 33).any()


# ---- 6: long reads: not coarse, per-read offsets ------------------------------------------------------------------------------
def check_long(eng, lib, genomes, idx, reads, prof, n_cu, *, first, count, read_id_base, trips, seed=3):
    blocks = assert_loops(count, n_cu, trips)
    eng.counters_reset()
    dev = eng.simulate_long_reads(idx, reads, prof, seed, first=first, count=count, read_id_base=read_id_base, qual_offset=33)
    cnt = eng.counters()
    o = _oracle.simulate_long(lib, [genomes[g] for g in idx], reads, prof, seed, first=first, count=count,
                              read_id_base=read_id_base, threads=THREADS, qual_offset=33).trimmed()
    o["genome"] = np.array(idx, dtype=np.uint32)[o["genome"]]
    assert dev.n_reads == count
    assert_same(dev.to_host(), o, cols=COLS + ("genome",))
    assert_counters(cnt, expected_counters(lib, o, genomes, 33))
    # items (16 bases) per block, from the oracle's lengths: which way an item finds its read (kernels.hip: `locate`)
    g = (np.diff(o["seq_off"].astype(np.int64)) + 15) // 16
    pad = np.zeros(blocks * UNITS, dtype=np.int64)
    pad[:count] = g
    items = pad.reshape(blocks, UNITS).sum(axis=1)
    nr = np.minimum(UNITS, count - UNITS * np.arange(blocks))
    later = np.arange(blocks) >= n_cu  # blocks that are not a workgroup's first
    return items, nr, later


def test_philox_long_reads_binary_search(loop, oracle, genomes, n_cu):
    """gamma(600, 250): 128 reads x 38 items are more than the 4096 the LDS item map holds and fewer than 64 per read"""
    lp = MinimalLongErrorProfile(gamma_mean=600.0, gamma_std=250.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX,
                                 mean_phred_score=20).pod()
    n = units_for(n_cu)
    items, nr, later = check_long(loop, oracle, genomes, [1, 0], [n // 2, n - n // 2 + 40], lp, n_cu, first=21, count=n,
                                  read_id_base=3, trips=TRIPS)
    search = (items > 4096) & (items < 64 * nr)
    # (every full block after a workgroup's first: the partial last block's 77 reads fit the item map)
    assert (search & later).sum() >= (TRIPS - 1) * n_cu, "the later blocks should take the binary search"


def test_philox_long_reads_walk(loop, oracle, genomes, n_cu):
    """gamma(3000, 2500): at least 64 items per read on average: `walk`.  The count keeps the oracle's output under about
    300 MB (100 000 reads of 3000 bases); on 256 CUs that is still the module's three trips and a partial block."""
    lp = MinimalLongErrorProfile(gamma_mean=3000.0, gamma_std=2500.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX,
                                 mean_phred_score=20).pod()
    n = min(units_for(n_cu), 100_000)
    trips = TRIPS if -(-n // UNITS) > TRIPS * n_cu else 2  # (more than 260 CUs: two trips, asserted below)
    items, nr, later = check_long(loop, oracle, genomes, [1, 0], [n // 2, n - n // 2 + 40], lp, n_cu, first=21, count=n,
                                  read_id_base=3, trips=trips)
    walk = (items > 4096) & (items >= 64 * nr)
    assert (walk & later).sum() >= (trips - 1) * n_cu


def test_philox_full_perfect_long_two_genomes(loop, oracle, genomes, n_cu):
    lp = PerfectLongErrorProfile(gamma_mean=900.0, gamma_std=700.0, length_mode=_abi.LEN_PER_READ,
                                 rng_mode=_abi.RNG_PHILOX_FULL).pod()
    n = units_for(n_cu)
    check_long(loop, oracle, genomes, [0, 2], [n // 2 + 11, n - n // 2], lp, n_cu, first=0, count=n + 11, read_id_base=0,
               trips=TRIPS)


# ---- 7: COPY_ONLY column form: custom-short pairs (k_emit_custom_pe writes the qualities) -----------------------------------
def test_custom_short_copy_only(loop, oracle, genomes, n_cu):
    from simmr_amd import CustomShortErrorProfile
    from tests import _model
    keep = CustomShortErrorProfile(_model.synthetic_short_model(n_positions=120, seed=42))
    check_pe(loop, oracle, genomes, 0, keep.pod(), n_cu, first=7, read_id_base=4)  # k_emit_philox<false, true, false>


# ---- reference mode and the perfect-short column form: their own grid-stride loops -------------------------------------------
def test_perfect_short_groups_loop(loop, oracle, genomes, n_cu):
    """k_emit_perfect_pe: min(groups of 256 reads, n_cu * 8 * SIMMR_GRID_MULT) workgroups (engine.hip): two trips and a
    partial group"""
    pairs = PERFECT_GROUP * 8 * n_cu + 77  # 2 * pairs reads
    assert -(-2 * pairs // PERFECT_GROUP) > 2 * 8 * n_cu
    check_pe(loop, oracle, genomes, 0, PerfectShortErrorProfile().pod(), n_cu, first=7, read_id_base=3, pairs=pairs,
             per_block=PERFECT_GROUP // 2, wgs_per_cu=8, trips=2)


def test_reference_mode_lanes_loop(loop, oracle, genomes, n_cu):
    """k_emit_lanes: min(workgroups of 512 reads, n_cu * per_cu * SIMMR_GRID_MULT) with per_cu <= LANES_PER_CU_MAX: two trips"""
    pairs = LANES_WG * LANES_PER_CU_MAX * n_cu + 77
    assert -(-2 * pairs // LANES_WG) > 2 * LANES_PER_CU_MAX * n_cu
    check_pe(loop, oracle, genomes, 1, MinimalShortErrorProfile(mean_phred_score=12).pod(), n_cu, first=7, read_id_base=3,
             pairs=pairs, per_block=LANES_WG // 2, wgs_per_cu=LANES_PER_CU_MAX, trips=2)


# ---- 8: TEXT forms: the FASTQ text straight from the plan, against text built from the ORACLE's columns ---------------------
def pe_text_case(name, lib, genomes, n_cu):
    pairs = units_for(n_cu)
    if name == "three-genomes":
        idx, reads, prof, pairs, o = multi_plan(lib, genomes, n_cu)
        return dict(plan=lambda e: e.pe_plan_multi(idx, reads, prof, 9), names=[NAMES[g] for g in idx], id_base=0, o=o, pairs=pairs)
    gidx, prof, first, idb = {
        "full-cached": (0, MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL), 7, 11),
        "exceptions-cached": (1, MinimalShortErrorProfile(mean_phred_score=8, rng_mode=_abi.RNG_PHILOX), 3, 5),
        "many-contigs": (2, MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX), 9, 1),
        # the text's offset is always 33 (engine.hip: escq = 33 + philox_qmax1 <= 127): the flag-bit form needs a high Phred
        "flag-bit-form": (1, MinimalShortErrorProfile(mean_phred_score=240, rng_mode=_abi.RNG_PHILOX), 5, 2),
        "perfect-copy-only": (0, PerfectShortErrorProfile(), 7, 3),
        "perfect-copy-only-exceptions": (1, PerfectShortErrorProfile(), 7, 3),
    }[name]
    if name == "flag-bit-form":
        assert 33 + qmax1(lib, _abi.MINIMAL_SHORT, 240) > 127
    pod = prof.pod()
    total = 2 * (first + pairs) + 5
    o = _oracle.simulate_pe(lib, genomes[gidx], pod, total, 42, first=first, count=pairs, read_id_base=idb, qual_offset=33,
                            threads=THREADS).trimmed()
    o["genome"][:] = gidx
    return dict(plan=lambda e: e.pe_plan(gidx, pod, total, 42, first, pairs), names=[NAMES[gidx]], id_base=idb, o=o, pairs=pairs,
                keep=prof)


@pytest.mark.parametrize("name", ["full-cached", "exceptions-cached", "many-contigs", "three-genomes", "flag-bit-form",
                                  "perfect-copy-only", "perfect-copy-only-exceptions"])
def test_text_of_pairs(loop, loop_lines, oracle, genomes, n_cu, name):
    """k_emit_philox<..., TEXT> on the item-form engine and k_emit_text_lines on the other: the same bytes, the oracle's"""
    case = pe_text_case(name, oracle, genomes, n_cu)
    assert_loops(case["pairs"], n_cu)
    want = _fastq.expected_text(case["o"], case["names"], FMT, True)
    for what, eng in (("item form: ", loop), ("whole-line form: ", loop_lines)):
        info = case["plan"](eng)
        assert info.n_reads == 2 * case["pairs"]
        got = eng.fastq_direct(FMT, case["names"], case["id_base"]).cpu().numpy().tobytes()
        _fastq.assert_same_text(got, want, what)


def test_text_of_long_reads(loop, loop_lines, oracle, genomes, n_cu):
    lp = MinimalLongErrorProfile(gamma_mean=600.0, gamma_std=250.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX,
                                 mean_phred_score=20).pod()
    n = units_for(n_cu)
    assert_loops(n, n_cu)
    idx, reads = [1, 0], [n // 2, n - n // 2 + 40]
    o = _oracle.simulate_long(oracle, [genomes[g] for g in idx], reads, lp, 3, first=21, count=n, read_id_base=3, threads=THREADS,
                              qual_offset=33).trimmed()
    o["genome"] = np.array(idx, dtype=np.uint32)[o["genome"]]
    names = [NAMES[g] for g in idx]
    want = _fastq.expected_text(o, names, FMT, False)
    for what, eng in (("item form: ", loop), ("SIMMR_TEXT_FORM=2 engine: ", loop_lines)):
        assert eng.long_plan(idx, reads, lp, 3, 21, n).n_reads == n
        _fastq.assert_same_text(eng.fastq_direct(FMT, names, 3).cpu().numpy().tobytes(), want, what)
