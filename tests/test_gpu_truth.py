"""Ground truth per read (simmr_truth_plan / simmr_truth_emit, include/simmr_hip.h) against the numpy restatement of the
header's definition (tests/_truth.py), applied to the ORACLE's reads and the host genome bytes; the device reads are first
shown to be the oracle's, so nothing expected here comes from the pass under test."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import (CustomShortErrorProfile, MinimalLongErrorProfile, MinimalShortErrorProfile, PerfectLongErrorProfile,
                       PerfectShortErrorProfile, _abi)
from tests import _model, _oracle, _synth, _truth
from tests._hand_built import hand_built
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

# truth_kernels.hip: TRUTH_WG_READS reads per workgroup and iteration, at most TRUTH_WGS_PER_CU workgroups per CU
TRUTH_WG_READS = 16
TRUTH_WGS_PER_CU = 64
RNG_MODES = [_abi.RNG_REFERENCE, _abi.RNG_PHILOX, _abi.RNG_PHILOX_FULL]
RNG_IDS = ["reference", "philox", "philox-full"]


@pytest.fixture(scope="module")
def genomes(engine):
    rng = np.random.default_rng(21)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30000)].copy()
    seq[rng.integers(0, 30000, 3000)] = ord("N")
    seq[rng.integers(0, 30000, 500)] = ord("-")
    seq[12_000:12_400] = ord("N")
    g = {0: _oracle.HostGenome(_synth.synthetic_contigs([1_000_000], 1)),
         1: _oracle.HostGenome(_synth.synthetic_contigs([300_000, 90_001, 30_017, 70_000, 123_457], 7)),
         3: _oracle.HostGenome([seq])}
    engine.stage_synthetic(0, [1_000_000], 1)
    engine.stage_genome(1, g[1].contigs)
    engine.stage_genome(3, g[3].contigs)
    return g


@pytest.fixture(params=[0, 16], ids=["compact", "slot16"])
def layout(request, engine):
    engine.set_read_slots(request.param)
    try:
        yield request.param
    finally:
        engine.set_read_slots(0)


def device_truth(eng, reads):
    return eng.truth(reads).to_host()


def check(eng, oracle, genomes, dev, ora, what, counter=None):
    """the device reads are the oracle's; the device truth is the model of the oracle's reads"""
    o = ora.trimmed()
    assert_same(dev.to_host(), o, cols=("seq_off", "start", "end", "contig", "flags", "qual", "seq"))
    if "genome" not in o or not np.array_equal(o["genome"], dev.to_host()["genome"]):
        o = dict(o, genome=dev.to_host()["genome"])
    want = _truth.model(oracle, o, genomes)
    got = device_truth(eng, dev)
    _truth.assert_truth(got, want, what)
    assert np.array_equal(got["nm"], np.diff(got["edit_off"].astype(np.int64)).astype(np.uint32))
    if counter is not None:
        assert int(got["nm"].sum()) == int(counter), f"{what}: sum(nm) against SIMMR_CNT_SUBSTITUTIONS"
    return got


@pytest.mark.parametrize("rng_mode", RNG_MODES, ids=RNG_IDS)
def test_minimal_short_pairs(engine, oracle, genomes, layout, rng_mode):
    prof = MinimalShortErrorProfile(rng_mode=rng_mode).pod()
    for gidx, reads, seed, first, count in ((1, 3001, 5, 0, _abi.U64_MAX), (0, 8000, 42, 0, _abi.U64_MAX), (0, 8000, 42, 1100, 900)):
        engine.counters_reset()
        dev = engine.simulate_pe_reads_from_genome(gidx, prof, reads, seed, first=first, count=count, qual_offset=33)
        subs = engine.counters()[_abi.CNT_SUBSTITUTIONS]
        ora = _oracle.simulate_pe(oracle, genomes[gidx], prof, reads, seed, first=first, count=count, qual_offset=33)
        got = check(engine, oracle, genomes, dev, ora, f"genome {gidx} first {first}", subs)
        assert got["nm"].sum() > 0


def test_perfect_short_has_no_edits(engine, oracle, genomes, layout):
    prof = PerfectShortErrorProfile().pod()
    dev = engine.simulate_pe_reads_from_genome(1, prof, 3001, 5)
    assert engine.truth_plan(dev) == 0
    got = device_truth(engine, dev)
    assert not got["nm"].any() and not got["edit_off"].any() and got["edit_pos"].size == 0
    # every edit column NULL: only nm
    import torch
    nm = torch.full((dev.n_reads,), 7, dtype=torch.int32, device=engine.device)
    out = _abi.TruthOut(nm.data_ptr(), None, None, None, None, None, dev.n_reads, 0)
    pod = dev.pod()
    engine._check(engine.lib.simmr_truth_emit(engine._h, C.byref(pod), C.byref(out)))
    assert not nm.cpu().numpy().any()


@pytest.mark.parametrize("rng_mode", [_abi.RNG_REFERENCE, _abi.RNG_PHILOX], ids=["reference", "philox"])
def test_exception_bases_are_expected_as_themselves(engine, oracle, genomes, layout, rng_mode):
    prof = MinimalShortErrorProfile(mean_phred_score=8, rng_mode=rng_mode).pod()
    engine.counters_reset()
    dev = engine.simulate_pe_reads_from_genome(3, prof, 3000, 8)
    ora = _oracle.simulate_pe(oracle, genomes[3], prof, 3000, 8)
    got = check(engine, oracle, genomes, dev, ora, "N and - runs")
    assert got["edit_pos"].size > 1000
    assert not np.isin(got["edit_ref"], [ord("N"), ord("-")]).any()  # no edit at an exception base
    assert np.isin(got["edit_ref"], list(b"ACGT")).all() and np.isin(got["edit_alt"], list(b"ACGT")).all()


@pytest.mark.parametrize("cls", [MinimalLongErrorProfile, PerfectLongErrorProfile], ids=["minimal-long", "perfect-long"])
@pytest.mark.parametrize("rng_mode", [_abi.RNG_REFERENCE, _abi.RNG_PHILOX], ids=["reference", "philox"])
def test_long_reads_two_genomes(engine, oracle, genomes, layout, cls, rng_mode):
    lp = cls(gamma_mean=3000.0, gamma_std=2500.0, length_mode=_abi.LEN_PER_READ, rng_mode=rng_mode).pod()
    engine.counters_reset()
    dev = engine.simulate_long_reads([1, 0], [150, 100], lp, 3, qual_offset=33)
    subs = engine.counters()[_abi.CNT_SUBSTITUTIONS]
    ora = _oracle.simulate_long(oracle, [genomes[1], genomes[0]], [150, 100], lp, 3, qual_offset=33)
    got = check(engine, oracle, genomes, dev, ora, "long reads", subs)
    h = dev.to_host()
    L = np.abs(h["end"].astype(np.int64) - h["start"].astype(np.int64))
    assert L.max() > 4096 and set(np.unique(h["genome"])) == {0, 1}
    assert got["nm"].sum() == subs  # (perfect-long still draws substitutions, at Phred 20)


def test_long_reads_of_65535_bases(engine, oracle, genomes, layout):
    # a narrow Gamma law (shape 1e6) far above the u16 limit: every length saturates at 65 535
    lp = MinimalLongErrorProfile(gamma_mean=200000.0, gamma_std=200.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    engine.counters_reset()
    dev = engine.simulate_long_reads([0], [6], lp, 9, qual_offset=33)
    subs = engine.counters()[_abi.CNT_SUBSTITUTIONS]
    ora = _oracle.simulate_long(oracle, [genomes[0]], [6], lp, 9, qual_offset=33)
    h = dev.to_host()
    assert (np.abs(h["end"].astype(np.int64) - h["start"].astype(np.int64)) == 65535).all()
    check(engine, oracle, genomes, dev, ora, "65 535-base reads", subs)


def test_hand_built_columns(engine, oracle, genomes, layout):
    """The columns of tests/test_gpu_stats.py::test_hand_built_columns through the truth pass: lengths 0, 1, 15, 16, 17, 511,
    512, 513 on both strands, reverse mates right-aligned in their slots, a read that ends at its contig's end, a window
    inside an N run.  k_truth and k_read_stats walk a read with the same code, so both answer for these shapes, and
    they count the same edits."""
    dev, host = hand_built(oracle, genomes, layout, engine.device, np.random.default_rng(5))
    want = _truth.model(oracle, host, genomes)
    got = device_truth(engine, dev)
    _truth.assert_truth(got, want, "hand-built")
    assert np.array_equal(got["nm"], np.diff(got["edit_off"].astype(np.int64)).astype(np.uint32)) and got["nm"].max() == 75
    engine.stats_reset()
    engine.stats_add(dev, 1)
    assert int(got["nm"].sum()) == int(engine.stats()["qual_mismatch"].sum())


@pytest.mark.parametrize("rng_mode", [_abi.RNG_REFERENCE, _abi.RNG_PHILOX], ids=["reference", "philox"])
def test_custom_long_model_with_the_splice(engine, oracle, genomes, rng_mode):
    blob = _model.synthetic_long_model(kmer_size=6, n_positions=2500, seed=12, n_kmers=4 ** 6, lengths=(800, 3000, 100))
    prof = CustomShortErrorProfile(blob, rng_mode)
    pod = prof.pod()
    pod.length_mode = _abi.LEN_PER_READ
    dev = engine.simulate_long_reads([1, 0], [40, 30], pod, 4, qual_offset=33)
    ora = _oracle.simulate_long(oracle, [genomes[1], genomes[0]], [40, 30], pod, 4, qual_offset=33)
    got = check(engine, oracle, genomes, dev, ora, "custom long model")
    assert got["nm"].sum() > 0


def test_pe_plan_multi_honours_the_genome_column(engine, oracle, genomes, layout):
    prof = MinimalShortErrorProfile(mean_phred_score=8, rng_mode=_abi.RNG_PHILOX).pod()
    idx, reads = [1, 3, 0], [2000, 1001, 3000]
    engine.counters_reset()
    dev = engine.simulate_pe_reads_multi(idx, reads, prof, 17, qual_offset=33)
    subs = engine.counters()[_abi.CNT_SUBSTITUTIONS]
    # the oracle's per-genome runs with the run's seed, concatenated (simulate.rs:137,172: every genome re-creates the
    # outer generator; ids continue across genomes), as tests/test_gpu_blockloop.py::multi_plan builds them
    parts, base = [], 0
    for g, n in zip(idx, reads):
        p = _oracle.simulate_pe(oracle, genomes[g], prof, n, 17, read_id_base=base, qual_offset=33).trimmed()
        p["genome"][:] = g
        parts.append(p)
        base += n // 2
    o = {c: np.concatenate([p[c] for p in parts]) for c in ("start", "end", "contig", "genome", "read_id", "flags", "qual", "seq")}
    lens = np.concatenate([np.diff(p["seq_off"].astype(np.int64)) for p in parts])
    o["seq_off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert set(np.unique(o["genome"])) == {0, 1, 3}
    assert_same(dev.to_host(), o, cols=("seq_off", "start", "end", "contig", "genome", "read_id", "flags", "qual", "seq"))
    got = device_truth(engine, dev)
    _truth.assert_truth(got, _truth.model(oracle, o, genomes), "multi")
    assert int(got["nm"].sum()) == int(subs)


def test_edits_written_after_the_emit_are_found(engine, oracle, genomes, layout):
    """independence from the simulator: bytes overwritten in the device seq tensor come back as exactly those edits"""
    prof = PerfectShortErrorProfile().pod() if layout == 0 else MinimalShortErrorProfile(mean_phred_score=90, rng_mode=_abi.RNG_PHILOX).pod()
    dev = engine.simulate_pe_reads_from_genome(0, prof, 400, 11, qual_offset=33)
    assert dev.slot_bytes == layout
    base = device_truth(engine, dev)
    assert base["edit_pos"].size == 0, "choose a quieter profile: the base run must have no edits"
    raw = dev.raw_to_host()
    L = np.abs(raw["end"].astype(np.int64) - raw["start"].astype(np.int64))
    first = raw["seq_off"][:-1].astype(np.int64)
    qfirst = first & ~np.int64(15) if layout == 16 else first
    fwd, rev = 10, 11
    assert not raw["flags"][fwd] & 1 and raw["flags"][rev] & 1 and L[fwd] % 16 != 0
    # first and last base of a forward and of a reverse mate (next to the slot padding in SLOT16: a forward read's last
    # base sits before its padding, a reverse mate's first base behind it), and an N over an ACGT base
    places = [(fwd, 0), (fwd, int(L[fwd]) - 1), (rev, 0), (rev, int(L[rev]) - 1), (20, 77), (21, 16), (21, 15)]
    want = {}
    for r, j in places:
        at = int(first[r]) + j
        old = int(raw["seq"][at])
        new = ord("N") if (r, j) == (20, 77) else ord("ACGT"[("ACGT".index(chr(old)) + 1 + (j % 3)) % 4])
        dev.seq[at] = new
        want.setdefault(r, []).append((j, old, new, int(raw["qual"][int(qfirst[r]) + j])))
    got = device_truth(engine, dev)
    assert int(got["nm"].sum()) == len(places)
    for r in range(dev.n_reads):
        a, b = int(got["edit_off"][r]), int(got["edit_off"][r + 1])
        have = [(int(got["edit_pos"][i]), int(got["edit_ref"][i]), int(got["edit_alt"][i]), int(got["edit_qual"][i])) for i in range(a, b)]
        assert have == sorted(want.get(r, [])), f"read {r}"


def test_capacities_and_call_order(engine, genomes):
    import torch
    from simmr_amd.engine import Engine
    prof = MinimalShortErrorProfile(mean_phred_score=12, rng_mode=_abi.RNG_PHILOX).pod()
    dev = engine.simulate_pe_reads_from_genome(1, prof, 2000, 3, qual_offset=33)
    n = dev.n_reads
    lib, h = engine.lib, engine._h
    pod = dev.pod()
    # emit before a plan for these columns
    fresh = Engine(0)
    try:
        out0 = _abi.TruthOut(None, None, None, None, None, None, 0, 0)
        assert fresh.lib.simmr_truth_emit(fresh._h, C.byref(pod), C.byref(out0)) == _abi.ESTATE
    finally:
        fresh.close()
    m = engine.truth_plan(dev)
    assert m > 100
    ref = engine.truth(dev).to_host()
    assert engine.truth_plan(dev) == m
    CAN = 64
    bufs = {name: torch.full((CAN + cnt + CAN,), fill, dtype=dt, device=engine.device)
            for name, cnt, dt, fill in (("nm", n, torch.int32, -3), ("edit_off", n + 1, torch.int64, -5), ("edit_pos", m, torch.int32, -7),
                                        ("edit_ref", m, torch.uint8, 0xA5), ("edit_alt", m, torch.uint8, 0xA6), ("edit_qual", m, torch.uint8, 0xA7))}
    before = {k: v.clone() for k, v in bufs.items()}
    ptr = lambda k: bufs[k].data_ptr() + CAN * bufs[k].element_size()
    make = lambda cap_r, cap_e: _abi.TruthOut(ptr("nm"), ptr("edit_off"), ptr("edit_pos"), ptr("edit_ref"), ptr("edit_alt"), ptr("edit_qual"), cap_r, cap_e)
    for cap_r, cap_e in ((n, m - 1), (n - 1, m)):
        out = make(cap_r, cap_e)
        assert lib.simmr_truth_emit(h, C.byref(pod), C.byref(out)) == _abi.ERANGE
        torch.cuda.synchronize()
        for k in bufs:
            assert torch.equal(bufs[k], before[k]), f"{k} was written by a refused emit"
    out = make(n, m)
    engine._check(lib.simmr_truth_emit(h, C.byref(pod), C.byref(out)))
    torch.cuda.synchronize()
    for k, cnt in (("nm", n), ("edit_off", n + 1), ("edit_pos", m), ("edit_ref", m), ("edit_alt", m), ("edit_qual", m)):
        t = bufs[k]
        assert torch.equal(t[:CAN], before[k][:CAN]) and torch.equal(t[CAN + cnt:], before[k][CAN + cnt:]), f"{k}: canary"
        assert np.array_equal(t[CAN:CAN + cnt].cpu().numpy().astype(ref[k].dtype), ref[k]), k
    # edit columns without edit_off
    bad = make(n, m); bad.edit_off = None
    assert lib.simmr_truth_emit(h, C.byref(pod), C.byref(bad)) == _abi.EINVAL
    # a NULL start
    total = C.c_uint64(0)
    nostart = dev.pod(); nostart.start = None
    assert lib.simmr_truth_plan(h, C.byref(nostart), n, C.byref(total)) == _abi.EINVAL
    # a contig entry out of range: the device bounds check answers through the error word
    keep = int(dev.contig[5])
    dev.contig[5] = 5
    try:
        assert lib.simmr_truth_plan(h, C.byref(pod), n, C.byref(total)) == _abi.EINVAL
        assert b"not staged" in lib.simmr_last_error(h)
        dev.genome[5] = 77
        assert lib.simmr_truth_plan(h, C.byref(pod), n, C.byref(total)) == _abi.EINVAL
    finally:
        dev.contig[5] = keep
        dev.genome[5] = 1
    assert engine.truth_plan(dev) == m
    # staging a genome discards the plan: the counts were taken against what is being replaced
    engine.stage_genome(3, genomes[3].contigs)
    out = make(n, m)
    assert lib.simmr_truth_emit(h, C.byref(pod), C.byref(out)) == _abi.ESTATE
    assert engine.truth_plan(dev) == m


def test_seq_past_4_gib_and_workgroups_loop(engine, oracle):
    """One SLOT16 run whose seq[] passes 4 GiB: sum(nm) is the emit's own counter, and a fixed sample of reads from the first
    and the last gigabyte has the model's edits."""
    import torch
    n_reads = 30_000_000
    engine.stage_synthetic(5, [100_000_000], 2)
    host = _oracle.HostGenome(_synth.synthetic_contigs([100_000_000], 2))
    prof = MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX_FULL).pod()
    engine.set_read_slots(16)
    try:
        engine.counters_reset()
        dev = engine.simulate_pe_reads_from_genome(5, prof, n_reads, 42, qual_offset=33)
    finally:
        engine.set_read_slots(0)
    subs = int(engine.counters()[_abi.CNT_SUBSTITUTIONS])
    n, tb = dev.n_reads, dev.total_bases
    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert tb > 1 << 32 and -(-n // TRUTH_WG_READS) > 3 * n_cu * TRUTH_WGS_PER_CU, "resize: seq[] must pass 4 GiB and workgroups must loop"
    t = engine.truth(dev)
    assert int(t.nm[:n].sum(dtype=torch.int64)) == subs == t.n_edits == int(t.edit_off[n])
    first = dev.seq_off[: n + 1]
    rng = np.random.default_rng(2024)
    lo_max = int(torch.searchsorted(first, 1 << 30))
    hi_min = int(torch.searchsorted(first, tb - (1 << 30)))
    assert int(first[n - 1]) > 1 << 32  # (the last gigabyte straddles 4 GiB: the sample below has reads on both sides, the last read among them)
    sample = np.sort(np.concatenate([rng.integers(0, lo_max, 300), rng.integers(hi_min, n, 300), [0, n - 1]]))
    for r in np.unique(sample):
        r = int(r)
        a, b = int(dev.start[r]), int(dev.end[r])
        L, rev = abs(b - a), bool(int(dev.flags[r]) & 1)
        so = int(first[r])
        cols = {"seq": dev.seq[so:so + L].cpu().numpy(), "qual": dev.qual[(so & ~15):(so & ~15) + L].cpu().numpy(),
                "seq_off": np.array([0, L], dtype=np.uint64), "start": np.array([a], dtype=np.uint64), "end": np.array([b], dtype=np.uint64),
                "contig": np.zeros(1, dtype=np.uint32), "genome": np.full(1, 5, dtype=np.uint32),
                "flags": np.array([1 if rev else 0], dtype=np.uint8)}
        want = _truth.model(oracle, cols, {5: host})
        ea, eb = int(t.edit_off[r]), int(t.edit_off[r + 1])
        assert int(t.nm[r]) == eb - ea == int(want["nm"][0]), f"read {r}"
        for col in ("edit_pos", "edit_ref", "edit_alt", "edit_qual"):
            assert np.array_equal(getattr(t, col)[ea:eb].cpu().numpy().astype(want[col].dtype), want[col]), f"read {r}: {col}"
