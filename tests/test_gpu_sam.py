"""The SAM text of the device (simmr_sam_plan / simmr_sam_emit, include/simmr_hip.h) against the plain-Python record of
tests/_sam.py over the host copies of the same columns and the numpy truth model (tests/_truth.py): byte for byte."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import MinimalLongErrorProfile, MinimalShortErrorProfile, PerfectShortErrorProfile, _abi
from simmr_amd.engine import Reads
from tests import _oracle, _sam, _synth, _truth
from tests._hand_built import hand_built

pytestmark = pytest.mark.gpu

# sam_kernels.hip: SAM_WG_READS reads per workgroup and iteration, at most SAM_WGS_PER_CU workgroups per CU
_KERNELS = (Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc" / "sam_kernels.hip").read_text()
_DEFINES = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(SAM_\w+)\s+(\d+)u?\b", _KERNELS, re.M)}
SAM_WG_READS = _DEFINES["SAM_WG_READS"]
SAM_WGS_PER_CU = _DEFINES["SAM_WGS_PER_CU"]


@pytest.fixture(scope="module")
def genomes(engine):
    rng = np.random.default_rng(21)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30000)].copy()
    seq[rng.integers(0, 30000, 3000)] = ord("N")
    seq[rng.integers(0, 30000, 500)] = ord("-")
    seq[12_000:12_400] = ord("N")
    g = {0: _oracle.HostGenome(_synth.synthetic_contigs([1_000_000], 1)),
         1: _oracle.HostGenome(_synth.synthetic_contigs([300_000, 90_001, 30_017, 70_000, 123_457], 7)),
         3: _oracle.HostGenome([seq]),
         4: _oracle.HostGenome(_synth.synthetic_contigs([700, 520, 900], 9))}
    engine.stage_synthetic(0, [1_000_000], 1)
    for slot in (1, 3, 4):
        engine.stage_genome(slot, g[slot].contigs)
    return g


@pytest.fixture(params=[0, 16], ids=["compact", "slot16"])
def layout(request, engine):
    engine.set_read_slots(request.param)
    try:
        yield request.param
    finally:
        engine.set_read_slots(0)


def names_of(genomes):
    return {(g, c): f"g{g}.c{c}|x" for g in genomes for c in range(len(genomes[g].contigs))}


def rnames_of(genomes, names=None):
    names = names or names_of(genomes)
    return [(g, [names[(g, c)] for c in range(len(genomes[g].contigs))]) for g in sorted(genomes)]


def expected(oracle, genomes, o, paired):
    t = _truth.model(oracle, o, genomes)
    return _sam.sam_text(o, t, names_of(genomes), paired), t


def same_text(got, want, what=""):
    got = bytes(got.cpu().numpy())
    if got != want:
        gl, wl = got.split(b"\n"), want.split(b"\n")
        i = next((k for k in range(min(len(gl), len(wl))) if gl[k] != wl[k]), min(len(gl), len(wl)))
        raise AssertionError(f"{what}: {len(got)} bytes against {len(want)}; line {i} differs:\n{gl[i:i + 1]}\n{wl[i:i + 1]}")


def check(engine, oracle, genomes, dev, paired, what):
    want, t = expected(oracle, genomes, dev.to_host(), paired)
    same_text(engine.sam(dev, rnames_of(genomes), paired), want, what)
    return want, t


def build(genomes, oracle, specs, layout, device, seed=1):
    """Reads copied from the host genomes with chosen offsets altered — specs of (genome, contig, lo, L, reverse, offsets) —
    as device columns in `layout`, mates sharing a read id."""
    import torch
    comp = _truth.complement_lut(oracle)
    rng = np.random.default_rng(seed)
    seqs, quals = [], []
    for g, c, lo, L, rev, alter in specs:
        want = genomes[g].contigs[c][lo:lo + L].copy()
        assert want.size == L
        if rev:
            want = comp[want[::-1]]
        for j in alter:
            want[j] = ord("ACGT"[("ACGT".find(chr(want[j])) + 1 + j % 3) % 4])
        seqs.append(want)
        quals.append((33 + rng.integers(0, 61, L)).astype(np.uint8))
    n = len(specs)
    L = np.array([s[3] for s in specs], dtype=np.int64)
    lo = np.array([s[2] for s in specs], dtype=np.int64)
    rev = np.array([s[4] for s in specs], dtype=np.uint8)
    slot = (L + 15) // 16 * 16 if layout == 16 else L
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(slot, out=first[1:])
    seq, qual = np.zeros(int(first[n]), dtype=np.uint8), np.zeros(int(first[n]), dtype=np.uint8)
    seq_off = first.copy()
    seq_off[:n] += np.where(rev == 1, slot - L, 0)  # reverse mates right-aligned
    for r in range(n):
        seq[seq_off[r]:seq_off[r] + L[r]] = seqs[r]
        qual[first[r]:first[r] + L[r]] = quals[r]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(device)
    return Reads(seq=t(seq, np.uint8), qual=t(qual, np.uint8), seq_off=t(seq_off, np.int64), start=t(np.where(rev == 1, lo + L, lo), np.int64),
                 end=t(np.where(rev == 1, lo, lo + L), np.int64), contig=t([s[1] for s in specs], np.int32), genome=t([s[0] for s in specs], np.int32),
                 read_id=t(np.arange(n) // 2 + 4_000_000_000, np.int64).to(torch.int32), flags=t(rev, np.uint8), n_reads=n,
                 total_bases=int(first[n]), qual_offset=33, slot_bytes=layout)


@pytest.mark.parametrize("rng_mode,slots", [(_abi.RNG_PHILOX, 16), (_abi.RNG_PHILOX, 0), (_abi.RNG_REFERENCE, 0)],
                         ids=["philox-slot16", "philox-compact", "reference-compact"])
def test_minimal_short_pairs(engine, oracle, genomes, rng_mode, slots):
    engine.set_read_slots(slots)
    try:
        dev = engine.simulate_pe_reads_from_genome(1, MinimalShortErrorProfile(rng_mode=rng_mode).pod(), 3000, 5, qual_offset=33)
    finally:
        engine.set_read_slots(0)
    assert dev.slot_bytes == slots
    want, t = check(engine, oracle, genomes, dev, True, "minimal-short")
    assert t["nm"].sum() > 0 and engine.last_sam_ms() > 0


def test_read_lengths_at_the_window_edges(engine, oracle, genomes, layout):
    """1, 15, 16, 17 and 33 bases on both strands (and 0, 31, 32), with edits at the first and the last base: in slots the
    reverse mates are right-aligned"""
    specs = []
    for i, L in enumerate((1, 15, 16, 17, 33, 0, 31, 32, 48)):
        ends = sorted({0, L - 1}) if L else []
        specs.append((1, i % 5, 100 + 31 * i, L, 0, ends))
        specs.append((1, i % 5, 160 + 31 * i, L, 1, ends))
        specs.append((3, 0, 11_990 + i, L, 1, []))      # runs into the N run: no edit, N in SEQ
        specs.append((3, 0, 11_990 + i, L, 0, []))
    dev = build(genomes, oracle, specs, layout, engine.device)
    for paired in (True, False):
        check(engine, oracle, genomes, dev, paired, f"edges paired={paired}")
    # the shapes of the truth and statistics tests as well: 511, 512, 513, 73 and 75 edits, reads at a contig's end
    dev, host = hand_built(oracle, genomes, layout, engine.device, np.random.default_rng(5))
    want, _ = expected(oracle, genomes, host, False)
    same_text(engine.sam(dev, rnames_of(genomes), False), want, "hand-built")


def test_perfect_short(engine, oracle, genomes, layout):
    dev = engine.simulate_pe_reads_from_genome(1, PerfectShortErrorProfile().pod(), 2000, 5, qual_offset=33)
    want, t = check(engine, oracle, genomes, dev, True, "perfect-short")
    assert not t["nm"].any()
    for line in want.decode().splitlines():
        f = _sam.parse(line)
        assert f["nm"] == 0 and f["md"] == str(len(f["seq"])) == f["cigar"][:-1]


def test_low_quality_reads_have_every_kind_of_edit(engine, oracle, genomes, layout):
    dev = engine.simulate_pe_reads_from_genome(1, MinimalShortErrorProfile(mean_phred_score=3, rng_mode=_abi.RNG_PHILOX).pod(), 600, 8, qual_offset=33)
    want, t = check(engine, oracle, genomes, dev, True, "phred 3")
    o = dev.to_host()
    L = np.abs(o["end"].astype(np.int64) - o["start"].astype(np.int64))
    seen = {(k, rev): False for k in ("first", "last", "adjacent") for rev in (0, 1)}
    for r in range(dev.n_reads):
        p = t["edit_pos"][int(t["edit_off"][r]):int(t["edit_off"][r + 1])].astype(np.int64)
        rev = int(o["flags"][r]) & 1
        seen[("first", rev)] |= bool(p.size and p[0] == 0)
        seen[("last", rev)] |= bool(p.size and p[-1] == L[r] - 1)
        seen[("adjacent", rev)] |= bool((np.diff(p) == 1).any())
    assert all(seen.values()), seen
    assert b"\tMD:Z:0" in want


def test_genome_with_n_and_dash(engine, oracle, genomes, layout):
    dev = engine.simulate_pe_reads_from_genome(3, MinimalShortErrorProfile(mean_phred_score=8, rng_mode=_abi.RNG_PHILOX).pod(), 2000, 8, qual_offset=33)
    want, _ = check(engine, oracle, genomes, dev, True, "N and -")
    o = dev.to_host()
    assert (o["seq"] == ord("-")).any() and (o["seq"] == ord("N")).any()
    shown = bytes(genomes[3].contigs[0]).decode().replace("-", "N")
    for line in want.decode().splitlines():
        f = _sam.parse(line)
        assert set(f["seq"]) <= set("ACGTN") and _sam.reference_from(f["seq"], f["md"]) == shown[f["pos"] - 1: f["pos"] - 1 + len(f["seq"])]


def test_decimal_widths_of_pos_pnext_and_tlen(engine, oracle, genomes):
    specs = []
    for lo, gap in ((0, 3), (4, 1), (42, 60), (512, 900), (7_000, 9_000), (20_000, 30_000), (65_000, 99_990), (100_001, 899_000), (999_960, 0)):
        specs.append((0, 0, lo, 20, 0, [3]))
        specs.append((0, 0, min(lo + gap, 999_980), 20, 1, [7]))
    specs = [(0, 0, 300, 5, 0, [1]), (0, 0, 302, 6, 1, [0]),   # short overlapping mates: a TLEN of one digit
             (0, 0, 77, 0, 0, []), (0, 0, 77, 0, 1, [])] + specs  # and mates without bases at one place: TLEN 0 for both
    dev = build(genomes, oracle, specs, 0, engine.device)
    want, _ = check(engine, oracle, genomes, dev, True, "widths")
    recs = [_sam.parse(l) for l in want.decode().splitlines()]
    for key in ("pos", "pnext", "tlen"):
        assert {len(str(abs(f[key]))) for f in recs} >= set(range(1, 7)), key
    assert (recs[0]["tlen"], recs[1]["tlen"], recs[2]["tlen"], recs[3]["tlen"]) == (8, -8, 0, 0)
    assert any(f["tlen"] < 0 for f in recs) and recs[-1]["tlen"] == -20 and recs[-2]["tlen"] == 20  # a tie: mate 1 is positive
    assert all(len(f["qname"]) == 10 for f in recs)


def test_redrawn_mates(engine, oracle, genomes, layout):
    dev = engine.simulate_pe_reads_from_genome(4, MinimalShortErrorProfile(rng_mode=_abi.RNG_PHILOX).pod(), 2000, 6, qual_offset=33)
    assert (dev.to_host()["flags"] & _abi.FLAG_REDRAWN).any()
    check(engine, oracle, genomes, dev, True, "re-drawn")


def test_long_reads(engine, oracle, genomes, layout):
    lp = MinimalLongErrorProfile(gamma_mean=3000.0, gamma_std=2500.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    dev = engine.simulate_long_reads([1, 0], [60, 40], lp, 3, qual_offset=33)
    o = dev.to_host()
    assert np.abs(o["end"].astype(np.int64) - o["start"].astype(np.int64)).max() > 4096
    check(engine, oracle, genomes, dev, False, "minimal-long")
    # lengths on both sides of 255 / 256, 999 / 1000 and 4096: the decimal width of CIGAR and MD, the rounds of the row
    specs = []
    for i, L in enumerate((255, 256, 257, 999, 1000, 4095, 4096, 4097)):
        for rev in (0, 1):
            specs.append((1, 0, 1000 + 5000 * i, L, rev, sorted({0, 1, L // 2, L - 2, L - 1} | set(range(5, L, 3 if L < 1000 else 97)))))
    dev = build(genomes, oracle, specs, layout, engine.device)
    check(engine, oracle, genomes, dev, False, "length edges")


def test_more_reads_than_one_pass_of_the_grid(engine, oracle, genomes):
    import torch
    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    one_pass = n_cu * SAM_WGS_PER_CU * SAM_WG_READS
    specs = []
    for i in range(one_pass // 2 + 700):
        L = 17 + i % 5
        specs.append((0, 0, 13 * i, L, 0, [i % L] if i % 3 else []))
        specs.append((0, 0, 13 * i + 9, L, 1, [0] if i % 4 == 0 else []))
    assert len(specs) > one_pass + 1024
    dev = build(genomes, oracle, specs, 0, engine.device)
    check(engine, oracle, genomes, dev, True, "workgroups loop")


def plan_and_emit(engine, dev, truth, rnames, paired, dst=None, capacity=None):
    """the raw calls: (plan status, total, emit status or None)"""
    out = _abi.TruthOut(truth.nm.data_ptr(), truth.edit_off.data_ptr(), truth.edit_pos.data_ptr(), truth.edit_ref.data_ptr(),
                        truth.edit_alt.data_ptr(), truth.edit_qual.data_ptr(), truth.n_reads, truth.n_edits)
    sn, pod, total = engine._sam_names(rnames), dev.pod(), C.c_uint64(0)
    rc = engine.lib.simmr_sam_plan(engine._h, C.byref(sn), C.byref(pod), C.byref(out), dev.n_reads, 1 if paired else 0, C.byref(total))
    if rc != 0 or dst is None:
        return rc, total.value, None
    cap = total.value if capacity is None else capacity
    return rc, total.value, engine.lib.simmr_sam_emit(engine._h, C.byref(pod), C.byref(out), C.c_void_p(dst), cap)


def test_exact_capacity_canaries_determinism_and_refusals(engine, oracle, genomes):
    import torch
    from simmr_amd.engine import Engine
    dev = engine.simulate_pe_reads_from_genome(1, MinimalShortErrorProfile(mean_phred_score=12, rng_mode=_abi.RNG_PHILOX).pod(), 2000, 3, qual_offset=33)
    rn = rnames_of(genomes)
    want, _ = expected(oracle, genomes, dev.to_host(), True)
    truth = engine.truth(dev)
    CAN = 256
    buf = torch.full((CAN + len(want) + CAN,), 0xA5, dtype=torch.uint8, device=engine.device)
    clean = buf.clone()
    dst = buf.data_ptr() + CAN
    # ERANGE: one byte short, nothing written
    assert plan_and_emit(engine, dev, truth, rn, True, dst, len(want) - 1) == (0, len(want), _abi.ERANGE)
    torch.cuda.synchronize()
    assert torch.equal(buf, clean)
    # exactly total_bytes between canaries, twice: the same bytes
    for _ in range(2):
        buf.copy_(clean)
        assert plan_and_emit(engine, dev, truth, rn, True, dst) == (0, len(want), 0)
        torch.cuda.synchronize()
        assert torch.equal(buf[:CAN], clean[:CAN]) and torch.equal(buf[CAN + len(want):], clean[CAN + len(want):])
        same_text(buf[CAN:CAN + len(want)], want, "between canaries")
    buf.copy_(clean)
    lib, pod = engine.lib, dev.pod()
    out = _abi.TruthOut(truth.nm.data_ptr(), truth.edit_off.data_ptr(), truth.edit_pos.data_ptr(), truth.edit_ref.data_ptr(),
                        truth.edit_alt.data_ptr(), truth.edit_qual.data_ptr(), truth.n_reads, truth.n_edits)
    # ESTATE: an engine without a plan; other columns than the plan's; after a staging call
    fresh = Engine(0)
    try:
        assert fresh.lib.simmr_sam_emit(fresh._h, C.byref(pod), C.byref(out), C.c_void_p(dst), len(want)) == _abi.ESTATE
    finally:
        fresh.close()
    for field, value in (("seq", dev.qual.data_ptr()), ("start", dev.end.data_ptr()), ("flags", dev.qual.data_ptr()),
                         ("seq_capacity", dev.seq.numel() + 1)):
        other = dev.pod(); setattr(other, field, value)
        assert lib.simmr_sam_emit(engine._h, C.byref(other), C.byref(out), C.c_void_p(dst), len(want)) == _abi.ESTATE, field
    more = _abi.TruthOut(truth.nm.data_ptr(), truth.edit_off.data_ptr(), truth.edit_pos.data_ptr(), truth.edit_ref.data_ptr(),
                         truth.edit_alt.data_ptr(), truth.edit_qual.data_ptr(), truth.n_reads, truth.n_edits + 1)
    assert lib.simmr_sam_emit(engine._h, C.byref(pod), C.byref(more), C.c_void_p(dst), len(want)) == _abi.ESTATE
    engine.stage_genome(4, genomes[4].contigs)
    assert lib.simmr_sam_emit(engine._h, C.byref(pod), C.byref(out), C.c_void_p(dst), len(want)) == _abi.ESTATE
    # EINVAL at once: a missing column, qualities without the offset, an odd number of mates, a slot that is not staged
    total, sn = C.c_uint64(0), engine._sam_names(rn)
    noid = dev.pod(); noid.read_id = None
    raw = dev.pod(); raw.qual_offset = 0
    noref = _abi.TruthOut(truth.nm.data_ptr(), truth.edit_off.data_ptr(), truth.edit_pos.data_ptr(), None, None, None, truth.n_reads, truth.n_edits)
    assert lib.simmr_sam_plan(engine._h, C.byref(sn), C.byref(noid), C.byref(out), dev.n_reads, 1, C.byref(total)) == _abi.EINVAL
    assert lib.simmr_sam_plan(engine._h, C.byref(sn), C.byref(raw), C.byref(out), dev.n_reads, 1, C.byref(total)) == _abi.EINVAL
    assert lib.simmr_sam_plan(engine._h, C.byref(sn), C.byref(pod), C.byref(noref), dev.n_reads, 1, C.byref(total)) == _abi.EINVAL
    assert lib.simmr_sam_plan(engine._h, C.byref(sn), C.byref(pod), C.byref(out), dev.n_reads - 1, 1, C.byref(total)) == _abi.EINVAL
    assert plan_and_emit(engine, dev, truth, rn + [(2, ["x"])], True)[0] == _abi.EINVAL
    # ENOTSUP: an RNAME with a space, an empty one, one of 255 bytes
    for bad in ("has space", "", "x" * 255, "=lead"):
        names = names_of(genomes); names[(1, 2)] = bad
        assert plan_and_emit(engine, dev, truth, rnames_of(genomes, names), True)[0] == _abi.ENOTSUP, bad
    # EINVAL through the error word: the bounds check comes before any load or store that the tampered value would address
    e_at = int(truth.edit_off[7])
    assert int(truth.edit_off[8]) > e_at  # (read 7 has an edit)
    for col, at, value in ((dev.contig, 5, 5), (dev.genome, 5, 2), (dev.genome, 5, 77), (truth.edit_off, 9, 1 << 40), (truth.edit_off, 9, 0),
                           (truth.edit_pos, e_at, 70_000), (dev.seq_off, 11, 1 << 40), (dev.start, 13, 1 << 20)):
        keep = int(col[at])
        col[at] = value
        try:
            assert plan_and_emit(engine, dev, truth, rn, True, dst) == (_abi.EINVAL, 0, None), (at, value)
            assert lib.simmr_sam_emit(engine._h, C.byref(pod), C.byref(out), C.c_void_p(dst), len(want)) == _abi.ESTATE
        finally:
            col[at] = keep
    torch.cuda.synchronize()
    assert torch.equal(buf, clean)  # no refusal stored a byte
    # edits of a read that do not ascend
    a = int(truth.edit_off[:dev.n_reads + 1].diff().argmax())
    e0 = int(truth.edit_off[a])
    assert int(truth.edit_off[a + 1]) - e0 >= 2
    keep = int(truth.edit_pos[e0 + 1])
    truth.edit_pos[e0 + 1] = int(truth.edit_pos[e0])
    try:
        assert plan_and_emit(engine, dev, truth, rn, True, dst)[0] == _abi.EINVAL
    finally:
        truth.edit_pos[e0 + 1] = keep
    # columns tampered with BETWEEN the plan and the emit: the read is refused again, and no store leaves a record
    assert plan_and_emit(engine, dev, truth, rn, True)[:2] == (0, len(want))
    keep = int(dev.contig[5])
    dev.contig[5] = 5
    try:
        assert lib.simmr_sam_emit(engine._h, C.byref(pod), C.byref(out), C.c_void_p(dst), len(want)) == _abi.EINVAL
    finally:
        dev.contig[5] = keep
    torch.cuda.synchronize()
    assert torch.equal(buf[:CAN], clean[:CAN]) and torch.equal(buf[CAN + len(want):], clean[CAN + len(want):])
    lines = want.split(b"\n")
    at5 = sum(len(l) + 1 for l in lines[:5])
    got = bytes(buf[CAN:CAN + len(want)].cpu().numpy())
    assert got[:at5] == want[:at5] and got[at5 + len(lines[5]) + 1:] == want[at5 + len(lines[5]) + 1:]
    assert got[at5:at5 + len(lines[5]) + 1] == b"\xa5" * (len(lines[5]) + 1)  # the refused read's record was left alone
    # an edit_pos changed between the plan and the emit is found while the MD is written: that record is unspecified, every other
    # record and the canaries are as they should be
    buf.copy_(clean)
    assert plan_and_emit(engine, dev, truth, rn, True)[:2] == (0, len(want))
    keep = int(truth.edit_pos[e_at])
    truth.edit_pos[e_at] = 70_000
    try:
        assert lib.simmr_sam_emit(engine._h, C.byref(pod), C.byref(out), C.c_void_p(dst), len(want)) == _abi.EINVAL
    finally:
        truth.edit_pos[e_at] = keep
    torch.cuda.synchronize()
    assert torch.equal(buf[:CAN], clean[:CAN]) and torch.equal(buf[CAN + len(want):], clean[CAN + len(want):])
    at7 = sum(len(l) + 1 for l in lines[:7])
    got = bytes(buf[CAN:CAN + len(want)].cpu().numpy())
    assert got[:at7] == want[:at7] and got[at7 + len(lines[7]) + 1:] == want[at7 + len(lines[7]) + 1:]
    # and everything is as before
    buf.copy_(clean)
    assert plan_and_emit(engine, dev, truth, rn, True, dst) == (0, len(want), 0)
    same_text(buf[CAN:CAN + len(want)], want, "after the refusals")
