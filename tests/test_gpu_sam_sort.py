"""The coordinate-sorted SAM text of the device (simmr_sam_sort_plan / simmr_sam_sort_emit, include/simmr_hip.h) against the
plain-Python model of tests/_sam_sort.py: the text byte for byte, and the key and the offset of every line.  Hand-built reads
carry hand-built truth columns (the SAM pass reads the columns, never the genome), so a shape costs what its reads cost."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import MinimalLongErrorProfile, MinimalShortErrorProfile, _abi
from simmr_amd.engine import Engine, Reads, Truth
from tests import _oracle, _sam, _sam_sort, _synth, _truth

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def _defines(name, prefix):
    return {m.group(1): int(m.group(2)) for m in re.finditer(rf"^#define\s+({prefix}\w+)\s+(\d+)u?\b", (CSRC / name).read_text(), re.M)}


T = _defines("sam_sort_kernels.hip", "SAMSORT_")["SAMSORT_TILE"]
DIGIT = _defines("sam_sort_kernels.hip", "SAMSORT_")["SAMSORT_DIGIT_BITS"]
SAM = _defines("sam_kernels.hip", "SAM_")
BIG = 20_000_000
SLOTS = {0: [1_000_000], 1: [300_000, 90_001, 30_017, 70_000, 123_457], 2: [BIG], 3: [400 + 3 * i for i in range(300)]}


@pytest.fixture(scope="module")
def eng():
    """an engine of this module's own: four slots staged once (0: one contig, 1: five, 2: one of 20 M bases, 3: 300 short ones)"""
    e = Engine(0)
    for slot, lens in SLOTS.items():
        e.stage_synthetic(slot, lens, 10 + slot)
    yield e
    e.close()


@pytest.fixture(scope="module")
def host_genomes():
    """host copies of the slots simulated reads are drawn from (the truth model compares against them)"""
    return {s: _oracle.HostGenome(_synth.synthetic_contigs(SLOTS[s], 10 + s)) for s in (0, 1)}


def rnames(slots=(0, 1, 2, 3)):
    return [(s, [f"g{s}.c{c}|x" for c in range(len(SLOTS[s]))]) for s in slots]


@pytest.fixture(params=[0, 16], ids=["compact", "slot16"])
def layout(request):
    return request.param


def build(specs, layout, device, seed=1):
    """Reads and their truth columns from specs of (genome, contig, lo, L, reverse, edit offsets): random bases and qualities,
    edits at the given offsets of the read as written (ascending) with a random reference base; mates share a read id.
    Returns (Reads, Truth, host columns, host truth)."""
    import torch
    rng = np.random.default_rng(seed)
    n = len(specs)
    g = np.array([s[0] for s in specs], dtype=np.int64).reshape(n)
    c = np.array([s[1] for s in specs], dtype=np.int64).reshape(n)
    lo = np.array([s[2] for s in specs], dtype=np.int64).reshape(n)
    L = np.array([s[3] for s in specs], dtype=np.int64).reshape(n)
    rev = np.array([s[4] for s in specs], dtype=np.uint8).reshape(n)
    csr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(L, out=csr[1:])
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(csr[n]))]
    quals = (33 + rng.integers(0, 61, int(csr[n]))).astype(np.uint8)
    slot = (L + 15) // 16 * 16 if layout == 16 else L
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(slot, out=first[1:])
    seq_off = first.copy()
    seq_off[:n] += np.where(rev == 1, slot - L, 0)  # reverse mates right-aligned
    within = np.arange(int(csr[n]), dtype=np.int64) - np.repeat(csr[:n], L)
    seq, qual = np.zeros(int(first[n]), dtype=np.uint8), np.zeros(int(first[n]), dtype=np.uint8)
    seq[np.repeat(seq_off[:n], L) + within] = bases
    qual[np.repeat(first[:n], L) + within] = quals
    edits = [sorted(s[5]) for s in specs]
    eoff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.array([len(e) for e in edits], dtype=np.int64), out=eoff[1:])
    epos = np.array([p for e in edits for p in e], dtype=np.int64)
    eref = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, epos.size)]
    start, end = np.where(rev == 1, lo + L, lo), np.where(rev == 1, lo, lo + L)
    rid = np.arange(n) // 2 + 4_000_000_000
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(device)
    pad = lambda a: np.concatenate([a, np.zeros(1, a.dtype)])  # (no tensor without an element)
    reads = Reads(seq=t(pad(seq), np.uint8), qual=t(pad(qual), np.uint8), seq_off=t(seq_off, np.int64), start=t(pad(start), np.int64),
                  end=t(pad(end), np.int64), contig=t(pad(c), np.int32), genome=t(pad(g), np.int32), read_id=t(pad(rid), np.int64).to(torch.int32),
                  flags=t(pad(rev), np.uint8), n_reads=n, total_bases=int(first[n]), qual_offset=33, slot_bytes=layout)
    m = int(eoff[n])
    truth = Truth(nm=t(pad(np.diff(eoff)), np.int32), edit_off=t(eoff, np.int64), edit_pos=t(pad(epos), np.int32), edit_ref=t(pad(eref), np.uint8),
                  edit_alt=t(pad(eref), np.uint8), edit_qual=t(pad(eref), np.uint8), n_reads=n, n_edits=m)
    o = {"start": start.astype(np.uint64), "end": end.astype(np.uint64), "contig": c.astype(np.uint32), "genome": g.astype(np.uint32),
         "read_id": rid.astype(np.uint32), "flags": rev, "seq_off": csr.astype(np.uint64), "seq": bases, "qual": quals}
    ht = {"edit_off": eoff.astype(np.uint64), "edit_pos": epos.astype(np.uint32), "edit_ref": eref}
    return reads, truth, o, ht


def same(got, want, what):
    text, key, line_off = got
    wtext, wkey, woff = want
    got_text = bytes(text.cpu().numpy())
    if got_text != wtext:
        gl, wl = got_text.split(b"\n"), wtext.split(b"\n")
        i = next((k for k in range(min(len(gl), len(wl))) if gl[k] != wl[k]), min(len(gl), len(wl)))
        raise AssertionError(f"{what}: {len(got_text)} bytes against {len(wtext)}; line {i} differs:\n{gl[i:i + 1]}\n{wl[i:i + 1]}")
    assert np.array_equal(key.cpu().numpy(), wkey), what + ": key"
    assert np.array_equal(line_off.cpu().numpy(), woff), what + ": line_off"


def check(eng, specs, layout, paired, what, rn=None, seed=1):
    rn = rn or rnames()
    reads, truth, o, ht = build(specs, layout, eng.device, seed)
    want = _sam_sort.sorted_text(o, ht, rn, paired)
    same(eng.sam_sorted(reads, rn, paired, truth=truth, with_keys=True), want, what)
    assert bytes(eng.sam_sorted(reads, rn, paired, truth=truth).cpu().numpy()) == want[0]  # without the key arrays
    return reads, truth, o, ht, want


def spread(n, seed, L=20):
    """n reads over slots 0 and 1 at random places, one in three with an edit"""
    rng = np.random.default_rng(seed)
    specs = []
    for i in range(n):
        s = int(rng.integers(0, 2))
        c = int(rng.integers(0, len(SLOTS[s])))
        specs.append((s, c, int(rng.integers(0, SLOTS[s][c] - L - 3)), L + i % 3, int(rng.integers(0, 2)), [i % L] if i % 3 == 0 else []))
    return specs


@pytest.mark.parametrize("n", [0, 1, 2, T - 1, T, T + 1, 3 * T + 5], ids=lambda n: f"n={n}")
def test_sizes_around_the_tile(eng, n):
    check(eng, spread(n, n + 1), 0, False, f"n={n}")
    if n % 2 == 0:
        check(eng, spread(n, n + 2), 16, True, f"n={n} paired, slots")


def test_more_reads_than_one_pass_of_the_writers_grid(eng):
    """k_samsort_write is the unit's one kernel whose grid is capped and loops"""
    import torch
    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    n = n_cu * SAM["SAM_WGS_PER_CU"] * SAM["SAM_WG_READS"] + 1024 + 6
    rng = np.random.default_rng(9)
    lo = rng.integers(0, 999_000, n)
    specs = [(0, 0, int(lo[i]), 17 + i % 5, i & 1, [i % 17] if i % 3 else []) for i in range(n)]
    check(eng, specs, 0, True, "the writer's workgroups loop")


def test_ties_and_stability(eng, layout):
    n = 2 * T + 38
    # every read at one (row, lo): the order is the read order, the text that of the unsorted call
    specs = [(1, 2, 777, 16 + i % 9, i & 1, [i % 16] if i % 2 else []) for i in range(n)]
    reads, truth, o, ht, want = check(eng, specs, layout, True, "one key")
    assert bytes(eng.sam(reads, rnames(), True, truth=truth).cpu().numpy()) == want[0] == _sam.sam_text(o, ht, _sam_sort.names_of(rnames()), True)
    # two keys alternating, keys ascending already, keys strictly descending
    check(eng, [(1, 2, 500 if i & 1 else 900, 20, 0, [3]) for i in range(n)], layout, True, "two keys")
    check(eng, [(1, 0, 3 * i, 18, i & 1, []) for i in range(n)], layout, True, "ascending")
    check(eng, [(1, 0, 3 * (n - i), 18, i & 1, []) for i in range(n)], layout, True, "descending")


def test_digit_boundaries(eng, layout):
    n = T + 100
    rng = np.random.default_rng(4)
    # keys that differ in the lowest digit only, and in the highest significant digit only (slot 2: lo has 25 bits, row 6)
    check(eng, [(2, 0, 5 * 2**DIGIT + int(x), 12, 0, []) for x in rng.integers(0, 2**DIGIT, n)], layout, False, "lowest digit")
    check(eng, [(2, 0, int(x) * 2**24 + 77, 12, 1, []) for x in rng.integers(0, 2, n)], layout, False, "highest digit of lo")
    check(eng, [((0, 0) if x else (3, 299)) + (9, 12, 0, [0]) for x in rng.integers(0, 2, n)], layout, False, "highest digit of the row")
    # 300 short contigs: the row crosses a digit, and with these names alone P + bits(rows - 1) = 11 + 9 is no multiple of 8
    rn3 = rnames((3,))
    specs = [(3, int(c), int(rng.integers(0, 380)), 15, int(c) & 1, []) for c in rng.integers(0, 300, n)]
    check(eng, specs, layout, False, "300 contigs", rn=rn3)
    check(eng, specs, layout, False, "300 contigs among all")
    # one contig of 20 M bases, reads on both sides of every digit's edge and at the contig's end
    L = 30
    los = [0, 2**8 - 1, 2**8, 2**16 - 1, 2**16, 2**24 - 1, 2**24, BIG - L]
    specs = [(2, 0, lo, L, i & 1, [0, L - 1]) for i, lo in enumerate(reversed(los + los))]
    check(eng, specs, layout, True, "digit edges of lo", rn=rnames((2,)))
    check(eng, specs + [(2, 0, BIG, 0, 0, []), (2, 0, BIG, 0, 1, [])], layout, True, "and a read without bases at the end")


def test_record_sizes_that_differ(eng, layout):
    """a length the scan and the writer disagreed on would shift every later line; mates far apart: PNEXT and TLEN are the
    unsorted call's"""
    specs = []
    for i, L in enumerate((0, 1, 15, 16, 17, 400, 17, 1, 400, 0, 16, 15)):
        ends = sorted({0, L - 1}) if L else []
        specs.append((1, 0, 250_000 - 20_000 * i, L, 0, ends))
        specs.append((1, 0, 1_000 + 20_000 * i, L, 1, ends))
    reads, truth, o, ht, want = check(eng, specs, layout, True, "sizes")
    lines = want[0].decode().splitlines()
    unsorted = _sam.sam_text(o, ht, _sam_sort.names_of(rnames()), True).decode().splitlines()
    assert sorted(lines) == sorted(unsorted) and lines != unsorted
    assert max(abs(_sam.parse(l)["tlen"]) for l in lines) > 200_000


def test_key_wider_than_32_bits():
    """a contig of 2^32 + 4096 bases (staged on an engine of its own, released at once): a dozen reads on both sides of 2^32"""
    e = Engine(0)
    try:
        n_bases = 2**32 + 4096
        e.stage_synthetic(0, [n_bases], 2)
        rn = [(0, ["big"])]
        los = [2**32 + 4000, 5, 2**32 - 1, 2**32, 2**31, 2**32 - 30, 77, 2**32 + 1, 2**24, n_bases - 30, 2**32 - 29, 2**16]
        specs = [(0, 0, lo, 30, i & 1, []) for i, lo in enumerate(los)]
        reads, truth, o, ht = build(specs, 0, e.device)
        want = _sam_sort.sorted_text(o, ht, rn, True)
        same(e.sam_sorted(reads, rn, True, truth=truth, with_keys=True), want, "above 2^32")
        assert int(want[1].max()) > 2**32 and b"\t4294967297\t" in want[0]
    finally:
        e.close()


@pytest.mark.parametrize("rng_mode,slots", [(_abi.RNG_PHILOX, 16), (_abi.RNG_REFERENCE, 0)], ids=["counter-slot16", "reference-compact"])
def test_simulated_short_pairs(eng, oracle, host_genomes, rng_mode, slots):
    eng.set_read_slots(slots)
    try:
        dev = eng.simulate_pe_reads_from_genome(1, MinimalShortErrorProfile(rng_mode=rng_mode).pod(), 3000, 5, qual_offset=33)
    finally:
        eng.set_read_slots(0)
    simulated(eng, oracle, host_genomes, dev, True)
    assert eng.last_sam_sort_ms() > 0


def test_simulated_long_reads(eng, oracle, host_genomes):
    lp = MinimalLongErrorProfile(gamma_mean=3000.0, gamma_std=2500.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    simulated(eng, oracle, host_genomes, eng.simulate_long_reads([1, 0], [200, 100], lp, 3, qual_offset=33), False)


def simulated(eng, oracle, host_genomes, dev, paired):
    rn = rnames()
    o = dev.to_host()
    t = _truth.model(oracle, o, host_genomes)
    want = _sam_sort.sorted_text(o, t, rn, paired)
    truth = eng.truth(dev)
    same(eng.sam_sorted(dev, rn, paired, truth=truth, with_keys=True), want, "simulated")
    # and the unsorted text of the device, stable-sorted on the host
    unsorted = bytes(eng.sam(dev, rn, paired, truth=truth).cpu().numpy())
    assert _sam_sort.stable_sort_of_text(unsorted, [n for _, names in rn for n in names]) == want[0]


def raw(eng, reads, truth, rn, paired, dst=None, capacity=None, key=None, line_off=None):
    """the raw calls: (plan status, total, emit status or None)"""
    out = _abi.TruthOut(truth.nm.data_ptr(), truth.edit_off.data_ptr(), truth.edit_pos.data_ptr(), truth.edit_ref.data_ptr(),
                        truth.edit_alt.data_ptr(), truth.edit_qual.data_ptr(), truth.n_reads, truth.n_edits)
    sn, pod, total = eng._sam_names(rn), reads.pod(), C.c_uint64(0)
    rc = eng.lib.simmr_sam_sort_plan(eng._h, C.byref(sn), C.byref(pod), C.byref(out), reads.n_reads, 1 if paired else 0, C.byref(total))
    if rc != 0 or dst is None:
        return rc, total.value, None
    cap = total.value if capacity is None else capacity
    return rc, total.value, eng.lib.simmr_sam_sort_emit(eng._h, C.byref(pod), C.byref(out), C.c_void_p(dst), cap, key, line_off)


def test_refusals_and_canaries(eng):
    import torch
    rn = rnames()
    specs = spread(600, 77)
    reads, truth, o, ht = build(specs, 0, eng.device)
    want, wkey, woff = _sam_sort.sorted_text(o, ht, rn, True)
    out = _abi.TruthOut(truth.nm.data_ptr(), truth.edit_off.data_ptr(), truth.edit_pos.data_ptr(), truth.edit_ref.data_ptr(),
                        truth.edit_alt.data_ptr(), truth.edit_qual.data_ptr(), truth.n_reads, truth.n_edits)
    pod, lib = reads.pod(), eng.lib
    CAN = 256
    buf = torch.full((CAN + len(want) + CAN,), 0xA5, dtype=torch.uint8, device=eng.device)
    clean = buf.clone()
    dst = buf.data_ptr() + CAN
    # the total is the unsorted plan's
    total = C.c_uint64(0)
    assert lib.simmr_sam_plan(eng._h, C.byref(eng._sam_names(rn)), C.byref(pod), C.byref(out), reads.n_reads, 1, C.byref(total)) == 0
    assert total.value == len(want)
    # the emit without its plan (an engine that has none; an unsorted plan is not one), and with other columns than the plan's
    fresh = Engine(0)
    try:
        assert fresh.lib.simmr_sam_sort_emit(fresh._h, C.byref(pod), C.byref(out), C.c_void_p(dst), len(want), None, None) == _abi.ESTATE
    finally:
        fresh.close()
    assert raw(eng, reads, truth, rn, True)[:2] == (0, len(want))
    other = reads.pod(); other.start = reads.end.data_ptr()
    assert lib.simmr_sam_sort_emit(eng._h, C.byref(other), C.byref(out), C.c_void_p(dst), len(want), None, None) == _abi.ESTATE
    # one byte short: ERANGE, nothing written
    assert raw(eng, reads, truth, rn, True, dst, len(want) - 1) == (0, len(want), _abi.ERANGE)
    torch.cuda.synchronize()
    assert torch.equal(buf, clean)
    # an unsorted plan on the same engine in between does not disturb the sorted one (and the other way round)
    assert raw(eng, reads, truth, rn, True)[:2] == (0, len(want))
    assert lib.simmr_sam_plan(eng._h, C.byref(eng._sam_names(rn)), C.byref(pod), C.byref(out), reads.n_reads, 1, C.byref(total)) == 0
    assert lib.simmr_sam_sort_emit(eng._h, C.byref(pod), C.byref(out), C.c_void_p(dst), len(want), None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[:CAN], clean[:CAN]) and torch.equal(buf[CAN + len(want):], clean[CAN + len(want):])
    assert bytes(buf[CAN:CAN + len(want)].cpu().numpy()) == want
    unsorted = torch.empty(len(want), dtype=torch.uint8, device=eng.device)
    assert lib.simmr_sam_emit(eng._h, C.byref(pod), C.byref(out), C.c_void_p(unsorted.data_ptr()), len(want)) == 0
    assert bytes(unsorted.cpu().numpy()) == _sam.sam_text(o, ht, _sam_sort.names_of(rn), True)
    # a read whose end passes its contig's length: EINVAL through the error word, and the plan is gone; the unsorted plan takes it
    at = next(i for i, s in enumerate(specs) if s[0] == 1 and s[4] == 0)
    keep = int(reads.end[at])
    reads.end[at] = SLOTS[1][specs[at][1]] + 1
    reads.start[at] = SLOTS[1][specs[at][1]] + 1 - specs[at][3]
    try:
        buf.copy_(clean)
        assert raw(eng, reads, truth, rn, True, dst) == (_abi.EINVAL, 0, None)
        assert lib.simmr_sam_sort_emit(eng._h, C.byref(pod), C.byref(out), C.c_void_p(dst), len(want), None, None) == _abi.ESTATE
        assert lib.simmr_sam_plan(eng._h, C.byref(eng._sam_names(rn)), C.byref(pod), C.byref(out), reads.n_reads, 1, C.byref(total)) == 0
        reads.end[at] = SLOTS[1][specs[at][1]]  # ending AT the contig's end is fine
        reads.start[at] = SLOTS[1][specs[at][1]] - specs[at][3]
        assert raw(eng, reads, truth, rn, True)[0] == 0
    finally:
        reads.end[at] = keep
        reads.start[at] = keep - specs[at][3]
    # a contig without a name, a slot that is not staged
    assert raw(eng, reads, truth, rnames((0, 2, 3)), True)[0] == _abi.EINVAL
    assert raw(eng, reads, truth, rn + [(7, ["x"])], True)[0] == _abi.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(buf, clean)  # no refusal stored a byte
    # columns altered between the plan and the emit: the read is refused by the writer, no store leaves a record's own bytes
    assert raw(eng, reads, truth, rn, True)[:2] == (0, len(want))
    keep = int(reads.contig[5])
    reads.contig[5] = 9
    try:
        assert lib.simmr_sam_sort_emit(eng._h, C.byref(pod), C.byref(out), C.c_void_p(dst), len(want), None, None) == _abi.EINVAL
    finally:
        reads.contig[5] = keep
    torch.cuda.synchronize()
    assert torch.equal(buf[:CAN], clean[:CAN]) and torch.equal(buf[CAN + len(want):], clean[CAN + len(want):])
    perm, _ = _sam_sort.order(o, rn)
    i5 = perm.index(5)
    a, b = int(woff[i5]), int(woff[i5 + 1])
    got = bytes(buf[CAN:CAN + len(want)].cpu().numpy())
    assert got[:a] == want[:a] and got[b:] == want[b:] and got[a:b] == b"\xa5" * (b - a)
    # a read whose line got shorter since the plan: every other line is where it was
    buf.copy_(clean)
    assert raw(eng, reads, truth, rn, True)[:2] == (0, len(want))
    r = next(i for i, s in enumerate(specs) if s[5])
    keep = int(reads.read_id[r])
    reads.read_id[r] = 7  # (a QNAME of one digit)
    try:
        rc = lib.simmr_sam_sort_emit(eng._h, C.byref(pod), C.byref(out), C.c_void_p(dst), len(want), None, None)
    finally:
        reads.read_id[r] = keep
    assert rc in (0, _abi.EINVAL)
    torch.cuda.synchronize()
    assert torch.equal(buf[:CAN], clean[:CAN]) and torch.equal(buf[CAN + len(want):], clean[CAN + len(want):])
    ir = perm.index(r)
    a, b = int(woff[ir]), int(woff[ir + 1])
    got = bytes(buf[CAN:CAN + len(want)].cpu().numpy())
    assert got[:a] == want[:a] and got[b:] == want[b:]
    # after a staging call the plan is stale; and everything is as before
    assert raw(eng, reads, truth, rn, True)[:2] == (0, len(want))
    eng.stage_synthetic(0, SLOTS[0], 10)
    assert lib.simmr_sam_sort_emit(eng._h, C.byref(pod), C.byref(out), C.c_void_p(dst), len(want), None, None) == _abi.ESTATE
    buf.copy_(clean)
    key = torch.empty(reads.n_reads, dtype=torch.int64, device=eng.device)
    off = torch.empty(reads.n_reads + 1, dtype=torch.int64, device=eng.device)
    assert raw(eng, reads, truth, rn, True, dst, None, C.c_void_p(key.data_ptr()), C.c_void_p(off.data_ptr())) == (0, len(want), 0)
    same((buf[CAN:CAN + len(want)], key, off), (want, wkey, woff), "after the refusals")


def test_limits_of_the_key(eng):
    """2^24 + 1 rows and a contig of 2^40 bases cannot be staged: the limits are checked on the routine the plan asks
    (simmr_sam_sort_key_bits) with counterfeit figures — tests/test_sam_sort_host.py — and here that the plan does ask it: the
    widths it answers for the staged names are those the model's keys need"""
    p, r = C.c_uint32(), C.c_uint32()
    n_rows = sum(len(v) for v in SLOTS.values())
    assert eng.lib.simmr_sam_sort_key_bits(n_rows, BIG, C.byref(p), C.byref(r)) == 0 and (p.value, r.value) == (25, 9)
    assert eng.lib.simmr_sam_sort_key_bits(2**24 + 1, BIG, None, None) == _abi.ERANGE
    assert eng.lib.simmr_sam_sort_key_bits(n_rows, 2**40, None, None) == _abi.ERANGE
