"""The BAM records of the device (simmr_bam_plan / simmr_bam_emit, include/simmr_hip.h) against the plain-Python record of
tests/_bam.py over the host copies of the same columns: byte for byte, and the same records read back as SAM lines against
the text simmr_sam_emit makes of the same columns.  The columns are hand-built (the pass reads the columns, never the genome)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from simmr_amd.engine import Engine
from tests import _bam, _sam
from tests.test_gpu_sam_seams import device_columns, truth_out

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"
CHUNK = int(re.search(r"^#define\s+SAM_CHUNK\s+(\d+)u", (CSRC / "sam_kernels.hip").read_text(), re.M).group(1))
SLOTS = {0: [1_000_000], 1: [3000, 901, 317], 3: [4000]}
RNAMES = [(s, [f"g{s}.c{c}|x" for c in range(len(SLOTS[s]))]) for s in SLOTS]
NAMES = {(s, c): n for s, ns in RNAMES for c, n in enumerate(ns)}
REFS = [(n, SLOTS[s][c]) for s, ns in RNAMES for c, n in enumerate(ns)]
CONTIGS = [(s, c) for s in SLOTS for c in range(len(SLOTS[s]))]
LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 150, 151, 65535)
CAN = 256


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    for slot, lens in SLOTS.items():
        e.stage_synthetic(slot, lens, 10 + slot)
    yield e
    e.close()


def columns(specs, seed=1, alphabet=b"ACGTN", qual_range=(33, 94)):
    """compact host columns and truth columns for specs of (contig index, lo, L, reverse, read_id, [edit offsets, ascending])"""
    rng = np.random.default_rng(seed)
    n = len(specs)
    L = np.array([s[2] for s in specs], dtype=np.int64)
    lo = np.array([s[1] for s in specs], dtype=np.int64)
    rev = np.array([s[3] for s in specs], dtype=np.uint8)
    csr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(L, out=csr[1:])
    eoff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(s[5]) for s in specs], out=eoff[1:])
    for s in specs:
        assert list(s[5]) == sorted(set(s[5])) and all(0 <= p < s[2] for p in s[5]), s
    o = {"start": np.where(rev == 1, lo + L, lo).astype(np.uint64), "end": np.where(rev == 1, lo, lo + L).astype(np.uint64),
         "contig": np.array([CONTIGS[s[0]][1] for s in specs], dtype=np.uint32), "genome": np.array([CONTIGS[s[0]][0] for s in specs], dtype=np.uint32),
         "read_id": np.array([s[4] for s in specs], dtype=np.uint32), "flags": rev, "seq_off": csr.astype(np.uint64),
         "seq": np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), int(csr[n]))],
         "qual": rng.integers(qual_range[0], qual_range[1], int(csr[n])).astype(np.uint8)}
    epos = np.array([p for s in specs for p in s[5]], dtype=np.uint32)
    t = {"edit_off": eoff.astype(np.uint64), "edit_pos": epos, "edit_ref": np.frombuffer(b"ACGTN-", dtype=np.uint8)[rng.integers(0, 6, epos.size)]}
    return o, t


def plan(eng, reads, truth, paired, rnames=RNAMES):
    sn, pod, out, total = eng._sam_names(rnames), reads.pod(), truth_out(truth), C.c_uint64(0)
    rc = eng.lib.simmr_bam_plan(eng._h, C.byref(sn), C.byref(pod), C.byref(out), reads.n_reads, 1 if paired else 0, C.byref(total))
    return rc, total.value


def emit(eng, reads, truth, dst, capacity):
    pod, out = reads.pod(), truth_out(truth)
    return eng.lib.simmr_bam_emit(eng._h, C.byref(pod), C.byref(out), C.c_void_p(dst), capacity)


def same_records(got, want, what):
    if got != want:
        i = next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} bytes against {len(want)}; first difference at byte {i}: {got[i:i + 24].hex()} / {want[i:i + 24].hex()}")


def check(eng, o, t, layout, paired, what, with_sam=True):
    """the records between guard bytes are the model's; read back, they are the lines of Engine.sam for the same columns"""
    import torch
    reads, truth = device_columns(o, t, layout, eng.device)
    want = _bam.bam_records(o, t, RNAMES, paired)
    rc, total = plan(eng, reads, truth, paired)
    assert (rc, total) == (0, len(want)), (what, rc, total, len(want))
    buf = torch.full((CAN + total + CAN,), 0xA5, dtype=torch.uint8, device=eng.device)
    assert emit(eng, reads, truth, buf.data_ptr() + CAN, total) == 0, what
    torch.cuda.synchronize()
    h = bytes(buf.cpu().numpy())
    assert h[:CAN] == b"\xa5" * CAN and h[CAN + total:] == b"\xa5" * CAN, what
    same_records(h[CAN:CAN + total], want, what)
    if with_sam:
        text = bytes(eng.sam(reads, RNAMES, paired, truth).cpu().numpy()).decode("latin-1")
        assert text == _sam.sam_text(o, t, NAMES, paired).decode("latin-1"), what
        assert "".join(_bam.to_sam_line(r, REFS) for r in _bam.parse_records(h[CAN:CAN + total])) == text, what
    return reads, truth, want


def edge_specs():
    """every length on both strands, with no edit, one, adjacent ones, and edits at offsets 0 and L - 1; ids of one to ten digits"""
    specs = []
    for i, L in enumerate(LENGTHS):
        for rev in (0, 1):
            for k, edits in enumerate(([], [0], [L - 1], [0, 1, L - 2, L - 1], [L // 2])):
                edits = sorted({p for p in edits if 0 <= p < L})
                rid = (4_294_967_295, 7, 10 ** 8 - 1, 10 ** 8, 123_456_789)[k] if i % 2 else (0, 99, 4_000_000_000, 10 ** 9 - 1, 65_536)[k]
                specs.append((i % len(CONTIGS), 40 + 977 * i + 13 * k + rev, L, rev, rid, edits))
    return specs


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "unpaired"])
@pytest.mark.parametrize("layout", [0, 16], ids=["compact", "slot16"])
def test_read_lengths_strands_and_edits_at_the_edges(eng, layout, paired):
    o, t = columns(edge_specs(), seed=2)
    check(eng, o, t, layout, paired, f"edges layout={layout} paired={paired}")
    assert eng.last_bam_ms() > 0


@pytest.mark.parametrize("layout", [0, 16], ids=["compact", "slot16"])
def test_bytes_outside_acgtn_and_qualities_outside_the_printable_range(eng, layout):
    specs = [(k % len(CONTIGS), 10 + k, L, k & 1, k, [L - 1] if L else []) for k, L in enumerate((5, 33, 64, 7, 150, 31, 16, 2))]
    o, t = columns(specs, seed=3, alphabet=b"ACGTN-acgtnRY*=")
    assert len(set(bytes(o["seq"])) - set(b"ACGTN")) >= 8
    check(eng, o, t, layout, True, "odd bases")
    # qualities below 33 (written as 0) and above 126: no SAM text shows them, the model alone decides
    o, t = columns(specs, seed=4, qual_range=(0, 256))
    assert o["qual"].min() < 33 and o["qual"].max() > 160
    check(eng, o, t, layout, False, "odd qualities", with_sam=False)


def test_edit_counts_on_both_sides_of_the_tag_type(eng):
    """NM:C up to 255 edits, NM:S from 256; runs of adjacent edits; both strands"""
    specs = []
    for k, n in enumerate((0, 1, 255, 256, 257, 1000)):
        for rev in (0, 1):
            specs.append((0, 5000 * k + rev, 1200, rev, 1000 + k, list(range(3, 3 + n))))               # adjacent
            specs.append((0, 5000 * k + 77, 1200, rev, 2000 + k, [(1199 * j) // max(n - 1, 1) for j in range(n)] if n > 1 else [0] * n))
    o, t = columns(specs, seed=5)
    _, _, want = check(eng, o, t, 0, True, "edit counts")
    recs = _bam.parse_records(want)
    assert {r["tags"]["NM"] for r in recs} >= {("C", 0), ("C", 1), ("C", 255), ("S", 256), ("S", 257), ("S", 1000)}


def test_the_last_position_an_int32_holds(eng):
    """pos + L == 2^31 - 1 is taken (bin is the low 16 bits of reg2bin out there), a read ending at 2^31 is refused, for either mate"""
    L = 5
    top = 2 ** 31 - 1
    specs = [(0, top - L, L, 0, 1, [2]), (0, top - L - 9, L, 1, 1, [])]
    o, t = columns(specs, seed=6)
    check(eng, o, t, 0, True, "the last position")
    check(eng, o, t, 16, False, "the last position")
    for r in (0, 1):
        bad = [list(s) for s in specs]
        bad[r][1] = top - L + 1
        o, t = columns([tuple(s) for s in bad], seed=6)
        for layout in (0, 16):
            reads, truth = device_columns(o, t, layout, eng.device)
            assert plan(eng, reads, truth, True) == (_abi.EINVAL, 0), (r, layout)
            assert emit(eng, reads, truth, reads.seq.data_ptr(), 0) == _abi.ESTATE


def chunk_specs(n):
    """n reads of 0 to 3 bases, pairs on changing contigs, an edit on one read in three"""
    specs = []
    for r in range(n):
        L = (r * 7 + r // CHUNK) % 4
        specs.append(((r // 2) % len(CONTIGS), (r * 37) % 300, L, (r >> 1 ^ r) & 1, (r // 2) * 2_654_435_761 % 2 ** 32 % 10 ** (1 + r % 10), [L - 1] if L and r % 3 == 0 else []))
    return specs


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2], ids=lambda n: f"{n}-reads")
def test_read_counts_around_a_chunk(eng, n):
    o, t = columns(chunk_specs(n), seed=7)
    check(eng, o, t, 0, n % 2 == 0, f"{n} reads")


def test_more_than_256_chunks(eng):
    """the scan of the chunk sums enters its second iteration: chunks 256 and 257 take their prefix from the carry"""
    n = 256 * CHUNK + CHUNK + 6
    o, t = columns(chunk_specs(n), seed=8)
    check(eng, o, t, 16, True, "258 chunks", with_sam=False)


def test_no_records_at_all(eng):
    o, t = columns([], seed=9)
    reads, truth = device_columns(o, t, 0, eng.device)
    assert plan(eng, reads, truth, True) == (0, 0) and emit(eng, reads, truth, None, 0) == 0
    assert eng.bam(reads, RNAMES, True, truth).numel() == 0


def test_capacity_state_and_columns_changed_between_plan_and_emit(eng):
    import torch
    o, t = columns(edge_specs()[:80], seed=10)
    reads, truth = device_columns(o, t, 0, eng.device)
    want = _bam.bam_records(o, t, RNAMES, True)
    buf = torch.full((CAN + len(want) + CAN,), 0xA5, dtype=torch.uint8, device=eng.device)
    clean, dst = buf.clone(), buf.data_ptr() + CAN
    assert int(truth.edit_off[42]) > 0 and int(truth.edit_off[44]) - int(truth.edit_off[43]) == 4
    # ESTATE: an engine without a plan, a plan for other columns, a staging call since the plan
    fresh = Engine(0)
    try:
        assert emit(fresh, reads, truth, dst, len(want)) == _abi.ESTATE
    finally:
        fresh.close()
    assert plan(eng, reads, truth, True) == (0, len(want))
    # ERANGE: one byte short, nothing written; the plan stays
    assert emit(eng, reads, truth, dst, len(want) - 1) == _abi.ERANGE
    torch.cuda.synchronize()
    assert torch.equal(buf, clean)
    other, other_truth = device_columns(o, t, 0, eng.device)
    assert emit(eng, other, truth, dst, len(want)) == _abi.ESTATE and emit(eng, reads, other_truth, dst, len(want)) == _abi.ESTATE
    # a SAM plan on the same engine does not disturb the BAM plan, nor the other way round
    text = eng.sam(reads, RNAMES, True, truth)
    assert emit(eng, reads, truth, dst, len(want)) == 0
    torch.cuda.synchronize()
    same_records(bytes(buf[CAN:CAN + len(want)].cpu().numpy()), want, "after a SAM plan")
    assert bytes(text.cpu().numpy()) == _sam.sam_text(o, t, NAMES, True)
    eng.stage_synthetic(3, SLOTS[3], 13)
    assert emit(eng, reads, truth, dst, len(want)) == _abi.ESTATE
    # the refusals of the SAM plan
    raw = reads.pod(); raw.qual_offset = 0
    sn, out, total = eng._sam_names(RNAMES), truth_out(truth), C.c_uint64(0)
    assert eng.lib.simmr_bam_plan(eng._h, C.byref(sn), C.byref(raw), C.byref(out), reads.n_reads, 1, C.byref(total)) == _abi.EINVAL
    pod = reads.pod()
    assert eng.lib.simmr_bam_plan(eng._h, C.byref(sn), C.byref(pod), C.byref(out), reads.n_reads - 1, 1, C.byref(total)) == _abi.EINVAL
    assert plan(eng, reads, truth, True, RNAMES[:2] + [(3, ["has space"])])[0] == _abi.ENOTSUP
    assert plan(eng, reads, truth, True, RNAMES[:2])[0] == _abi.EINVAL  # reads on a slot without names: the error word
    # columns corrupted BETWEEN the plan and the emit: EINVAL, and no store leaves dst — nor, for the reads still taken, their records
    offs = np.cumsum([0] + [len(_bam.record(o, t, _bam.rows_of(RNAMES), r, True)) for r in range(reads.n_reads)])
    for col, at, value, refused in ((truth.edit_off, 43, 1 << 40, (42, 43)), (truth.edit_off, 43, 0, (42, 43)), (reads.seq_off, 45, 1 << 40, (44, 45)),
                                    (reads.contig, 41, 5, (41,)), (reads.start, 47, 1 << 31, (47,))):
        buf.copy_(clean)
        assert plan(eng, reads, truth, True) == (0, len(want))
        keep = int(col[at])
        col[at] = value
        try:
            assert emit(eng, reads, truth, dst, len(want)) == _abi.EINVAL, (at, value)
        finally:
            col[at] = keep
        torch.cuda.synchronize()
        h = bytes(buf.cpu().numpy())
        assert h[:CAN] == b"\xa5" * CAN and h[CAN + len(want):] == b"\xa5" * CAN, (at, value)
        got = h[CAN:CAN + len(want)]
        for r in range(reads.n_reads):
            a, b = int(offs[r]), int(offs[r + 1])
            if r not in refused and (r ^ 1) not in refused:
                assert got[a:b] == want[a:b], (at, value, r)
        for r in refused:  # (a refused read: its record was left alone)
            assert got[int(offs[r]):int(offs[r + 1])] == b"\xa5" * int(offs[r + 1] - offs[r]), (at, value, r)
        assert emit(eng, reads, truth, dst, len(want)) == _abi.ESTATE  # the plan is gone
    # and everything is as before
    buf.copy_(clean)
    assert plan(eng, reads, truth, True) == (0, len(want)) and emit(eng, reads, truth, dst, len(want)) == 0
    torch.cuda.synchronize()
    same_records(bytes(buf[CAN:CAN + len(want)].cpu().numpy()), want, "after the refusals")


def test_the_python_method_frames_the_records(eng):
    o, t = columns(edge_specs(), seed=11)
    reads, truth = device_columns(o, t, 0, eng.device)
    want = _bam.bam_records(o, t, RNAMES, False)
    assert bytes(eng.bam(reads, RNAMES, False, truth, framed=False).cpu().numpy()) == want
    framed = bytes(eng.bam(reads, RNAMES, False, truth).cpu().numpy())
    assert b"".join(_bam.bgzf_blocks(framed)) == want and len(want) > 2 * _bam.BGZF_BLOCK
