"""The SAM text and the coordinate-sorted SAM text of the device past 256 chunks of reads, against the plain-Python models of
tests/_sam.py and tests/_sam_sort.py, byte for byte.

One workgroup scans the per-chunk sums 256 at a time and carries a running total into the next 256 (sam_scan_chunks,
sam_kernels.hip).  Every test here is the first to enter the SECOND iteration of that loop:
  test_unsorted_text_past_256_chunks, test_unsorted_exact_capacity_past_256_chunks
      through k_sam_scan (sam_kernels.hip): chunks 256 and 257 of the record sizes take their prefix from the carry;
  test_sorted_text_keys_and_offsets_past_256_chunks, test_sorted_exact_capacity_past_256_chunks
      through k_samsort_scan (sam_sort_kernels.hip), over the sizes in sorted order; the sort before it runs five passes over
      a key of 34 bits, the last pass a partial digit, on 129 tiles (the loop of k_samsort_digit_scan stays in its first
      iteration here: tests/test_gpu_overlap_seams.py takes it further).
The read set is hand-built (the SAM pass reads the columns, never the genome), 258 chunks of SAM_CHUNK reads with the last one
partial; lengths, ids, strands and edits differ on both sides of reads 255, 256 and 257 x SAM_CHUNK, so a stale or lost carry
shifts bytes that differ.  Every expected byte comes from the models."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from simmr_amd.engine import Engine, Reads, Truth
from tests import _sam, _sam_sort

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def _defines(name, prefix):
    return {m.group(1): int(m.group(2)) for m in re.finditer(rf"^#define\s+({prefix}\w+)\s+(\d+)u?\b", (CSRC / name).read_text(), re.M)}


CHUNK = _defines("sam_kernels.hip", "SAM_")["SAM_CHUNK"]
SORT = _defines("sam_sort_kernels.hip", "SAMSORT_")
T, DIGIT = SORT["SAMSORT_TILE"], SORT["SAMSORT_DIGIT_BITS"]
SCAN = 256  # chunk sums a pass of sam_scan_chunks takes: its workgroup's threads
BIG = 20_000_000
SLOTS = {0: [1_000_000], 1: [300_000, 90_001, 30_017, 70_000, 123_457], 2: [BIG], 3: [400 + 3 * i for i in range(300)]}
N = SCAN * CHUNK + CHUNK + 6
SEAMS = [(SCAN - 1) * CHUNK, SCAN * CHUNK, (SCAN + 1) * CHUNK]
CAN = 256


def rnames():
    return [(s, [f"g{s}.c{c}|x" for c in range(len(SLOTS[s]))]) for s in SLOTS]


@pytest.fixture(scope="module")
def eng():
    """an engine of this module's own: four slots staged once (0: one contig, 1: five, 2: one of 20 M bases, 3: 300 short ones)"""
    e = Engine(0)
    for slot, lens in SLOTS.items():
        e.stage_synthetic(slot, lens, 10 + slot)
    yield e
    e.close()


def host_columns(seed=3):
    """N paired reads of 0 to 3 bases as compact host columns and truth columns (what tests/_sam.py takes): pairs on random
    contigs of the four slots at random places, mates sharing an id of one to ten digits, an edit or two on some reads"""
    rng = np.random.default_rng(seed)
    n, n_pairs = N, N // 2
    contigs = np.array([(s, c, SLOTS[s][c]) for s in SLOTS for c in range(len(SLOTS[s]))], dtype=np.int64)
    # a pair in three on the contig of 20 M bases, one in six on one of the 300 short ones, the rest on slots 0 and 1
    kind = rng.integers(0, 6, n_pairs)
    pick = np.where(kind < 2, 6, np.where(kind == 2, 7 + rng.integers(0, 300, n_pairs), rng.integers(0, 6, n_pairs)))
    at = np.repeat(pick, 2)
    g, c, clen = contigs[at, 0], contigs[at, 1], contigs[at, 2]
    L = rng.integers(0, 4, n)
    lo = (rng.random(n) * (clen - 3)).astype(np.int64)
    lo[::7] = np.where(rng.integers(0, 2, lo[::7].size) == 1, (clen - L)[::7], 0)  # at a contig's first base, ending at its last
    rev = rng.integers(0, 2, n).astype(np.uint8)
    rid = np.repeat((rng.integers(0, 10 ** 10, n_pairs) % 10 ** rng.integers(1, 11, n_pairs)) % 2**32, 2)
    n_edits = np.minimum(L, np.where(np.arange(n) % 3 == 0, 1 + np.arange(n) % 2, 0))
    # both sides of every seam of the chunk scan: lengths 0 3 | 1 2, ids of one digit | ten digits, edits on the reads next to it
    for k, seam in enumerate(SEAMS):
        L[seam - 2:seam + 2] = [0, 3, 1, 2] if k != 1 else [3, 0, 2, 1]
        rid[seam - 2:seam + 2] = [7, 7, 4_000_000_000 + k, 4_000_000_000 + k] if k != 1 else [4_294_967_295, 4_294_967_295, 0, 0]
        rev[seam - 2:seam + 2] = [0, 1, 1, 0]
        n_edits[seam - 2:seam + 2] = np.minimum(L[seam - 2:seam + 2], [0, 2, 1, 0] if k != 1 else [3, 0, 0, 1])
        lo[seam - 2:seam + 2] = np.minimum(lo[seam - 2:seam + 2], (clen - L)[seam - 2:seam + 2])
    assert ((lo >= 0) & (lo + L <= clen)).all()
    csr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(L, out=csr[1:])
    bases = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, int(csr[n]))]
    quals = (33 + rng.integers(0, 61, int(csr[n]))).astype(np.uint8)
    eoff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(n_edits, out=eoff[1:])
    within = np.arange(int(eoff[n]), dtype=np.int64) - np.repeat(eoff[:n], n_edits)
    # ascending offsets inside the read: the first ones, or (one read in two with room) the last ones
    epos = within + np.repeat(np.where(np.arange(n) % 2 == 1, L - n_edits, 0), n_edits)
    eref = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, epos.size)]
    start, end = np.where(rev == 1, lo + L, lo), np.where(rev == 1, lo, lo + L)
    o = {"start": start.astype(np.uint64), "end": end.astype(np.uint64), "contig": c.astype(np.uint32), "genome": g.astype(np.uint32),
         "read_id": rid.astype(np.uint32), "flags": rev, "seq_off": csr.astype(np.uint64), "seq": bases, "qual": quals}
    ht = {"edit_off": eoff.astype(np.uint64), "edit_pos": epos.astype(np.uint32), "edit_ref": eref}
    return o, ht


def device_columns(o, ht, layout, device):
    """Reads and Truth on the device from the host columns, in the compact or the 16-byte slot layout (reverse mates right-aligned)"""
    import torch
    n = len(o["start"])
    csr, rev = o["seq_off"].astype(np.int64), o["flags"]
    L = np.diff(csr)
    slot = (L + 15) // 16 * 16 if layout == 16 else L
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(slot, out=first[1:])
    seq_off = first.copy()
    seq_off[:n] += np.where(rev == 1, slot - L, 0)
    within = np.arange(int(csr[n]), dtype=np.int64) - np.repeat(csr[:n], L)
    seq, qual = np.zeros(int(first[n]), dtype=np.uint8), np.zeros(int(first[n]), dtype=np.uint8)
    seq[np.repeat(seq_off[:n], L) + within] = o["seq"]
    qual[np.repeat(first[:n], L) + within] = o["qual"]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(device)
    pad = lambda a: np.concatenate([a, np.zeros(1, a.dtype)])  # (no tensor without an element)
    i64 = lambda a: a.astype(np.int64)
    reads = Reads(seq=t(pad(seq), np.uint8), qual=t(pad(qual), np.uint8), seq_off=t(seq_off, np.int64), start=t(pad(i64(o["start"])), np.int64),
                  end=t(pad(i64(o["end"])), np.int64), contig=t(pad(i64(o["contig"])), np.int32), genome=t(pad(i64(o["genome"])), np.int32),
                  read_id=t(pad(i64(o["read_id"])), np.int64).to(torch.int32), flags=t(pad(rev), np.uint8), n_reads=n, total_bases=int(first[n]),
                  qual_offset=33, slot_bytes=layout)
    eoff = i64(ht["edit_off"])
    truth = Truth(nm=t(pad(np.diff(eoff)), np.int32), edit_off=t(eoff, np.int64), edit_pos=t(pad(i64(ht["edit_pos"])), np.int32),
                  edit_ref=t(pad(ht["edit_ref"]), np.uint8), edit_alt=t(pad(ht["edit_ref"]), np.uint8), edit_qual=t(pad(ht["edit_ref"]), np.uint8),
                  n_reads=n, n_edits=int(eoff[n]))
    return reads, truth


@pytest.fixture(scope="module")
def columns():
    return host_columns()


@pytest.fixture(scope="module")
def on_device(eng, columns):
    """the read set on the device, once per layout"""
    return {layout: device_columns(*columns, layout, eng.device) for layout in (0, 16)}


@pytest.fixture(scope="module")
def unsorted_text(columns):
    return _sam.sam_text(*columns, _sam_sort.names_of(rnames()), True)


@pytest.fixture(scope="module")
def sorted_model(columns):
    return _sam_sort.sorted_text(*columns, rnames(), True)


def truth_out(truth):
    return _abi.TruthOut(truth.nm.data_ptr(), truth.edit_off.data_ptr(), truth.edit_pos.data_ptr(), truth.edit_ref.data_ptr(),
                         truth.edit_alt.data_ptr(), truth.edit_qual.data_ptr(), truth.n_reads, truth.n_edits)


def same_text(got, want, what):
    if got != want:
        gl, wl = got.split(b"\n"), want.split(b"\n")
        i = next((k for k in range(min(len(gl), len(wl))) if gl[k] != wl[k]), min(len(gl), len(wl)))
        raise AssertionError(f"{what}: {len(got)} bytes against {len(want)}; line {i} differs:\n{gl[i:i + 1]}\n{wl[i:i + 1]}")


def second_level(n):
    """the precondition of every test here: the scan over the n reads' chunk sums enters its second iteration, with two chunks"""
    n_chunks = (n + CHUNK - 1) // CHUNK
    assert n_chunks > SCAN and n_chunks - SCAN == 2 and n % CHUNK not in (0, CHUNK - 1), (n, CHUNK)
    return n_chunks


def test_the_read_set_differs_across_the_seams(columns, unsorted_text):
    """what the set promises: records of different sizes, strands and edits on both sides of every seam of the scan, ids of one
    to ten digits, and a sorted order far from the read order on a key of 34 bits"""
    o, ht = columns
    assert second_level(len(o["start"])) == 258 or CHUNK != 1024
    lines = unsorted_text.split(b"\n")[:-1]
    assert len(lines) == N
    for seam in SEAMS:
        around = [len(l) for l in lines[seam - 2:seam + 2]]
        assert around[1] != around[2] and len(set(around)) >= 3, (seam, around)
        assert int(np.diff(ht["edit_off"].astype(np.int64))[seam - 2:seam + 2].sum()) >= 1
    assert {len(str(int(x))) for x in o["read_id"]} == set(range(1, 11))
    assert set(np.diff(o["seq_off"].astype(np.int64)).tolist()) == {0, 1, 2, 3}
    perm, key = _sam_sort.order(o, rnames())
    n_rows = sum(len(v) for v in SLOTS.values())
    bits = int(max(o["start"].max(), o["end"].max())).bit_length() + (n_rows - 1).bit_length()
    assert BIG.bit_length() + (n_rows - 1).bit_length() == 34 and bits == 34 and -(-34 // DIGIT) == 5 and 34 % DIGIT != 0
    assert len({k >> 40 for k in key}) == n_rows and int(np.mean(np.abs(np.array(perm) - np.arange(N)))) > N // 8
    assert (N + T - 1) // T > 1


def test_unsorted_text_past_256_chunks(eng, on_device, unsorted_text):
    """k_sam_scan's second iteration: the text in both layouts, and simmr_sam_plan's total"""
    second_level(N)
    for layout, (reads, truth) in on_device.items():
        pod, out, total = reads.pod(), truth_out(truth), C.c_uint64(0)
        assert eng.lib.simmr_sam_plan(eng._h, C.byref(eng._sam_names(rnames())), C.byref(pod), C.byref(out), reads.n_reads, 1, C.byref(total)) == 0
        assert total.value == len(unsorted_text), f"layout {layout}: the plan's total"
        same_text(bytes(eng.sam(reads, rnames(), True, truth=truth).cpu().numpy()), unsorted_text, f"layout {layout}")


def test_sorted_text_keys_and_offsets_past_256_chunks(eng, on_device, sorted_model):
    """k_samsort_scan's second iteration: the text, every key and every entry of line_off"""
    second_level(N)
    wtext, wkey, woff = sorted_model
    for layout, (reads, truth) in on_device.items():
        text, key, line_off = eng.sam_sorted(reads, rnames(), True, truth=truth, with_keys=True)
        same_text(bytes(text.cpu().numpy()), wtext, f"layout {layout}")
        assert np.array_equal(key.cpu().numpy(), wkey), f"layout {layout}: key"
        assert np.array_equal(line_off.cpu().numpy(), woff), f"layout {layout}: line_off"


def canaries(eng, want, emit):
    """emit(dst, capacity) -> status: one byte short is ERANGE with nothing written; at the exact capacity the text lies between
    untouched canaries"""
    import torch
    buf = torch.full((CAN + len(want) + CAN,), 0xA5, dtype=torch.uint8, device=eng.device)
    dst = buf.data_ptr() + CAN
    assert emit(dst, len(want) - 1) == _abi.ERANGE
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    assert emit(dst, len(want)) == 0
    torch.cuda.synchronize()
    assert bool((buf[:CAN] == 0xA5).all()) and bool((buf[CAN + len(want):] == 0xA5).all())
    same_text(bytes(buf[CAN:CAN + len(want)].cpu().numpy()), want, "between canaries")


def test_unsorted_exact_capacity_past_256_chunks(eng, on_device, unsorted_text):
    second_level(N)
    reads, truth = on_device[0]
    pod, out, total = reads.pod(), truth_out(truth), C.c_uint64(0)
    assert eng.lib.simmr_sam_plan(eng._h, C.byref(eng._sam_names(rnames())), C.byref(pod), C.byref(out), reads.n_reads, 1, C.byref(total)) == 0
    assert total.value == len(unsorted_text)
    canaries(eng, unsorted_text, lambda dst, cap: eng.lib.simmr_sam_emit(eng._h, C.byref(pod), C.byref(out), C.c_void_p(dst), cap))


def test_sorted_exact_capacity_past_256_chunks(eng, on_device, sorted_model):
    second_level(N)
    reads, truth = on_device[0]
    pod, out, total = reads.pod(), truth_out(truth), C.c_uint64(0)
    assert eng.lib.simmr_sam_sort_plan(eng._h, C.byref(eng._sam_names(rnames())), C.byref(pod), C.byref(out), reads.n_reads, 1, C.byref(total)) == 0
    assert total.value == len(sorted_model[0])
    canaries(eng, sorted_model[0], lambda dst, cap: eng.lib.simmr_sam_sort_emit(eng._h, C.byref(pod), C.byref(out), C.c_void_p(dst), cap, None, None))
