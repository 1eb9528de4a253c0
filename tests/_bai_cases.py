"""Shapes for the sorted BAM and its index (tests/test_bai_host.py, tests/test_gpu_bam_sorted.py): hand-built read columns on a
names set whose first contig passes 2^20 bases, the records of tests/_bam.py in coordinate order, and the file around them; and
the columns of an index alone, by the loop of the index kernels they are meant to pass (index_shape: tests/test_gpu_bai_seams.py
at full size, tests/test_seams_host.py at a small one)."""
import struct

import numpy as np

from simmr_amd.sam import BGZF_EOF, bam_header
from tests import _bam

SLOTS = {0: [1_100_000], 1: [3000, 901, 317], 3: [4000]}
RNAMES = [(s, [f"g{s}.c{c}|x" for c in range(len(SLOTS[s]))]) for s in SLOTS]
REFS = [(n, SLOTS[s][c]) for s, ns in RNAMES for c, n in enumerate(ns)]
CONTIGS = [(s, c) for s in SLOTS for c in range(len(SLOTS[s]))]
WINDOW = 1 << 14
MANY_SLOT = 5  # a names set of its own: 300 short contigs
MANY = [200 + c for c in range(300)]
MANY_RNAMES = [(MANY_SLOT, [f"m{c}" for c in range(300)])]
MANY_REFS = [(f"m{c}", MANY[c]) for c in range(300)]
MANY_CONTIGS = [(MANY_SLOT, c) for c in range(300)]


def columns(specs, seed=1, contigs=CONTIGS):
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
    o = {"start": np.where(rev == 1, lo + L, lo).astype(np.uint64), "end": np.where(rev == 1, lo, lo + L).astype(np.uint64),
         "contig": np.array([contigs[s[0]][1] for s in specs], dtype=np.uint32), "genome": np.array([contigs[s[0]][0] for s in specs], dtype=np.uint32),
         "read_id": np.array([s[4] for s in specs], dtype=np.uint32), "flags": rev, "seq_off": csr.astype(np.uint64),
         "seq": np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, int(csr[n]))],
         "qual": rng.integers(33, 94, int(csr[n])).astype(np.uint8)}
    epos = np.array([p for s in specs for p in s[5]], dtype=np.uint32)
    t = {"edit_off": eoff.astype(np.uint64), "edit_pos": epos, "edit_ref": np.frombuffer(b"ACGTN-", dtype=np.uint8)[rng.integers(0, 6, epos.size)]}
    return o, t


def mixed_specs():
    """the lengths of tests/_hand_built.py on both strands over every contig, out of order, with ties on one position"""
    specs = []
    for i, L in enumerate((0, 1, 15, 16, 17, 511, 512, 513)):
        for rev in (0, 1):
            specs.append((0, 11_900 - 37 * i, L, rev, len(specs), [0, L // 2, L - 1] if L > 2 and i % 2 else []))
            specs.append((1 + i % 4, (1000 - 97 * i + rev) % 100, min(L, 200), rev, len(specs), [L - 1] if 0 < L <= 200 else []))
    for k in range(6):  # ties: one position, the stable order decides
        specs.append((4, 77, 20 + k % 2, k & 1, len(specs), []))
    return specs


def level_specs():
    """contig 0 (1.1 Mbases): reads that straddle 2^14, 2^17 and 2^20, end exactly at a window edge, start exactly at one, a read
    without bases on an edge, and the longest read over five windows; a far gap of empty windows in front of the last"""
    at = [(WINDOW - 5, 10), ((1 << 17) - 5, 10), ((1 << 20) - 5, 20), (WINDOW - 50, 50), (2 * WINDOW, 30), (3 * WINDOW, 0), (3 * WINDOW - 1, 1),
          (200_000, 65_535), (200_001, 3), (1_099_990, 10), (0, 1), (5 * WINDOW + 100, WINDOW), (40, 2), (100_000, 150)]  # (an even count: pairs)
    return [(0, lo, L, k & 1, 100 + k, [L // 2] if L else []) for k, (lo, L) in enumerate(at)]


def many_specs():
    """one read per reference of the 300, none on every third and none on the first and the last, in descending order"""
    used = [c for c in range(1, 299) if c % 3]
    return [(c, (c * 13) % 150, 20, c & 1, k, []) for k, c in enumerate(reversed(used))]


def sorted_records(o, t, paired, rnames=RNAMES):
    """(the records of tests/_bam.py stably sorted by (row, lo), the order as read indices)"""
    rows = _bam.rows_of(rnames)
    n = len(o["start"])
    key = [(rows[(int(o["genome"][r]), int(o["contig"][r]))], int(min(o["start"][r], o["end"][r]))) for r in range(n)]
    order = sorted(range(n), key=lambda r: key[r])
    return b"".join(_bam.record(o, t, rows, r, paired) for r in order), order


def header(refs=REFS):
    return bam_header([n for n, _ in refs], [l for _, l in refs], "coordinate")


def file_of(records, refs=REFS):
    """(the file: header and records framed as one stream, then the end-of-file block; the header's bytes)"""
    head = header(refs)
    return _bam.bgzf_frame(head + records) + BGZF_EOF, len(head)


def edges(refs=REFS):
    """(ref, beg, end) around every window edge of every reference, and a few whole-reference and empty-tail queries"""
    out = []
    for ref, (_, length) in enumerate(refs):
        out.append((ref, 0, max(length, 1)))
        for w in range(0, length + WINDOW, WINDOW):
            for b in (w - 1, w, w + 1):
                if b >= 0:
                    out.extend([(ref, b, b + 1), (ref, b, b + WINDOW), (ref, max(b - 40, 0), b + 1)])
    return out


# ---- records and columns the index alone needs (tests/test_seams_host.py, tests/test_gpu_bam_sorted.py, tests/test_gpu_bai_seams.py)
TOP = (1 << 29) - 1  # the longest reference a BAI index covers


def plain(ref_id, pos, L):
    """a record without cigar and tags whose interval is [pos, pos + L)"""
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, 2, 255, _bam.reg2bin(pos, pos + L), 0, 0, L, -1, -1, 0) + b"a\0"
    body += bytes([0x11] * (L // 2)) + (bytes([0x10]) if L & 1 else b"") + bytes([30] * L)
    return struct.pack("<i", len(body)) + body


def plain_offsets(lo, end):
    """rec_off[0 .. n] of the stream of plain(ref, lo, end - lo) records: 38 bytes and the packed bases and qualities of each"""
    L = np.asarray(end, dtype=np.int64) - np.asarray(lo, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(38 + (L + 1) // 2 + L)]).astype(np.int64)


def _around_edges(edges):
    """(lo, end) of records that change bin at every record.  For an edge between windows e - 1 and e, taken c times: c pairs of
    a one-base record in window e - 1 (its leaf bin) and, one base on, a record that reaches one base over the edge: it lands
    in the smallest bin that holds both windows — level 4, 3, 2, 1 or bin 0 for an e divisible by 1, 8, 64, 512, 4096.  The pairs of
    an edge step two bases towards it, so the leaf and the upper bin take c chunks each, interleaved in file order."""
    lo, end = [], []
    for e, c in edges:
        assert 0 < e < 1 << 15 and 2 * c <= WINDOW
        p = e * WINDOW - 2 * (c - np.arange(c, dtype=np.int64))
        lo.append(np.stack([p, p + 1], axis=1).ravel())
        end.append(np.stack([p + 1, np.full(c, e * WINDOW + 1, dtype=np.int64)], axis=1).ravel())
    return np.concatenate(lo), np.concatenate(end)


def _bin_change_edges(m, big):
    assert m < 4096
    return [(e, 1) for e in range(1, m + 1)] + [(e, 2) for e in (8, 64, 512) if e > m] + [(4096, big), (8192, 3)]


def _sparse_windows(n_intv):
    """windows with a one-base record: none in the first 256, then lane 255 alone (511), lane 0 alone (512), two tiles of 256
    without any, a few, and the last window; what of that a shorter reference has room for"""
    ws = (511, 512, 1287, 1480, 1791, 1792, 20000, 20001) if n_intv > 1800 else (3, 255, 256)
    return sorted({w for w in ws if w < n_intv - 1} | {n_intv - 1})


def index_shape(kind, **size):
    """Columns for Engine.bai and tests/_seams.py:bai_from_columns, by the loop they are meant to pass; the sizes are the
    caller's (the GPU tests derive them from the kernels' constants and the CU count, the host test passes small ones).
    Returns {n_ref, ref, lo, end, ref_len}: int64 arrays ascending by (ref, lo), ref_len a list or None.
      bin_changes  m, big, n_ref      the bin changes at every record (_around_edges): edges 1 .. m once, 8, 64 and 512 twice, 4096
                                      `big` times, 8192 three times; on n_ref references (a little fewer edges on each, `big` on the last)
      ties         k                  k records on one position, alternately of 1 and of 16385 bases: two bins, every record a chunk
      linear       n_intvs, long      a reference of n windows per entry with records in few windows (_sparse_windows), an empty one,
                                      and one whose first record spans `long` windows with later short ones inside it
      strides      n_ref, n           n records over the references that are neither the first, the last nor every third; the bin
                                      changes at every record (every fifth reference: ties on one position)
      sparse_refs  n_ref              three records each on the first, the middle and the last reference"""
    if kind == "bin_changes":
        m, big, n_ref = size["m"], size["big"], size["n_ref"]
        parts = [_around_edges(_bin_change_edges(m - 7 * r, big if r == n_ref - 1 else 3)) for r in range(n_ref)]
        ref = np.concatenate([np.full(p[0].size, r, dtype=np.int64) for r, p in enumerate(parts)])
        return {"n_ref": n_ref, "ref": ref, "lo": np.concatenate([p[0] for p in parts]), "end": np.concatenate([p[1] for p in parts]), "ref_len": [TOP] * n_ref}
    if kind == "ties":
        k, p = size["k"], 5 * WINDOW + 100
        j = np.arange(k, dtype=np.int64)
        return {"n_ref": 1, "ref": np.zeros(k, dtype=np.int64), "lo": np.full(k, p, dtype=np.int64), "end": p + np.where(j % 2 == 0, 1, WINDOW + 1), "ref_len": [TOP]}
    if kind == "linear":
        ref, lo, end, ref_len = [], [], [], []
        for n_intv in size["n_intvs"]:  # the record of the last window ends on the window's last base: n_intv windows exactly
            ws = np.array(_sparse_windows(n_intv), dtype=np.int64)
            at = np.where(ws == n_intv - 1, n_intv * WINDOW - 1, ws * WINDOW + ws * 37 % WINDOW)
            ref.append(np.full(ws.size, len(ref_len), dtype=np.int64)); lo.append(at); end.append(at + 1)
            ref_len.append(n_intv * WINDOW - 1)
        ref_len.append(1000)  # (without records)
        long = size["long"]
        inside = np.array(sorted({w for w in (1, 2, 300, long - 1) if 0 < w < long}), dtype=np.int64)
        at = np.concatenate([[0], inside * WINDOW + 5, [long * WINDOW - 1]])
        ref.append(np.full(at.size, len(ref_len), dtype=np.int64)); lo.append(at)
        end.append(np.concatenate([[long * WINDOW], inside * WINDOW + 6, [long * WINDOW]]))
        ref_len.append(long * WINDOW - 1)
        return {"n_ref": len(ref_len), "ref": np.concatenate(ref), "lo": np.concatenate(lo), "end": np.concatenate(end), "ref_len": ref_len}
    if kind == "strides":
        n_ref, n = size["n_ref"], size["n"]
        used = np.array([r for r in range(1, n_ref - 1) if r % 3], dtype=np.int64)
        per = n // used.size + (np.arange(used.size) < n % used.size)
        assert per.max() // 2 + 1 < 1 << 15
        ref = np.repeat(used, per)
        j = np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)  # the record's place inside its reference
        edge = (1 + j // 2) * WINDOW
        lo = np.where(ref % 5 == 0, WINDOW - 1, edge - 2 + (j & 1))
        end = np.where(ref % 5 == 0, WINDOW + (j & 1), np.where(j & 1 == 1, edge + 1, lo + 1))
        return {"n_ref": n_ref, "ref": ref, "lo": lo, "end": end, "ref_len": [TOP] * n_ref}
    if kind == "sparse_refs":
        n_ref = size["n_ref"]
        ref = np.repeat(np.array([0, n_ref // 2, n_ref - 1], dtype=np.int64), 3)
        lo = np.tile(np.array([WINDOW - 2, WINDOW - 1, 2 * WINDOW - 2], dtype=np.int64), 3)
        return {"n_ref": n_ref, "ref": ref, "lo": lo, "end": lo + np.tile(np.array([1, 2, 1], dtype=np.int64), 3), "ref_len": None}
    raise ValueError(kind)
