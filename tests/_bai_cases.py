"""Shapes for the sorted BAM and its index (tests/test_bai_host.py, tests/test_gpu_bam_sorted.py): hand-built read columns on a
names set whose first contig passes 2^20 bases, the records of tests/_bam.py in coordinate order, and the file around them."""
import numpy as np

from simmr_amd.sam import BGZF_EOF, bam_header
from tests import _bam

SLOTS = {0: [1_100_000], 1: [3000, 901, 317], 3: [4000]}
RNAMES = [(s, [f"g{s}.c{c}|x" for c in range(len(SLOTS[s]))]) for s in SLOTS]
REFS = [(n, SLOTS[s][c]) for s, ns in RNAMES for c, n in enumerate(ns)]
CONTIGS = [(s, c) for s in SLOTS for c in range(len(SLOTS[s]))]
WINDOW = 1 << 14


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
