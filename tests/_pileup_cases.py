"""The reads and site lists of tests/test_gpu_pileup_seams.py as plain numpy columns — TEST INFRASTRUCTURE ONLY.  The GPU tests
copy them to the device; tests/test_seams_host.py runs the small ones through the plain model of tests/_pileup.py, so the shapes
are known to hold the seams they are named after before a kernel sees them.  Nothing here comes from the code under test."""
import numpy as np

BYTES = np.frombuffer(b"ACGTACGTACGTNn-acgtR", dtype=np.uint8)  # tests/test_gpu_pileup.py's alphabet: mostly bases, some of class 4
LENS = {0: [1_000_000], 1: [300_000, 90_001, 30_017, 70_000, 123_457], 3: [30_000]}  # the three genomes of test_gpu_pileup.stage_three
STRANDS = ("forward", "reverse", "alternating")


def read_columns(g, c, lo, L, rev, layout, rng, shared=False):
    """test_gpu_pileup.make_reads without its loop over reads: the host columns of reads (genome, contig, lo, L, reverse) in the
    compact layout (0) or in 16-byte slots (16, reverse reads right-aligned), every byte of seq[] drawn from BYTES.  shared:
    every read starts at byte 0 of seq[] (the pass never asks the reads' bytes to be disjoint), so equal reads are equal bytes."""
    g, c, lo, L, rev = (np.asarray(x, dtype=np.int64) for x in (g, c, lo, L, rev))
    n = L.size
    slot = (L + 15) // 16 * 16 if layout == 16 else L
    seq_off = np.zeros(n + 1, dtype=np.int64)
    if shared:
        assert layout == 0
        total = int(L.max()) if n else 0
        seq_off[n] = total
    else:
        np.cumsum(slot, out=seq_off[1:])
        total = int(seq_off[n])
        if layout == 16:
            seq_off[:n] += np.where(rev == 1, slot - L, 0)
    return {"seq": BYTES[rng.integers(0, BYTES.size, total + 16)], "seq_off": seq_off.astype(np.uint64),
            "start": np.where(rev == 1, lo + L, lo).astype(np.uint64), "end": np.where(rev == 1, lo, lo + L).astype(np.uint64),
            "contig": c.astype(np.uint32), "genome": g.astype(np.uint32), "flags": rev.astype(np.uint8), "total_bases": total,
            "layout": layout}


def site_columns(g, c, p):
    return np.asarray(g, dtype=np.uint32), np.asarray(c, dtype=np.uint32), np.asarray(p, dtype=np.uint64)


def strands(which, n):
    return {"forward": np.zeros(n, dtype=np.int64), "reverse": np.ones(n, dtype=np.int64), "alternating": np.arange(n, dtype=np.int64) & 1}[which]


# ---- (a) more reads than one trip of the grid ---------------------------------------------------------------------------------
def spread_reads(n_reads, lens, rng, lmax=40):
    """n_reads reads of L in [0, lmax) on random strands, spread over every contig of `lens` in proportion to its length"""
    slots = sorted(lens)
    g = np.array([s for s in slots for _ in lens[s]], dtype=np.int64)
    c = np.array([k for s in slots for k in range(len(lens[s]))], dtype=np.int64)
    n = np.array([x for s in slots for x in lens[s]], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(n)])
    x = rng.integers(0, first[-1], n_reads)
    row = np.searchsorted(first, x, side="right") - 1
    L = np.minimum(rng.integers(0, lmax, n_reads), n[row])
    lo = np.minimum(x - first[row], n[row] - L)  # (a read that would leave its contig ends at the contig's last base)
    return g[row], c[row], lo, L, rng.integers(0, 2, n_reads)


def every_kth_position(lens, k=13):
    slots = sorted(lens)
    cols = [(np.full(-(-n // k), s), np.full(-(-n // k), ci), np.arange(0, n, k)) for s in slots for ci, n in enumerate(lens[s])]
    return site_columns(*(np.concatenate([x[i] for x in cols]) for i in range(3)))


# ---- (d) the 64-pair steps of the expansion -----------------------------------------------------------------------------------
def _lanes(pairs):
    v = np.zeros(64, dtype=np.int64)
    for lane, n in pairs:
        v[lane] = n
    return v


STEP_COUNTS = {
    "edges_64_128_256": _lanes([(0, 64), (3, 1), (4, 63), (5, 128), (8, 65)]),      # prefixes 64, 65, 128, 256, 321; 55 zero lanes behind
    "edges_reversed": _lanes([(0, 64), (3, 1), (4, 63), (5, 128), (8, 65)])[::-1].copy(),  # lane 63 has the first 64, 55 zero lanes in front
    "all_64": np.full(64, 64, dtype=np.int64),                                       # 4096 pairs: 64 full steps, a read per step
    "lane_63_one": _lanes([(63, 1)]),
    "lane_0_65": _lanes([(0, 65)]),
    "lanes_31_32": _lanes([(31, 100), (32, 93)]),                                    # 64 * 3 + 1 pairs across the row-broadcast seam
}
STEP_WINDOW, STEP_L = 400, 200


def step_case(name, which):
    """Three waves of reads on contig 0 of slot 0, one disjoint window of STEP_WINDOW positions per read: the count vector, 64
    reads that cover no site, the count vector again on other windows.  Read k lies at its window's position 20 with L = STEP_L
    and covers exactly counts[k % 64] sites on consecutive positions — at its first bases, at its last ones or in between, by
    k % 3; every other window also has a site in front of its read that no read covers.
    -> (g, c, lo, L, rev), sites, the 192 counts"""
    counts = np.concatenate([STEP_COUNTS[name], np.zeros(64, dtype=np.int64), STEP_COUNTS[name]])
    k = np.arange(192, dtype=np.int64)
    lo = 1000 + STEP_WINDOW * k + 20
    free = STEP_L - counts
    assert (free >= 0).all()
    at = lo + np.where(k % 3 == 0, 0, np.where(k % 3 == 1, free, (k * 37) % (free + 1)))
    covered = np.repeat(at, counts) + (np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts))
    pos = np.sort(np.concatenate([covered, lo[k % 2 == 0] - 15]))
    zero = np.zeros(192, dtype=np.int64)
    return (zero, zero, lo, np.full(192, STEP_L), strands(which, 192)), site_columns(np.zeros(pos.size), np.zeros(pos.size), pos), counts


# ---- (e) the ends of the site list --------------------------------------------------------------------------------------------
END_L, END_LO, END_AT = 150, 40_000, (1, 1)  # contig 1 of slot 1: 90 001 positions


def _both_strands(windows):
    lo = np.repeat(np.array([w[0] for w in windows], dtype=np.int64), 2)
    L = np.repeat(np.array([w[1] for w in windows], dtype=np.int64), 2)
    n = lo.size
    return np.full(n, END_AT[0]), np.full(n, END_AT[1]), lo, L, np.arange(n, dtype=np.int64) & 1


def list_end_case(m, before):
    """`before` sites in front of END_LO, then m on consecutive positions from END_LO: the list ends m sites behind the first
    site of a read at END_LO.  Reads 0 and 1 are that read, forward and reverse; then, on both strands: one wholly below the
    first site and one wholly above the last, one that covers the whole list, one that starts in the middle of the run, one that
    ends where the run starts, one on the run's last site alone and one that starts behind it."""
    lo = END_LO
    pos = np.concatenate([lo - np.array([40, 39, 37])[:before], lo + np.arange(m)])
    windows = [(lo, END_L), (lo - 400, END_L), (lo + 400, END_L), (lo - 100, 600), (lo + 75, END_L), (lo - END_L, END_L), (lo + m - 1, END_L), (lo + m, END_L)]
    return _both_strands(windows), site_columns(np.full(pos.size, END_AT[0]), np.full(pos.size, END_AT[1]), pos)


def short_list_case(pos):
    """a list of one or two sites, the first at END_LO, and on both strands: reads that start and end on the first site and
    beside it, reads below and above the list, one that covers it whole, one of L = 1 on the site and one of L = 0"""
    p = END_LO
    assert pos[0] == p and len(pos) in (1, 2)
    windows = [(p, END_L), (p - END_L + 1, END_L), (p - END_L, END_L), (p + 1, END_L), (p - 400, END_L), (p + 400, END_L), (p - 100, 600), (p, 1), (p, 0)]
    return _both_strands(windows), site_columns(np.full(len(pos), END_AT[0]), np.full(len(pos), END_AT[1]), pos)


# ---- (c) one deep column --------------------------------------------------------------------------------------------------------
DEEP_P, DEEP_L, DEEP_AT = 50_000, 20, (1, 4)


def deep_case(n_reads, identical, rng):
    """n_reads reads of L = DEEP_L that all cover position DEEP_P: on alternating strands with the site on every offset of a
    read, or (identical) one read n_reads times.  Sites: DEEP_P, DEEP_P -+ 19 (under some of the reads) and DEEP_P -+ 20 (under none)."""
    n = n_reads
    lo = np.full(n, DEEP_P - 7) if identical else DEEP_P - rng.integers(0, DEEP_L, n)
    rev = np.ones(n, dtype=np.int64) if identical else np.arange(n, dtype=np.int64) & 1
    pos = DEEP_P + np.array([-20, -19, 0, 19, 20])
    return (np.full(n, DEEP_AT[0]), np.full(n, DEEP_AT[1]), lo, np.full(n, DEEP_L), rev), site_columns(np.full(5, DEEP_AT[0]), np.full(5, DEEP_AT[1]), pos)
