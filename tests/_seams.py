"""Fast restatements of tests/_overlap.py for the sizes at which the device's scans take their second level — TEST
INFRASTRUCTURE ONLY.  tests/_overlap.py stays the reference: tests/test_seams_host.py holds both restatements to it on a few
hundred reads, and the large GPU tests (tests/test_gpu_overlap_seams.py) use them where the model's cost is quadratic.

  pair_columns / pairs_by_index   _overlap.pairs with `order` walked by index: the same rule and output order, without the copy
                                  of order[i + 1:] per read;
  record_lengths                  the bytes of every PAF record from decimal-digit counts: the digits of the ten numbers
                                  _overlap.record writes, 16 fixed bytes (eleven tabs, the strand, "255", the newline) and
                                  "/1" or "/2" behind both names of a paired run.  No line is formatted.
Nothing here comes from the code under test."""
import numpy as np

POW10 = np.array([10 ** k for k in range(1, 20)], dtype=np.uint64)


def dec_digits(v):
    """decimal digits of every entry of a non-negative integer array (0 has one)"""
    return 1 + np.searchsorted(POW10, np.asarray(v).astype(np.uint64), side="right").astype(np.int64)


def sorted_order(row, lo, hi, min_overlap):
    """the ordinals of the reads with hi - lo >= min_overlap in the order of (row, lo, ordinal) — the model's `order`"""
    row, lo, hi = (np.asarray(x, dtype=np.int64) for x in (row, lo, hi))
    keep = np.flatnonzero(hi - lo >= min_overlap)
    return keep[np.lexsort((keep, lo[keep], row[keep]))]


def pair_columns(row, lo, hi, min_overlap):
    """_overlap.pairs over columns, as five int64 arrays (a, b, ref_start, ref_end, row) in the model's order"""
    assert min_overlap >= 1
    order = sorted_order(row, lo, hi, min_overlap).tolist()
    row, lo, hi = (np.asarray(x, dtype=np.int64).tolist() for x in (row, lo, hi))
    n = len(order)
    A, B, S, E, R = [], [], [], [], []
    for i in range(n):
        a = order[i]
        row_a, lo_a, hi_a = row[a], lo[a], hi[a]
        reach = hi_a - min_overlap
        j = i + 1
        while j < n:
            b = order[j]
            lo_b = lo[b]
            if row[b] != row_a or lo_b > reach:
                break  # (sorted by lo inside a row: nobody further on reaches back far enough)
            s, e = max(lo_a, lo_b), min(hi_a, hi[b])
            if e - s >= min_overlap:
                A.append(a); B.append(b); S.append(s); E.append(e); R.append(row_a)
            j += 1
    return tuple(np.array(x, dtype=np.int64) for x in (A, B, S, E, R))


def pairs_by_index(reads, min_overlap):
    """_overlap.pairs(reads, min_overlap) for the model's own read tuples: the same list"""
    cols = pair_columns([r[0] for r in reads], [r[1] for r in reads], [r[2] for r in reads], min_overlap)
    return list(zip(*(c.tolist() for c in cols)))


def record_lengths(lo, hi, rev, read_id, a, b, s, e, paired):
    """len(_overlap.record(reads, (a, b, s, e, row))) for every pair, as an int64 array"""
    lo, hi, rev, read_id = (np.asarray(x, dtype=np.int64) for x in (lo, hi, rev, read_id))
    a, b, s, e = (np.asarray(x, dtype=np.int64) for x in (a, b, s, e))
    total = np.full(a.shape, 16 + (4 if paired else 0), dtype=np.int64)
    for r in (a, b):  # the query, then the target: id, length, start and end on the read
        start = np.where(rev[r] == 1, hi[r] - e, s - lo[r])
        total += dec_digits(read_id[r]) + dec_digits(hi[r] - lo[r]) + dec_digits(start) + dec_digits(start + (e - s))
    return total + 2 * dec_digits(e - s)
