"""Fast restatements of tests/_overlap.py for the sizes at which the device's scans take their second level — TEST
INFRASTRUCTURE ONLY.  tests/_overlap.py stays the reference: tests/test_seams_host.py holds both restatements to it on a few
hundred reads, and the large GPU tests (tests/test_gpu_overlap_seams.py) use them where the model's cost is quadratic.

  pair_columns / pairs_by_index   _overlap.pairs with `order` walked by index: the same rule and output order, without the copy
                                  of order[i + 1:] per read;
  record_lengths                  the bytes of every PAF record from decimal-digit counts: the digits of the ten numbers
                                  _overlap.record writes, 16 fixed bytes (eleven tabs, the strand, "255", the newline) and
                                  "/1" or "/2" behind both names of a paired run.  No line is formatted.
And a fast restatement of tests/_bai.py for the sizes at which the index kernels leave their first tile, chunk and grid trip
(tests/test_gpu_bai_seams.py), held to _bai.bai_bytes byte for byte by tests/test_seams_host.py:

  bai_from_columns                _bai.bai_bytes from the columns (reference, lo, end, offset) instead of record bytes, with numpy
                                  over all records, runs, bins, references and windows at once: the rules of include/simmr_hip.h
                                  (simmr_bai_plan), no loop over references times records.
Nothing here comes from the code under test."""
import numpy as np

POW10 = np.array([10 ** k for k in range(1, 20)], dtype=np.uint64)
BGZF_BLOCK, BGZF_FRAMED = 65280, 65311  # source bytes of a full block, and its bytes in the file
BAI_META_BIN = 37450
BAI_WINDOW_BITS = 14
BAI_LEVELS = ((1, 26), (9, 23), (73, 20), (585, 17), (4681, 14))  # (first bin, shift) of levels 1 to 5; level 0 is bin 0


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


# ---- the BAI index from columns ---------------------------------------------------------------------------------------------
def virtual_offsets(p):
    """_bai.voff of every entry of an array of uncompressed positions, as uint64"""
    p = np.asarray(p).astype(np.uint64)
    blk = p // np.uint64(BGZF_BLOCK)
    return ((blk * np.uint64(BGZF_FRAMED)) << np.uint64(16)) | (p - blk * np.uint64(BGZF_BLOCK))


def bins_of(lo, end):
    """reg2bin (SAM spec 5.3) of every [lo, end): the smallest bin that holds the interval, coarse levels first so a finer one wins"""
    last = end - 1
    out = np.zeros(lo.shape, dtype=np.int64)
    for first, shift in BAI_LEVELS:
        out = np.where(lo >> shift == last >> shift, first + (lo >> shift), out)
    return out


def bin_level(b):
    """the level (0: the whole 2^29, 5: a 16 Kbase leaf) of every bin number"""
    return np.searchsorted(np.array([first for first, _ in BAI_LEVELS], dtype=np.int64), np.asarray(b, dtype=np.int64), side="right")


def _put64(words, at, v):
    """the uint64 values v at the 32-bit word indices `at` of a little-endian file held as uint32 words"""
    v = np.asarray(v).astype(np.uint64)
    words[at] = (v & np.uint64(0xffffffff)).astype(np.uint32)
    words[at + 1] = (v >> np.uint64(32)).astype(np.uint32)


def bai_from_columns(n_ref, ref, lo, end, rec_off, base, counts=None):
    """_bai.bai_bytes(n_ref, records, base) for n records given as columns: their reference, their interval [lo, end) and
    rec_off[0 .. n], the offsets of the records behind the `base` bytes of the header (rec_off[n]: the stream's length).  The
    records ascend by (ref, lo).  A dict given as `counts` is filled with what the index holds: n_runs (chunks of real bins),
    n_bins, max_chunks (of one bin), bins (the bin numbers, per reference ascending), n_intv (per reference)."""
    ref, lo, end, rec_off = (np.asarray(x, dtype=np.int64) for x in (ref, lo, end, rec_off))
    n = ref.size
    assert lo.size == n and end.size == n and rec_off.size == n + 1
    assert n == 0 or (0 <= ref.min() and ref.max() < n_ref and (lo >= 0).all() and (end > lo).all() and end.max() <= 1 << 29)
    sort_key = (ref << 40) | lo
    assert (np.diff(sort_key) >= 0).all() and (np.diff(rec_off) >= 0).all(), "the records are not sorted"
    at_voff = virtual_offsets(np.uint64(base) + rec_off.astype(np.uint64))  # of every record's start, and of the end behind the last

    # the chunks: maximal runs of consecutive records of one (reference, bin); a bin's chunks stay in file order
    rb = (ref << 16) | bins_of(lo, end)
    run_first = np.flatnonzero(np.concatenate([[True], rb[1:] != rb[:-1]])) if n else np.zeros(0, dtype=np.int64)
    run_end = np.concatenate([run_first[1:], [n]]) if n else run_first
    order = np.argsort(rb[run_first], kind="stable")
    bin_key, bin_run0, bin_chunks = np.unique(rb[run_first][order], return_index=True, return_counts=True)
    n_runs, n_bins = run_first.size, bin_key.size

    # per reference: its records, its bins, its chunks, its windows
    every = np.arange(n_ref + 1, dtype=np.int64)
    rec0 = np.searchsorted(ref, every)
    bin0 = np.searchsorted(bin_key >> 16, every)
    n_rec, ref_bins = np.diff(rec0), np.diff(bin0)
    chunks_before = np.concatenate([[0], np.cumsum(bin_chunks)])
    ref_chunks = chunks_before[bin0[1:]] - chunks_before[bin0[:-1]]
    max_end = np.zeros(n_ref, dtype=np.int64)
    np.maximum.at(max_end, ref, end)
    has = n_rec > 0
    n_intv = np.where(has, 1 + ((max_end - 1) >> BAI_WINDOW_BITS), 0)

    # the layout in 32-bit words: n_bin, the bins (number, n_chunk, 16 bytes a chunk), bin 37450 (40 bytes), n_intv, the windows
    ref_words = np.where(has, 1 + 2 * ref_bins + 4 * ref_chunks + 10 + 1 + 2 * n_intv, 2)
    ref_at = 2 + np.concatenate([[0], np.cumsum(ref_words)])
    words = np.zeros(int(ref_at[n_ref]) + 2, dtype=np.uint32)  # (the two behind: n_no_coor = 0)
    words[0], words[1] = 0x01494142, n_ref  # "BAI\1"
    used = np.flatnonzero(has)
    words[ref_at[used]] = ref_bins[used] + 1

    bin_ref = bin_key >> 16
    bin_words = 2 + 4 * bin_chunks
    words_before = np.concatenate([[0], np.cumsum(bin_words)])
    bin_at = ref_at[bin_ref] + 1 + words_before[:-1] - words_before[bin0[bin_ref]]
    words[bin_at] = bin_key & 0xffff
    words[bin_at + 1] = bin_chunks
    run_bin = np.repeat(np.arange(n_bins), bin_chunks)  # of every run in (reference, bin) order
    chunk_at = bin_at[run_bin] + 2 + 4 * (np.arange(n_runs) - bin_run0[run_bin])
    _put64(words, chunk_at, at_voff[run_first[order]])
    _put64(words, chunk_at + 2, at_voff[run_end[order]])

    meta_at = ref_at[:-1] + 1 + 2 * ref_bins + 4 * ref_chunks  # (meaningful for the references with records)
    m = meta_at[used]
    words[m], words[m + 1] = BAI_META_BIN, 2
    _put64(words, m + 2, at_voff[rec0[used]])
    _put64(words, m + 4, at_voff[rec0[used + 1]])
    _put64(words, m + 6, n_rec[used])
    words[m + 10] = n_intv[used]

    # the linear index over all references' windows laid end to end: the smallest start of a record that overlaps the window,
    # a window without one shows the last one before it that has, inside its reference (0 at the front)
    win0 = np.concatenate([[0], np.cumsum(n_intv)])
    n_win = int(win0[n_ref])
    w_first, w_last = lo >> BAI_WINDOW_BITS, (end - 1) >> BAI_WINDOW_BITS
    span = w_last - w_first + 1
    who = np.repeat(np.arange(n), span)
    where = win0[ref[who]] + w_first[who] + np.arange(int(span.sum())) - np.repeat(np.cumsum(span) - span, span)
    smallest = np.full(n_win, np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(smallest, where, at_voff[who])
    filled = smallest != np.iinfo(np.uint64).max
    last = np.maximum.accumulate(np.where(filled, np.arange(n_win), -1)) if n_win else np.zeros(0, dtype=np.int64)
    win_ref = np.repeat(np.arange(n_ref), n_intv)
    shown = np.where(last >= win0[win_ref], smallest[np.maximum(last, 0)], np.uint64(0)) if n_win else smallest
    _put64(words, meta_at[win_ref] + 11 + 2 * (np.arange(n_win) - win0[win_ref]), shown)

    if counts is not None:
        counts.update(n_runs=n_runs, n_bins=n_bins, max_chunks=int(bin_chunks.max()) if n_bins else 0, bins=bin_key & 0xffff, n_intv=n_intv)
    return words.astype("<u4").tobytes()
