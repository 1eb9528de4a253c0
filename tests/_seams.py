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
And a fast restatement of tests/_mapeval.py for the sizes at which the mapeval kernels take their second grid trips
(tests/test_gpu_mapeval_seams.py), held to _mapeval.evaluate table for table by tests/test_seams_host.py:

  mapeval_from_columns            both SAM texts and every table of _mapeval.evaluate from columns (read id, mate, strand, name
                                  row, pos, span; on the aligned side also MAPQ and flag bits) instead of lines: the texts as
                                  byte matrices, the tables with searchsorted, bincount and maximum.at.  No loop over lines.
And a fast restatement of tests/_pileup.py for the sizes at which k_pileup_add takes its second grid trip and its second scan
round (tests/test_gpu_pileup_seams.py), held to _pileup.site_keys and _pileup.pileup cell for cell by tests/test_seams_host.py:

  pileup_keys                     _pileup.site_keys with a (slot, contig) -> first table and one gather, under the same assertions.
                                  No loop over sites.
  pileup_from_columns             _pileup.pileup from the same columns: two searchsorted calls over all reads, the (read, site)
                                  pairs laid out with repeat, one bincount over site * 10 + strand * 5 + class per chunk of
                                  pairs (a chunk may end inside a read; `unique` instead where a chunk's few pairs lie far
                                  apart).  No loop over reads or sites.
Nothing here comes from the code under test."""
import numpy as np

from tests import _pileup

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


# ---- mapeval from columns ---------------------------------------------------------------------------------------------------
MEV_STAR = -1  # a name row: RNAME "*", POS 0 and CIGAR "*" (unmapped without the flag)
MEV_COUNTS = ("truth_lines", "truth_header", "truth_entries", "truth_skipped", "lines", "header", "records", "secondary", "cigar_op",
              "unknown_read", "unknown_ref", "unmapped", "correct", "wrong", "missing", "multiple", "reads_correct", "reads_wrong",
              "reads_unmapped")
MEV_TAIL = b"\t*\t0\t0\t*\t*\n"


def _column(cols, name, n, default=None):
    v = cols.get(name, default)
    assert v is not None, name
    return np.broadcast_to(np.asarray(v, dtype=np.int64), (n,))


def _put_number(mat, at, width, v, pad):
    """v in decimal, right-aligned in mat[:, at : at + width]: the places in front hold '0' (pad) or NUL"""
    v = v.astype(np.uint64)
    shown = dec_digits(v)
    assert (shown <= width).all()
    for j in range(width):  # (over the places of a number, not over the lines)
        place = ((v // np.uint64(10 ** j)) % np.uint64(10) + np.uint64(48)).astype(np.uint8)
        if not pad:
            place[shown <= j] = 0
        mat[:, at + width - 1 - j] = place


def mapeval_text(names, qid, flag, row, pos, mapq, span, pad, header=b""):
    """The SAM text of n records `<id> <flag> <name> <pos> <mapq> <span>M * 0 0 * *` as a byte matrix: every field right-aligned
    in a slot as wide as the column's widest value.  pad: the numbers are filled up with zeros in front (they stay the same
    numbers under the rules) and a text whose names have one length is the matrix itself, all lines of one width; otherwise, and
    for the names and the "*" of a row MEV_STAR always, the slot's front is NUL and the NULs are taken out of the text."""
    n = qid.size
    table = [bytes(x) for x in names] + [b"*"]  # (row -1, MEV_STAR, is the last)
    w_name = max(len(x) for x in table)
    name_mat = np.zeros((len(table), w_name), dtype=np.uint8)
    for r, x in enumerate(table):  # (over the names, not over the lines)
        name_mat[r, w_name - len(x):] = np.frombuffer(x, dtype=np.uint8)
    star = row == MEV_STAR
    assert ((row >= -1) & (row < len(names))).all() and (pos[star] == 0).all() and (pos[~star] >= 1).all() and (span <= 999_999_999).all()
    width = lambda v: int(dec_digits(np.array([int(v.max()) if n else 0], dtype=np.uint64))[0])
    w_id, w_flag, w_pos, w_mapq, w_span = width(qid), width(flag), width(pos), width(mapq), width(span)
    p_flag = w_id + 1  # every slot is followed by a tab, the span's by its op
    p_name = p_flag + w_flag + 1
    p_pos = p_name + w_name + 1
    p_mapq = p_pos + w_pos + 1
    p_span = p_mapq + w_mapq + 1
    p_tail = p_span + w_span + 1
    mat = np.full((n, p_tail + len(MEV_TAIL)), 9, dtype=np.uint8)  # (9: a tab)
    for p, w, v in ((0, w_id, qid), (p_flag, w_flag, flag), (p_pos, w_pos, pos), (p_mapq, w_mapq, mapq), (p_span, w_span, span)):
        _put_number(mat, p, w, v, pad)
    mat[:, p_name:p_name + w_name] = name_mat[row]
    mat[:, p_tail - 1] = ord("M")
    mat[star, p_span:p_tail - 1] = 0  # CIGAR "*"
    mat[star, p_tail - 1] = ord("*")
    mat[:, p_tail:] = np.frombuffer(MEV_TAIL, dtype=np.uint8)
    return header + (mat.tobytes() if mat.all() else mat[mat != 0].tobytes())


def mapeval_from_columns(names, truth, aligned, pct=10, pad=True, header=b"", n_present=None):
    """_mapeval.evaluate(names[:n_present], [truth text], [aligned text], pct) from columns: a dict with both texts ("truth",
    "aligned": `header`, then a record per entry of the columns), "counts", "by_mapq", "key", "best" and "hits".
      truth    id, mate (1 or 2: FLAG 0x40 or 0x80, and bit 0 of the key), strand, row, pos, span [, mapq: 255];
      aligned  the same and mapq and bits (0x4, 0x100, 0x800: or-ed into FLAG).
    A row is an index into `names`; the names from n_present on are not in the table (an unknown reference; aligned side only);
    MEV_STAR on the aligned side is RNAME "*".  A read is unknown when its (id, mate) is not in the truth.  A value given as a
    scalar holds for every record.  The truth's keys are unique, every truth record is an entry, CIGAR is `<span>M`."""
    n_present = len(names) if n_present is None else n_present
    assert len(set(names)) == len(names) and b"*" not in names
    nt, na = np.asarray(truth["id"]).size, np.asarray(aligned["id"]).size
    t = {k: _column(truth, k, nt, d) for k, d in (("id", None), ("mate", None), ("strand", None), ("row", None), ("pos", None), ("span", None), ("mapq", 255))}
    a = {k: _column(aligned, k, na, d) for k, d in (("id", None), ("mate", None), ("strand", None), ("row", None), ("pos", None), ("span", None), ("mapq", None), ("bits", 0))}
    for c in (t, a):
        assert ((c["mate"] == 1) | (c["mate"] == 2)).all() and ((c["strand"] | 1) == 1).all() and (c["id"] >= 0).all() and (c["mapq"] >> 8 == 0).all()
    assert ((t["row"] >= 0) & (t["row"] < n_present)).all() and (a["bits"] & ~0x904 == 0).all()
    flag_of = lambda c: np.where(c["mate"] == 2, 0x80, 0x40) | c["strand"] << 4
    head_lines = sum(1 for ln in header.split(b"\n") if ln)
    assert all(ln[:1] == b"@" for ln in header.split(b"\n") if ln) and (not header or header.endswith(b"\n"))
    out = dict(truth=mapeval_text(names, t["id"], flag_of(t), t["row"], t["pos"], t["mapq"], t["span"], pad, header),
               aligned=mapeval_text(names, a["id"], flag_of(a) | a["bits"], a["row"], a["pos"], a["mapq"], a["span"], pad, header))

    key_of = lambda c: (c["id"].astype(np.uint64) << np.uint64(1)) | (c["mate"] == 2).astype(np.uint64)
    t_key = key_of(t)
    order = np.argsort(t_key, kind="stable")
    key = t_key[order]
    assert (key[1:] != key[:-1]).all(), "two truth records with one key"
    t_row, t_strand, t_lo, t_hi = t["row"][order], t["strand"][order], (t["pos"] - 1)[order], (t["pos"] - 1 + t["span"])[order]

    secondary = a["bits"] & 0x900 != 0
    at = np.searchsorted(key, key_of(a))
    at_in = np.minimum(at, max(nt - 1, 0))
    found = ~secondary & (at < nt) & (key[at_in] == key_of(a) if nt else False)
    unmapped = found & ((a["bits"] & 4 != 0) | (a["row"] == MEV_STAR))
    mapped = found & ~unmapped
    unknown_ref = mapped & (a["row"] >= n_present)
    lo, hi = a["pos"] - 1, a["pos"] - 1 + a["span"]
    if nt:
        tl, th = t_lo[at_in], t_hi[at_in]
        ov = np.maximum(0, np.minimum(hi, th) - np.maximum(lo, tl))
        un = np.maximum(hi, th) - np.minimum(lo, tl)
        correct = mapped & ~unknown_ref & (a["row"] == t_row[at_in]) & (a["strand"] == t_strand[at_in]) & (ov >= 1) & (100 * ov >= pct * un)
    else:
        correct = np.zeros(na, dtype=bool)
    wrong = mapped & ~correct
    cls = np.where(unmapped, 1, np.where(correct, 3, 2))
    best = np.zeros(nt, dtype=np.uint32)
    np.maximum.at(best, at[found], (cls[found] << 8 | a["mapq"][found]).astype(np.uint32))
    hits = np.bincount(at[found], minlength=nt).astype(np.uint32)
    by_mapq = np.bincount(2 * a["mapq"][mapped] + wrong[mapped], minlength=512).astype(np.uint64).reshape(256, 2)
    counts = dict.fromkeys(MEV_COUNTS, 0)
    counts.update(truth_lines=head_lines + nt, truth_header=head_lines, truth_entries=nt, lines=head_lines + na, header=head_lines, records=na,
                  secondary=int(secondary.sum()), unknown_read=int((~secondary & ~found).sum()), unknown_ref=int(unknown_ref.sum()),
                  unmapped=int(unmapped.sum()), correct=int(correct.sum()), wrong=int(wrong.sum()), missing=int((hits == 0).sum()),
                  multiple=int((hits > 1).sum()), reads_correct=int((best >> 8 == 3).sum()), reads_wrong=int((best >> 8 == 2).sum()),
                  reads_unmapped=int((best >> 8 == 1).sum()))
    out.update(counts=counts, by_mapq=by_mapq, key=key, best=best, hits=hits)
    return out


# ---- the pileup from columns ------------------------------------------------------------------------------------------------
def pileup_layout(lens):
    """lens: {genome slot: [contig lengths]} -> (first, length), int64 tables indexed [slot, contig]: slots ascending, contigs in
    order, no padding; first is -1 where there is no contig"""
    n_slots = max(lens) + 1 if lens else 0
    width = max((len(v) for v in lens.values()), default=0)
    first, length = np.full((n_slots, width), -1, dtype=np.int64), np.zeros((n_slots, width), dtype=np.int64)
    at = 0
    for g in sorted(lens):  # (over the contigs, not over sites or reads)
        for c, n in enumerate(lens[g]):
            first[g, c], length[g, c] = at, int(n)
            at += int(n)
    return first, length


def _first_of(first, g, c):
    """first[g, c] of every entry, after the assertion that the slot is staged and the contig exists"""
    assert ((g >= 0) & (g < first.shape[0]) & (c >= 0) & (c < first.shape[1])).all(), "a slot or contig beyond the table"
    f = first[g, c]
    assert (f >= 0).all(), "a slot that is not staged or a contig that does not exist"
    return f


def pileup_keys(sites, lens):
    """_pileup.site_keys(sites, lens): int64 keys first(slot, contig) + pos, under the same assertions"""
    first, length = pileup_layout(lens)
    g, c, p = (np.asarray(x).astype(np.int64) for x in sites)
    assert g.shape == c.shape == p.shape
    k = _first_of(first, g, c) + p
    assert ((p >= 0) & (p < length[g, c])).all(), "a position outside its contig"
    assert (np.diff(k) > 0).all(), "sites are strictly ascending by (slot, contig, pos)"
    return k


def pileup_from_columns(cols, sites, lens, chunk_pairs=1 << 24, seq_base=0, keys=None):
    """_pileup.pileup(cols, sites, lens) as uint32[n, 2, 5].  cols["seq"] may be the tail of the device's buffer that starts at
    byte `seq_base` of it: seq_off counts from the buffer's start.  The pairs are taken `chunk_pairs` at a time, so the host's
    memory is bounded by the chunk whatever a read's length.  keys: pileup_keys(sites, lens) where the caller has them already."""
    assert chunk_pairs >= 1
    first, _ = pileup_layout(lens)
    keys = pileup_keys(sites, lens) if keys is None else keys
    n_reads = len(cols["start"])
    col = lambda name: np.asarray(cols[name])[:n_reads].astype(np.int64)
    a, b, rev = col("start"), col("end"), col("flags") & _pileup.REVCOMP
    lo, L = np.minimum(a, b), np.abs(b - a)
    klo = _first_of(first, col("genome"), col("contig")) + lo
    s0 = np.searchsorted(keys, klo, side="left")
    n_pairs = np.searchsorted(keys, klo + L, side="left") - s0
    off = col("seq_off") - int(seq_base)
    seq = np.asarray(cols["seq"])
    has = n_pairs > 0
    assert (off[has] >= 0).all() and (off[has] + L[has] <= seq.size).all(), "a read's bytes outside the part of seq[] given"
    end = np.cumsum(n_pairs)  # pair q of all belongs to the read with begin <= q < end
    begin = end - n_pairs
    observed = np.stack([_pileup.CLASS, np.where(_pileup.CLASS < 4, 3 - _pileup.CLASS, 4)])  # [strand, byte]: a reverse read's class is complemented
    cell_of = observed + np.array([[0], [5]])
    flat = np.zeros(keys.size * 10, dtype=np.uint32)
    for q0 in range(0, int(end[-1]) if n_reads else 0, chunk_pairs):  # (over chunks of pairs)
        q1 = min(q0 + chunk_pairs, int(end[-1]))
        some = np.arange(np.searchsorted(end, q0, side="right"), np.searchsorted(begin, q1, side="left"))
        take = np.maximum(np.minimum(end[some], q1) - np.maximum(begin[some], q0), 0)
        of_read = lambda v: np.repeat(v[some], take)  # a column of the reads, pair by pair
        s = np.arange(q0, q1) + of_read(s0 - begin)
        d = keys[s] - of_read(klo)  # pos - lo
        strand = of_read(rev)
        j = np.where(strand == 1, of_read(L - 1) - d, d)
        cell = s * 10 + cell_of[strand, seq[of_read(off) + j]]
        at = int(cell.min())
        if int(cell.max()) - at < 16 * cell.size:  # one bincount over the cells the chunk spans
            k = np.bincount(cell - at)
            flat[at:at + k.size] += k.astype(np.uint32)
        else:  # a few pairs spread over a long list: the span is not worth an array
            at, k = np.unique(cell, return_counts=True)
            flat[at] += k.astype(np.uint32)
    return flat.reshape(keys.size, 2, 5)
