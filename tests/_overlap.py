"""The true overlaps of include/simmr_hip.h (simmr_overlap_*) restated in plain Python — TEST INFRASTRUCTURE ONLY.

A read is (row, lo, hi, rev, read_id, mate): mate 0 for an unpaired run, else 1 or 2.  Sort by (row, lo, ordinal), a double loop
with a break, format.  Nothing here comes from the code under test."""


def reads_of(o, rows, paired, call_sizes=None):
    """the model's reads from host columns (start, end, contig, genome, read_id, flags) and {(genome, contig): row}; the mate is
    the parity of the read's index within its add call (call_sizes: reads of every add, default one add of everything)"""
    n = len(o["start"])
    first_of = []
    for m in (call_sizes or [n]):
        first_of += [len(first_of)] * m
    out = []
    for r in range(n):
        a, b = int(o["start"][r]), int(o["end"][r])
        mate = 1 + ((r - first_of[r]) & 1) if paired else 0
        out.append((rows[(int(o["genome"][r]), int(o["contig"][r]))], min(a, b), max(a, b), int(o["flags"][r]) & 1, int(o["read_id"][r]), mate))
    return out


def name(read):
    return f"{read[4]}/{read[5]}" if read[5] else str(read[4])


def pairs(reads, min_overlap):
    """[(a, b, ref_start, ref_end, row)]: ordinals of query and target, in the order of (place of the query, place of the target)"""
    assert min_overlap >= 1
    order = sorted((r for r in range(len(reads)) if reads[r][2] - reads[r][1] >= min_overlap), key=lambda r: (reads[r][0], reads[r][1], r))
    out = []
    for i, a in enumerate(order):
        row, lo_a, hi_a = reads[a][:3]
        for b in order[i + 1:]:
            if reads[b][0] != row or reads[b][1] > hi_a - min_overlap:
                break  # (sorted by lo inside a row: nobody further on reaches back far enough)
            s, e = max(lo_a, reads[b][1]), min(hi_a, reads[b][2])
            if e - s >= min_overlap:
                out.append((a, b, s, e, row))
    return out


def coords(read, s, e):
    _, lo, hi, rev = read[:4]
    return (hi - e, hi - s) if rev else (s - lo, e - lo)


def record(reads, pair):
    a, b, s, e, _ = pair
    q, t = reads[a], reads[b]
    qs, qe = coords(q, s, e)
    ts, te = coords(t, s, e)
    ov = e - s
    return "\t".join(str(x) for x in (name(q), q[2] - q[1], qs, qe, "+" if q[3] == t[3] else "-", name(t), t[2] - t[1], ts, te, ov, ov, 255)) + "\n"


def paf(reads, min_overlap):
    """(text as bytes, the pairs)"""
    ps = pairs(reads, min_overlap)
    return "".join(record(reads, p) for p in ps).encode(), ps


def brute(reads, min_overlap):
    """the unordered pairs by definition, O(n^2): {(a, b)} with a at the earlier place"""
    key = lambda r: (reads[r][0], reads[r][1], r)
    out = set()
    for a in range(len(reads)):
        for b in range(a + 1, len(reads)):
            if reads[a][0] != reads[b][0]:
                continue
            ov = min(reads[a][2], reads[b][2]) - max(reads[a][1], reads[b][1])
            if ov >= min_overlap:
                out.add((a, b) if key(a) < key(b) else (b, a))
    return out
