"""The hand-made cases of tests/test_gpu_mapeval_seams.py — TEST INFRASTRUCTURE ONLY.  A case of columns is what
tests/_seams.py:mapeval_from_columns takes (names, n_present, truth, aligned, and what the case promises about itself); tests/
test_seams_host.py runs every one at a small size against the plain model, the GPU tests at the sizes of the kernels' seams.
A case of text (the lane rounds, the limits) is lines for tests/_mapeval.py:evaluate.  Nothing here comes from the code under test."""
import math

import numpy as np

from tests._seams import MEV_STAR

ABC = [b"a", b"b", b"c", b"d"]  # the table is a, b, c; d is a reference nobody has
KINDS = ("correct", "wrong_pos", "wrong_strand", "wrong_contig", "unknown_ref", "unmapped_flag", "unmapped_star", "unknown_read", "secondary",
         "supplementary")


def _shuffled(cols, seed):
    n = max(np.asarray(v).size for v in cols.values())
    order = np.random.default_rng(seed).permutation(n)
    return {k: (np.asarray(v)[order] if np.asarray(v).ndim else v) for k, v in cols.items()}


def _cat(*parts):
    """columns laid end to end; a scalar holds for its whole part"""
    n = [np.asarray(p["id"]).size for p in parts]
    return {k: np.concatenate([np.broadcast_to(np.asarray(p.get(k, 0), dtype=np.int64), (m,)) for p, m in zip(parts, n)]) for k in parts[0]}


def entry_columns(eid):
    """what a truth entry is, from its id alone (the cases' entries are all mate 1 unless they say otherwise)"""
    eid = np.asarray(eid, dtype=np.int64)
    return dict(id=eid, mate=1, strand=(eid >> 1) & 1, row=eid % 3, pos=1 + eid % 9000, span=100)


def records_of_kind(eid, kind, mapq, stranger):
    """an aligned record per entry id of the given kind (an index into KINDS, per record); `stranger`: ids no entry has"""
    e = entry_columns(eid)
    kind = np.asarray(kind, dtype=np.int64)
    is_ = lambda name: kind == KINDS.index(name)
    row = np.where(is_("wrong_contig"), (e["row"] + 1) % 3, np.where(is_("unknown_ref"), 3, np.where(is_("unmapped_star"), MEV_STAR, e["row"])))
    pos = np.where(is_("unmapped_star"), 0, e["pos"] + np.where(is_("wrong_pos"), 5000, np.where(is_("correct"), e["id"] % 7, 0)))
    bits = np.where(is_("unmapped_flag"), 4, np.where(is_("secondary"), 0x100, np.where(is_("supplementary"), 0x800, 0)))
    return dict(id=np.where(is_("unknown_read"), stranger, e["id"]), mate=1, strand=e["strand"] ^ is_("wrong_strand"), row=row, pos=pos, span=100,
                mapq=np.asarray(mapq, dtype=np.int64), bits=bits)


# ---- the search ------------------------------------------------------------------------------------------------------------------
def search(n, seed=1):
    """entries 3 i + 1; a record for every entry, for the ids on both sides of it, for id 0, for an id behind the last, and for
    mate 2 of every 7th entry"""
    i = np.arange(n, dtype=np.int64)
    tid = 3 * i + 1
    truth = dict(id=tid, mate=1, strand=i & 1, row=i % 3, pos=1 + (i * 7) % 1000, span=50)
    own = dict(truth, mapq=i % 256, bits=0)
    gaps = dict(id=np.concatenate([tid - 1, tid + 1, [3 * n + 5]]), mate=1, strand=0, row=0, pos=1, span=50, mapq=9, bits=0)
    other_mate = dict(id=tid[::7], mate=2, strand=0, row=0, pos=1, span=50, mapq=9, bits=0)
    assert gaps["id"].min() == 0
    return dict(names=ABC, n_present=3, truth=truth, aligned=_shuffled(_cat(own, gaps, other_mate), seed), absent=2 * n + 1 + tid[::7].size,
                mapq=(i % 256).astype(np.uint32))


# ---- the second trips ------------------------------------------------------------------------------------------------------------
def trips(n, edge, grid_lines, extra=300, tail=300):
    """n entries 0 .. n - 1 (entry e is the e-th key) in a scattered order of lines; grid_lines + extra aligned records: record
    j and record j + grid_lines are of one kind and one MAPQ (j % 256: every MAPQ twice in one workgroup where grid_lines is
    16 x the grid); the first 3000 go to an entry three at a time, a record of the second trip in four goes where the record
    grid_lines before it went; records 1 .. 6 go to the last entry, to the four around `edge`, and to entry 0, the 2 x tail
    records behind them to the last `tail` entries."""
    mult = 1_000_003
    while math.gcd(mult, n) != 1:
        mult += 2
    truth = entry_columns((np.arange(n, dtype=np.int64) * mult) % n)
    m = grid_lines + extra
    j = np.arange(m, dtype=np.int64)
    r = j % grid_lines
    kind = (r + r // 256) % len(KINDS)
    x = np.where((j >= grid_lines) & (r % 4 == 0), r, j)
    x = np.where(j < 3000, j - j % 3, x)
    target = (x * max(n // (m + 1), 1)) % n
    special = np.array([n - 1, edge - 2, edge - 1, edge, edge + 1, 0], dtype=np.int64) % n
    target[1:7] = special
    tail = min(tail, n)
    k = np.arange(2 * tail)[:m - 7]
    target[7:7 + 2 * tail] = n - 1 - (k + 3 * (k // tail)) % tail  # the last `tail` entries twice each, by records of two kinds
    aligned = records_of_kind(target, kind, r % 256, n + j)
    return dict(names=ABC, n_present=3, truth=truth, aligned=aligned, special=special, kind=kind, mapq=r % 256)


# ---- every MAPQ in both columns -----------------------------------------------------------------------------------------------------
def every_mapq(seed=3):
    """100 entries; for every MAPQ q, 1 + q % 5 correct records and 1 + q % 3 wrong ones of four kinds"""
    q = np.arange(256, dtype=np.int64)
    right, wrong = np.repeat(q, 1 + q % 5), np.repeat(q, 1 + q % 3)
    truth = entry_columns(10 + 3 * np.arange(100, dtype=np.int64))
    a = records_of_kind(truth["id"][np.arange(right.size) % 100], 0, right, 0)
    b = records_of_kind(truth["id"][(7 * np.arange(wrong.size)) % 100], 1 + np.arange(wrong.size) % 4, wrong, 0)
    return dict(names=ABC, n_present=3, truth=truth, aligned=_shuffled(_cat(a, b), seed), right=1 + q % 5, wrong=1 + q % 3)


# ---- one entry, many records ---------------------------------------------------------------------------------------------------------
def many_records(which, m=40_000, seed=4):
    """entry 37 of a hundred gets m records: `all`: unmapped at MAPQ 255, wrong at 200 and correct at 0 .. 17 in turn; `no_correct`:
    the correct ones are wrong too; `unmapped`: all unmapped, at every MAPQ.  Every second other entry gets one correct record."""
    truth = entry_columns(2 + 5 * np.arange(100, dtype=np.int64))
    j = np.arange(m, dtype=np.int64)
    K = KINDS.index
    un = np.where(j % 2 == 0, K("unmapped_flag"), K("unmapped_star"))
    low = (j // 3) % 18
    if which == "all":
        kind = np.where(j % 3 == 0, un, np.where(j % 3 == 1, K("wrong_pos"), K("correct")))
        mapq, best = np.where(j % 3 == 0, 255, np.where(j % 3 == 1, 200, low)), 3 << 8 | 17
    elif which == "no_correct":
        kind = np.where(j % 3 == 0, un, np.where(j % 3 == 1, K("wrong_pos"), K("wrong_strand")))
        mapq, best = np.where(j % 3 == 0, 255, np.where(j % 3 == 1, 200, low)), 2 << 8 | 200
    else:
        kind, mapq, best = un, j % 256, 1 << 8 | 255
    assert m >= 3 * 18 and m >= 256
    others = np.delete(truth["id"], 37)[::2]
    aligned = _cat(records_of_kind(np.full(m, truth["id"][37]), kind, mapq, 0), records_of_kind(others, 0, 60, 0))
    return dict(names=ABC, n_present=3, truth=truth, aligned=_shuffled(aligned, seed), best=best, hits=m)


# ---- the name table ---------------------------------------------------------------------------------------------------------------------
SHARED = (16, 15, 17, 31, 32, 33, 47, 48, 253)  # leading bytes a family of names shares: around the 16-byte rounds of the comparison


def name_table(n):
    """n names: families that share SHARED[k] bytes (the prefix itself, the prefix + "a", + "c", + "ab"), then short fillers"""
    fam = []
    for k, p in enumerate(SHARED):
        P = bytes([65 + k]) * p
        fam += [P, P + b"a", P + b"c"] + ([P + b"ab"] if p + 2 <= 254 else [])
    return (fam + [b"s%x" % i for i in range(max(n - len(fam), 0))])[:n]


def absent_names(table):
    """names the table does not hold, next to ones it holds: a byte shorter, a byte longer, the last byte one down and one up;
    one below the first, one above the last, one of 255 bytes"""
    have = set(table)
    near = [x for x in table if not x.startswith(b"s")] + [x for x in table if x.startswith(b"s")][:3] + [x for x in table if x.startswith(b"s")][-3:]
    out = [b"0", b"zzzz", b"L" * 255]
    for x in near:
        out += [x[:-1], x + b"0", x[:-1] + bytes([x[-1] - 1]), x[:-1] + bytes([x[-1] + 1])]
    seen, kept = set(), []
    for x in out:
        if x and x not in have and x not in seen and len(x) <= 255:
            seen.add(x)
            kept.append(x)
    assert min(kept) < min(table) and max(kept) > max(table)
    return kept


def names(n, seed=5):
    """every name of the table as RNAME on both sides, every absent name on the aligned side"""
    table = name_table(n)
    absent = absent_names(table)
    n_entries = max(n, 40)
    e = np.arange(n_entries, dtype=np.int64)
    truth = dict(id=e + 1, mate=1 + (e & 1), strand=(e >> 1) & 1, row=e % n, pos=1 + e % 500, span=30)
    own = dict(truth, mapq=e % 61, bits=0)
    k = np.arange(len(absent), dtype=np.int64)
    t = (3 * k) % n_entries
    lost = dict(id=t + 1, mate=1 + (t & 1), strand=(t >> 1) & 1, row=n + k, pos=1 + t % 500, span=30, mapq=7, bits=0)
    t = e[::5] if n > 1 else e[:0]  # (another name's row: a table of one has none)
    moved =dict(id=t + 1, mate=1 + (t & 1), strand=(t >> 1) & 1, row=(t + 1) % n, pos=1 + t % 500, span=30, mapq=8, bits=0)
    return dict(names=table + absent, n_present=n, truth=truth, aligned=_shuffled(_cat(own, lost, moved), seed), absent=len(absent),
                moved=t.size)


def shared_prefix(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


# ---- fields at the lane rounds (text) ---------------------------------------------------------------------------------------------------
LANE_NAMES = [b"r" * k for k in range(1, 41)]
OPS = b"M=XDISH"


def lane_lines(n=360):
    """n truth records as field lists: QNAMEs of 1 to 18 digits, RNAMEs of 1 to 40 bytes, CIGARs of 1 to 8 runs of 1 to 9 digits, 0, 1
    or 30 optional fields, and a SEQ as long as it takes to put the newline on lane (7 i) % 16 of its round"""
    out = []
    for i in range(n):
        d, k, c = 1 + i % 18, 1 + i % 40, i // 18
        assert c < 20
        qid, mate = (c % 10, 1 + c // 10) if d == 1 else (10 ** (d - 1) + c, 1)
        runs = []
        for m in range(1 + i % 8):
            digits = 1 + (i + 4 * m) % 9
            runs.append(b"%d%c" % (10 ** (digits - 1) + i % 7, OPS[(i + m) % 7]))
        f = [b"%d" % qid, b"%d" % ((0x40 if mate == 1 else 0x80) | 16 * (i & 1)), LANE_NAMES[k - 1], b"%d" % (1 + 3 * i), b"255", b"".join(runs), b"*", b"0",
             b"0", b"", b"*"] + [[], [b"NM:i:0"], [b"X%c:i:%d" % (65 + t % 26, t) for t in range(30)]][i % 3]
        base = len(b"\t".join(f))  # the newline's offset with an empty SEQ
        f[9] = b"A" * (1 + (7 * i - base - 1) % 16)
        assert len(b"\t".join(f)) % 16 == (7 * i) % 16
        out.append(f)
    out.append([b"777777", b"64", b"rrr", b"5", b"255", b"12M", b"*", b"0", b"0", b"ACGT", b""])  # ten tabs, an empty QUAL
    return out


def lane_aligned(fields, i):
    """the aligner's record for truth record i: MAPQ i % 256; one in four on the other strand, one in four a base further on"""
    f = list(fields)
    f[4] = b"%d" % (i % 256)
    if i % 4 == 1:
        f[1] = b"%d" % (int(f[1]) ^ 16)
    if i % 4 == 2:
        f[3] = b"%d" % (int(f[3]) + 1)
    return f


def lane_facts(lines):
    """where the tabs, the newline, the CIGAR's start and its op bytes fall, as sets of lanes (offsets from the line's start, or
    from the CIGAR's start for the ops, mod 16)"""
    facts = dict(first_tab=set(), tabs=set(), newline=set(), cigar_start=set(), op=set(), digits=set())
    for f in lines:
        ln = b"\t".join(f)
        tabs = [p for p in range(len(ln)) if ln[p] == 9]
        facts["first_tab"].add(tabs[0])
        facts["tabs"] |= {p % 16 for p in tabs[1:6]}
        facts["newline"].add(len(ln) % 16)
        facts["cigar_start"].add((tabs[4] + 1) % 16)
        run = 0
        for p, ch in enumerate(f[5]):
            if 48 <= ch <= 57:
                run += 1
            else:
                facts["op"].add(p % 16)
                facts["digits"].add(run)
                run = 0
    return facts


def pad_line(o):
    """a comment line after which the next line starts at offset o mod 16"""
    return b"@CO\t" + b"x" * (o + 11) + b"\n"


def runs_summing_to(total):
    """a CIGAR of M runs of at most nine digits whose sum is `total`"""
    full, rest = divmod(total, 999_999_999)
    return b"999999999M" * full + (b"%dM" % rest if rest else b"")
