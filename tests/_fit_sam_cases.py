"""The hand-made cases of tests/test_gpu_fit_sam_seams.py — TEST INFRASTRUCTURE ONLY.  SAM lines placed on the seams of the six
kernels of simmr_amd/csrc/fit_sam_kernels.hip: the 16-byte rounds over MD, CIGAR and the line, the 16-column groups and 256-column
rounds of the windows, the LDS limits of the tables, the 4096-byte tiles of the line index, the 256 tile counts of a scan
iteration and the grid trips of every kernel.  Pure Python; nothing here comes from the code under test.  A builder answers
Items (a line, the counter it lands in or "malformed", what it is) or a dict with the text and what it placed where, and asserts
its own precondition: that the byte it is about sits on the lane, tile or trip it claims.  MD rounds start at MD's first byte,
CIGAR rounds at CIGAR's first byte, the field scan at the line's first byte; a thread of the index owns the 16 bytes from a
multiple of 16 of the text.  tests/test_fit_sam_host.py runs every builder through the plain restatement (tests/_fit_sam.py) and
pins where each case lands; the GPU tests run the same texts through the device.

Two rules the header (include/simmr_hip.h, above simmr_fit_add_sam) leaves unsaid, as the reference's alignment.rs shows them:
a run of zero (0M, 0I, 0D, 0S, 0H) expands to nothing (expand_cigar pushes its op `runs` times), and mismatch letters that follow
one another without a 0 between them are each a mismatch (expand_md_tag plucks letters until a byte that is none)."""
import random
import re
from collections import namedtuple
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def constants():
    """the kernels' geometry as the sources state it"""
    kern, dev = (CSRC / "fit_sam_kernels.hip").read_text(), (CSRC / "fit_device.hpp").read_text()
    host, scans = (CSRC / "fit_sam.hip").read_text(), (CSRC / "sam_kernels.hip").read_text()
    define = lambda src, name: int(re.search(rf"^#define\s+{name}\s+(\d+)u?\b", src, re.M).group(1))
    c = {n: define(kern, n) for n in ("FSAM_LANES", "FSAM_TILE", "FSAM_WG_RECS", "FSAM_MIN_TAKEN")}
    c.update({n: define(dev, n) for n in ("FIT_LDS_POS", "FIT_LDS_K")})
    body = scans[scans.index("void sam_scan_chunks("):]
    c["SCAN_CHUNK"] = int(re.search(r"base \+= (\d+)u\)", body[:body.index("\n}\n")]).group(1))
    c["INDEX_WGS"] = int(re.search(r"tile_grid = .*\(uint64_t\)cus \* (\d+)u\);", host).group(1))
    c["RECORD_WGS"] = int(re.search(r"rec_grid = .*FSAM_WG_RECS \* FSAM_MIN_TAKEN\) \+ 1, \(uint64_t\)cus \* (\d+)u\);", host).group(1))
    c["WINDOWS_WGS"] = int(re.search(r"k_fsam_windows, dim3\(std::min\(rec_grid, cus \* (\d+)u\)\)", host).group(1))
    return c


C = constants()
LANES, TILE, WG_RECS, MIN_TAKEN = C["FSAM_LANES"], C["FSAM_TILE"], C["FSAM_WG_RECS"], C["FSAM_MIN_TAKEN"]
LDS_POS, LDS_K, SCAN_CHUNK = C["FIT_LDS_POS"], C["FIT_LDS_K"], C["SCAN_CHUNK"]
INDEX_WGS, RECORD_WGS, WINDOWS_WGS = C["INDEX_WGS"], C["RECORD_WGS"], C["WINDOWS_WGS"]
# the cases below are laid out for these values: a change of constant fails here, and the cases are then moved with it
assert (LANES, TILE, WG_RECS, MIN_TAKEN, LDS_POS, LDS_K, SCAN_CHUNK) == (16, 4096, 16, 28, 160, 7, 256), C
assert (INDEX_WGS, RECORD_WGS, WINDOWS_WGS) == (16, 8, 2), C

Item = namedtuple("Item", "what line lands last")  # last: the line must end its text (it has no '\n')
STRANDS = (0, 16)
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def rec_grid(n_bytes, cus):
    """workgroups of the record, md and expand kernels (fit_sam.hip)"""
    return min(n_bytes // (WG_RECS * MIN_TAKEN) + 1, RECORD_WGS * cus)


def batches(n):
    return (n + WG_RECS - 1) // WG_RECS


# ---- lines ----------------------------------------------------------------------------------------------------------------------
def line(seq, cigar, md=None, flag=0, name="r", mapq="60", tlen="0", qual=None, rnext="=", opt=("NM:i:0",), md_at=None, nl=True):
    """a SAM line; the MD field stands at optional index md_at (None: last)"""
    qual = "I" * len(seq) if qual is None else qual
    opt = list(opt)
    if md is not None:
        opt.insert(len(opt) if md_at is None else md_at, "MD:Z:" + md)
    f = [name, str(flag), "c0", "100", str(mapq), cigar, rnext, "300", str(tlen), seq, qual, *opt]
    return "\t".join(f).encode("latin-1") + (b"\n" if nl else b"")


def spans(ln):
    """offsets in the line of CIGAR and of the MD the rules take: the first optional field that starts with MD:Z:"""
    f, at, out = ln.rstrip(b"\n").split(b"\t"), 0, {"md": None}
    for j, x in enumerate(f):
        if j == 5:
            out["cigar"] = (at, at + len(x))
        if j >= 11 and out["md"] is None and x[:5] == b"MD:Z:":
            out["md"] = (at + 5, at + len(x))
        at += len(x) + 1
    return out


def _bases(n, rng):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _runs(ops):
    out = []
    for op in ops:
        if out and out[-1][0] == op:
            out[-1][1] += 1
        else:
            out.append([op, 1])
    return "".join(f"{n}{op}" for op, n in out)


def from_md(md, seed=0, **kw):
    """a record that is consistent with the literal MD: M for its matches and mismatches, D for its '^' runs"""
    rng, ops, seq = random.Random(seed), [], []
    for num, dele, mis in re.findall(r"(\d+)|\^([A-Z]*)|([A-Z])", md):
        if num:
            ops += "M" * int(num)
            seq.append(_bases(int(num), rng))
        elif mis:
            ops.append("M")
            seq.append(OTHER.get(mis, "A"))
        else:
            ops += "D" * len(dele)
    return line("".join(seq), _runs(ops), md, **kw)


def rows_md(ref, qry):
    """MD of two aligned rows ('-' a gap)"""
    md, run, in_del = "", 0, False
    for r, q in zip(ref, qry):
        if r == "-":
            continue
        if q == "-":
            if not in_del:
                md, run, in_del = md + f"{run}^", 0, True
            md += r
            continue
        in_del = False
        if r == q:
            run += 1
        else:
            md, run = md + f"{run}{r}", 0
    return md + str(run)


def from_cigar(cigar, seed=0, every=4, **kw):
    """a record that is consistent with the literal CIGAR (its digits kept as written): SEQ and MD made here; M mismatches at
    every `every`-th of its columns, = never, X always"""
    rng, ref, qry, clip, n = random.Random(seed), [], [], {}, 0
    runs = re.findall(r"(\d+)(\D)", cigar)
    assert "".join(a + b for a, b in runs) == cigar
    seq = []
    for digits, op in runs:
        for _ in range(int(digits)):
            b = rng.choice("ACGT")
            if op in "M=X":
                n += 1
                miss = op == "X" or (op == "M" and n % every == 0)
                ref.append(OTHER[b] if miss else b), qry.append(b), seq.append(b)
            elif op == "I":
                ref.append("-"), qry.append(b), seq.append(b)
            elif op == "D":
                ref.append(b), qry.append("-")
            elif op == "S":
                seq.append(b)
    return line("".join(seq), cigar, rows_md(ref, qry), **kw)


def from_rows(ref, qry, **kw):
    """a record of two aligned rows"""
    ops = ["I" if r == "-" else "D" if q == "-" else "M" for r, q in zip(ref, qry)]
    return line("".join(q for q in qry if q != "-"), _runs(ops), rows_md(ref, qry), **kw)


GOOD = line("ACGTACGTAC", "10M", "10")


def md_pad(n, letter=False):
    """n bytes of MD that end in a digit (or, with `letter`, in a mismatch letter): 1A1A..1 or 1A1A..11"""
    if letter:
        return md_pad(n - 1) + "C"
    assert n >= 1
    return "1A" * (n // 2) + "1" if n % 2 else "1A" * (n // 2 - 1) + "11"


def _md_checks(ln, checks, whole_round=None):
    """the precondition of an MD case: byte `off` of MD is `ch` (its lane is off % 16); whole_round: some round holds letters only"""
    a, b = spans(ln)["md"]
    for off, ch, lane in checks:
        assert ln[a + off:a + off + 1] == ch.encode() and off % LANES == lane, (ln, off, ch, lane)
    if whole_round is not None:
        rounds = [ln[p:min(p + LANES, b)] for p in range(a, b, LANES)]
        assert any(len(r) == LANES and r.isalpha() and r.isupper() for r in rounds) == whole_round, rounds


# ---- A: MD rounds ---------------------------------------------------------------------------------------------------------------
def md_rounds(flag, name="r"):
    kw = dict(flag=flag, name=name)
    out = []

    def add(what, ln, lands="taken_alignment", checks=(), whole_round=None, last=False):
        if checks or whole_round is not None:
            _md_checks(ln, checks, whole_round)
        out.append(Item(f"{what}, flag {flag}", ln, lands, last))

    dele = "ACGGTCATTGCAAGTCCGTAGGCTTAACGTCAGTCAGGTTACGCATGC"  # 48 letters
    add("^ on lane 15, its letters from lane 0", from_md(md_pad(15) + "^ACG5", 1, **kw), checks=[(15, "^", 15), (16, "A", 0)])
    for n in (33, 48):
        for shift in (0, 1):
            md = md_pad(15 + shift) + "^" + dele[:n] + "7"
            add(f"^ run of {n} letters, shift {shift}", from_md(md, 2, **kw), checks=[(15 + shift, "^", (15 + shift) % LANES), (16 + shift, "A", shift)], whole_round=True)
    mism = "CATGGTCAGTTGCAAGCTAGGATCCTAGGCATCGATTGCA"  # 40 letters
    for shift in (0, 1):
        add(f"40 adjacent mismatch letters, shift {shift}", from_md(md_pad(15 + shift) + mism + "3", 3, **kw), checks=[(15 + shift, "C", (15 + shift) % LANES)], whole_round=True)
    add("^AC0T, the 0 on lane 15", from_md(md_pad(12) + "^AC0T4", 4, **kw), checks=[(12, "^", 12), (15, "0", 15), (16, "T", 0)])
    add("^AC0T, the 0 on lane 0", from_md(md_pad(13) + "^AC0T4", 5, **kw), checks=[(13, "^", 13), (16, "0", 0), (17, "T", 1)])
    add("a mismatch letter on lane 0 behind a digit on lane 15", from_md(md_pad(16) + "G4", 6, **kw), checks=[(15, "1", 15), (16, "G", 0)])
    for digits in (1, 2, 9):
        for lane in (0, 1, 8):
            number = "12".rjust(digits, "0") if digits > 1 else "7"
            first = LANES + lane - digits + 1  # MD offset of the number's first digit: its last is on `lane` of the second round
            md = md_pad(first, letter=True) + number + "T2"
            add(f"a number of {digits} digits, the last on lane {lane}", from_md(md, 7, **kw),
                checks=[(first, number[0], first % LANES), (LANES + lane, number[-1], lane), (LANES + lane + 1, "T", lane + 1)])
            assert (first < LANES) == (digits > lane + 1)  # it straddles the seam exactly where it has more digits than lanes
    md = md_pad(10, letter=True) + "0000000012" + "T2"
    add("a number of 10 digits over the seam", from_md(md, 8, **kw), "skip_inconsistent", checks=[(10, "0", 10), (19, "2", 3), (20, "T", 4)])
    for n in (15, 16, 17, 31, 32, 33):
        ln = from_md(md_pad(n), 9, **kw)
        a, b = spans(ln)["md"]
        assert b - a == n and ln.endswith(b"\n") and b == len(ln) - 1
        add(f"MD of {n} bytes, the line's last field", ln)
        ln = from_md(md_pad(n), 9, md_at=0, **kw)
        assert spans(ln)["md"][1] - spans(ln)["md"][0] == n and ln[spans(ln)["md"][1]:][:1] == b"\t"
        add(f"MD of {n} bytes before another optional field", ln)
    opt = ("NM:i:0", "AS:i:9", "XS:i:0", "RG:Z:g", "XA:Z:MD:Z:5")
    for at in (1, 4):
        ln = from_md("3A4^TT2", 10, opt=opt, md_at=at, **kw)
        assert ln.split(b"\t")[11 + at] == b"MD:Z:3A4^TT2"
        add(f"MD as optional field {at + 1}", ln)
    ln = from_md("3A4", 11, opt=("NM:i:0", "MD:Z:99"), md_at=0, **kw)
    assert [x[:5] for x in ln.rstrip(b"\n").split(b"\t")[11:]] == [b"MD:Z:", b"NM:i:", b"MD:Z:"]
    add("two MD fields: the first is taken", ln)  # (the second would be inconsistent)
    ln = from_md("3A4", 11, opt=("MD:Z:99", "NM:i:0"), **kw)
    assert [x[:7] for x in ln.rstrip(b"\n").split(b"\t")[11:]] == [b"MD:Z:99", b"NM:i:0", b"MD:Z:3A"]
    add("the other order of the two", ln, "skip_inconsistent")
    ln = line("ACGTACGTA", "9M", None, rnext="MD:Z:9", **kw)
    assert ln.split(b"\t")[6] == b"MD:Z:9" and spans(ln)["md"] is None
    add("MD:Z:9 as RNEXT and no MD behind QUAL", ln, "skip_no_md")
    for bad in ("a", "*", " "):
        for lane in (0, 15):
            md = md_pad(LANES + lane) + bad + "T2"
            ln = from_md(md.replace(bad, "G"), 12, **kw).replace(md.replace(bad, "G").encode(), md.encode())
            add(f"the byte {bad!r} on lane {lane}", ln, "skip_inconsistent", checks=[(LANES + lane, bad, lane)])
    tail = line("ACGT", "4I", "", nl=False, **kw)
    assert tail.endswith(b"\tMD:Z:") and len(tail) >= MIN_TAKEN
    add("the text ends in an empty MD, the CIGAR has no M", tail, last=True)
    add("the text ends in an empty MD, the CIGAR has 4M", line("ACGT", "4M", "", nl=False, **kw), "skip_inconsistent", last=True)
    add("the text ends inside the tag", line("ACGT", "4M", "", nl=False, **kw)[:-1], "skip_no_md", last=True)
    assert out[-1].line.endswith(b"\tMD:Z")
    return out


# ---- B: CIGAR rounds and the run search -------------------------------------------------------------------------------------------
def _cigar_checks(ln, checks):
    a, _ = spans(ln)["cigar"]
    for off, ch, lane in checks:
        assert ln[a + off:a + off + 1] == ch.encode() and off % LANES == lane, (ln, off, ch, lane)


def cigar_rounds(flag, name="r"):
    kw = dict(flag=flag, name=name)
    out = []

    def add(what, ln, lands="taken_alignment", checks=()):
        _cigar_checks(ln, checks)
        out.append(Item(f"{what}, flag {flag}", ln, lands, False))

    seven, fifteen = "2M1I3M1D2M1I4M", "2M1I3M1D2M12I4M"  # 14 and 15 bytes that end in an op
    assert (len(seven), len(fifteen)) == (14, 15)
    add("an op on lane 0, its digits in the round before", from_cigar(seven + "12M3I2M", 20, **kw), checks=[(14, "1", 14), (15, "2", 15), (16, "M", 0)])
    add("runs of 9 digits with leading zeros", from_cigar("000000012M000000003I000000009M000000002D000000011M", 21, **kw),
        checks=[(9, "M", 9), (19, "I", 3), (29, "M", 13), (39, "D", 7), (49, "M", 1)])
    for op in "MIDSH":
        z = "0" + op
        add(f"0{op} first", from_cigar(z + "5M2I5M", 22, **kw))
        add(f"0{op} last", from_cigar("5M2D5M" + z, 23, **kw))
        add(f"0{op} twice in a row", from_cigar("5M" + z + z + "2I6M" + z + z, 24, **kw))
        add(f"0{op} on lane 15", from_cigar(seven + z + "3M" + z + "4M", 25, **kw), checks=[(14, "0", 14), (15, op, 15), (18, "0", 2)])
        add(f"0{op} on lanes 0 and 1", from_cigar(seven + "9M" + z + "3M", 26, **kw), checks=[(15, "M", 15), (16, "0", 0), (17, op, 1)])
        add(f"0{op}: the 0 on lane 15, the op on lane 0", from_cigar(fifteen + z + "3M", 27, **kw), checks=[(14, "M", 14), (15, "0", 15), (16, op, 0)])
    for cols in (15, 16, 17):
        cigar = "1M1I1M1D1M1I" + f"{cols - 6:03d}M" + "5M1I3M"
        add(f"a round of {cols} columns ending on its last op", from_cigar(cigar, 28, **kw), checks=[(15, "M", 15), (16, "5", 0)])
    add("eight one-digit ops, then one run of 1000 columns", from_cigar("1M1I1M1D1M1I1M1D1000M", 29, every=97, qual="*", **kw), checks=[(15, "D", 15), (20, "M", 4)])
    add("a first round of one run of 1000 columns", from_cigar("1000M1I1M1D1M1I1M1D1M", 30, every=89, qual="*", **kw))
    add("= and X mixed with M", from_cigar("3=1X4M2=1I2X1D3M1X5=", 31, **kw))
    add("clips on both ends with 0S", from_cigar("1H0S3S8M2S0S1H", 32, **kw))
    add("0S alone at both ends", from_cigar("0S12M0S", 33, **kw))
    for op in "NP":
        add(f"{op} on lane 15", from_cigar(seven + "3M", 34, **kw).replace(seven.encode() + b"3M", (seven + "3" + op + "3M").encode()), "skip_cigar_op",
            checks=[(15, op, 15)])
        add(f"{op} on lane 0", from_cigar(seven + "13M", 35, **kw).replace(seven.encode() + b"13M", (seven + "13" + op + "13M").encode()), "skip_cigar_op",
            checks=[(16, op, 0)])
    return out


def texts_of(items):
    """[the lines that end in '\\n' in one text, then a text of GOOD and the line for every line that must end its text]"""
    body = b"".join(i.line for i in items if not i.last)
    assert all(i.line.endswith(b"\n") != i.last for i in items)
    return [body] + [GOOD + i.line for i in items if i.last]


def rounds_items(name="r"):
    return [i for flag in STRANDS for i in md_rounds(flag, name) + cigar_rounds(flag, name)]


# ---- C: rows and tables ---------------------------------------------------------------------------------------------------------
EDGES = (16, 256, 512)  # a lane's group, a round of 16 groups, the second such round
KS = (3, 7, 8, 10)      # 7 = FIT_LDS_K: the dense table's last k in LDS, 8 its first in HBM


def window_rows(k):
    """Items around every edge E: one substitution, one inserted base, one N in SEQ at each column E - k .. E + 1, a deleted base
    at E - 1, E, E + 1, and records of E - 1, E, E + 1 columns"""
    assert LDS_K in KS and LDS_K + 1 in KS
    out = []
    for flag in STRANDS:
        for E in EDGES:
            rng = random.Random(1000 * E + k)
            base = _bases(E + k + 3, rng)
            n = len(base)

            def add(what, ref, qry):
                ln = from_rows(ref, qry, flag=flag, qual="*")
                assert ln.count(b"\n") == 1
                out.append(Item(f"{what}, E {E}, k {k}, flag {flag}", ln, "taken_alignment", False))
                return ln

            for c in range(E - k, E + 2):
                add(f"a substitution at column {c}", base, base[:c] + OTHER[base[c]] + base[c + 1:])
                add(f"an inserted base at column {c}", base[:c] + "-" + base[c:n - 1], base[:c] + "G" + base[c:n - 1])
                add(f"an N in SEQ at column {c}", base, base[:c] + "N" + base[c + 1:])
            for c in (E - 1, E, E + 1):
                add(f"a deleted base at column {c}", base, base[:c] + "-" + base[c + 1:])
            for cols in (E - 1, E, E + 1):
                ln = add(f"{cols} columns", base[:cols], base[:cols - 2] + OTHER[base[cols - 2]] + base[cols - 1:cols])
                assert ln.split(b"\t")[5] == b"%dM" % cols
    return out


def quality_offsets():
    """reads of 159, 160, 161 and 320 bases with a quality of their own at each of the offsets 158 .. 161 of the READ, on both
    strands (QUAL is indexed L - 1 - i on the reverse one), between records without QUAL; (items, {offset: {quality: count}})"""
    out, want = [], {}
    for L in (159, 160, 161, 320):
        for flag in STRANDS:
            q = [60] * L
            for off in range(158, min(162, L)):
                q[off] = 2 + (off - 158) + 5 * (159, 160, 161, 320).index(L) + (21 if flag else 0)  # distinct by offset, length and strand
                want.setdefault(off, {})
                want[off][q[off]] = want[off].get(q[off], 0) + 1
            for off in range(162, L):
                want.setdefault(off, {})
                want[off][60] = want[off].get(60, 0) + 1
            qual = "".join(chr(33 + v) for v in (q[::-1] if flag else q))
            seq = _bases(L, random.Random(L))
            out.append(Item(f"{L} bases, flag {flag}", line(seq, f"{L}M", str(L), flag=flag, qual=qual), "taken_alignment", False))
            out.append(Item(f"{L} bases without QUAL, flag {flag}", line(seq, f"{L}M", str(L), flag=flag, qual="*"), "taken_alignment", False))
    assert LDS_POS == 160 and set(want) >= {158, 159, 160, 161} and [len(want[o]) for o in (158, 159, 160, 161)] == [8, 6, 4, 2]
    return out, want


# ---- E: malformed records -------------------------------------------------------------------------------------------------------
MALFORMED = {
    "MAPQ no number": line("ACGTACGTAC", "10M", "10", mapq="6o"),
    "TLEN of - alone": line("ACGTACGTAC", "10M", "10", tlen="-"),
    "FLAG of 19 digits": line("ACGTACGTAC", "10M", "10", flag="0" * 19),
    "an empty SEQ": line("", "10M", "10", qual="*"),
    "SEQ * with a QUAL": line("*", "*", None, qual="I"),
    "CIGAR M10": line("ACGTACGTAC", "M10", "10"),
    "an empty CIGAR": line("ACGTACGTAC", "", "10"),
    "a CIGAR run of 10 digits": line("ACGTACGTAC", "0000000010M", "10"),
    "QUAL byte 0x20": line("ACGTACGTAC", "10M", "10", qual="IIIIIIIII "),
    "QUAL byte 0x7f": line("ACGTACGTAC", "10M", "10", qual="\x7fIIIIIIIII"),
}
assert MALFORMED["FLAG of 19 digits"].split(b"\t")[1] == b"0" * 19 and MALFORMED["an empty SEQ"].split(b"\t")[9] == b""


# ---- D: geometry ------------------------------------------------------------------------------------------------------------------
def line_shift():
    """every record of A and B under QNAMEs of 1 .. 16 bytes, one text a length: the texts, the items of one length, and the
    lanes the lines' first bytes, their tabs and their newlines fall on"""
    starts, tabs, newlines, items, body, at = set(), set(), set(), None, [], 0
    for n in range(1, LANES + 1):
        items = [i for i in rounds_items("q" * n) if not i.last]
        for i in items:
            starts.add(at % LANES)
            at += len(i.line)
            tabs |= {p % LANES for p in range(len(i.line)) if i.line[p] == 9}
            newlines.add((len(i.line) - 1) % LANES)
            body.append(i.line)
    texts = [b"".join(body)]
    assert starts == tabs == newlines == set(range(LANES))  # every phase of the index, every lane of the field scan
    return texts, items


def comment(n):
    """a header line of n bytes, its '\\n' included"""
    assert n >= 5
    return b"@CO\t" + b"x" * (n - 5) + b"\n"


def _fill(out, upto, width=2000):
    """header lines until the text is `upto` bytes long"""
    at = sum(len(x) for x in out)
    while upto - at >= 5:
        n = min(width, upto - at)
        n = n if upto - at - n == 0 or upto - at - n >= 5 else n - 5
        out.append(comment(n))
        at += n
    assert at == upto, (at, upto)


def tiles_text(n_tiles, seams, last_records=3):
    """a text of n_tiles tiles of long @CO lines.  seams: [(tile, how)]: a record whose first byte is byte 0 of `tile` ("first"),
    the last byte of the tile before ("last"), or 100 bytes before the tile ("straddle").  Records in the last tile; the final
    line lacks its '\\n'.  {text, taken, starts: [(offset, how)]}"""
    recs = [from_md(md_pad(15) + "^ACGGTCATTGCAAGTCCGTAGGCTTAACGTCAGTC0T9", 40 + j, flag=16 * (j & 1)) for j in range(len(seams) + last_records)]
    out, starts = [], []
    for j, (tile, how) in enumerate(sorted(seams)):
        at = tile * TILE - {"first": 0, "last": 1, "straddle": 100}[how]
        _fill(out, at)
        starts.append((at, how))
        out.append(recs[j])
        assert len(recs[j]) > 100
    _fill(out, (n_tiles - 1) * TILE + 400)
    tail = recs[len(seams):]
    tail[-1] = tail[-1].rstrip(b"\n")
    text = b"".join(out + tail)
    assert (len(text) + TILE - 1) // TILE == n_tiles and not text.endswith(b"\n") and len(text) - sum(map(len, tail)) >= (n_tiles - 1) * TILE
    for at, how in starts:
        assert text[at - 1:at] == b"\n" and text[at:at + 1] == b"r"
        assert at % TILE == {"first": 0, "last": TILE - 1, "straddle": TILE - 100}[how]
    return dict(text=text, taken=len(recs), starts=starts, n_tiles=n_tiles)


def scan_chunk_texts():
    """three texts of just over SCAN_CHUNK + 1 tiles: a record on byte 0 of tile SCAN_CHUNK, on the last byte of the tile before,
    and across the two (the three cannot share one seam)"""
    cases = [tiles_text(SCAN_CHUNK + 2, [(SCAN_CHUNK, how)]) for how in ("first", "last", "straddle")]
    for c in cases:
        assert c["n_tiles"] > SCAN_CHUNK + 1 and c["starts"][0][0] // TILE in (SCAN_CHUNK - 1, SCAN_CHUNK)  # a second scan iteration
    return cases


def index_trips_text(cus):
    """INDEX_WGS x cus + 2 tiles: records on the first byte of tile INDEX_WGS x cus (the first of the second trip, its '\n' the
    last byte of the first trip), on the last byte of that tile (a second seam: the two cannot share one), across the last seam
    of the first trip, and in the last tile"""
    grid = INDEX_WGS * cus
    c = tiles_text(grid + 2, [(grid - 1, "straddle"), (grid, "first"), (grid + 1, "last")])
    assert c["n_tiles"] > grid and min(c["n_tiles"], grid) == grid  # k_fsam_index: tile += gridDim.x is taken
    return c


def record_trips_text(cus, n_headers=30_000, last=None):
    """n_headers two-byte header lines "@\\n" with the records of A among them: in the first batch of 16 lines, in the last, and
    in batches `grid` and `grid + 1` (the first of the record kernel's second trip); `last`: a final line of its own.
    {text, items, grid, n_batches, where: {line index: item}}"""
    items = [i for i in md_rounds(0) + md_rounds(16) if not i.last]
    lines = [b"@\n"] * n_headers
    where, free = {}, iter(items * 4)

    def put(li):
        if li not in where:
            where[li] = next(free)
            lines[li] = where[li].line

    for li in (0, 3, 15, n_headers - 1, n_headers - 9, n_headers - 16):
        put(li)
    for step in range(97, n_headers, 997):  # sprinkled
        put(step)
    # the records at batch `grid` move the grid, which follows the bytes: the grid is chosen first, and one header line in the
    # middle of the text is made as long as it takes to reach it
    unit = WG_RECS * MIN_TAKEN
    grid = min((sum(map(len, lines)) + len(last or b"") + 4 * max(len(i.line) for i in items)) // unit + 2, RECORD_WGS * cus)
    for li in (grid * WG_RECS, grid * WG_RECS + 5, (grid + 1) * WG_RECS, (grid + 1) * WG_RECS + 15):
        put(li)
    short = (grid - 1) * unit + 10 - (sum(map(len, lines)) + len(last or b""))
    mid = n_headers // 2
    assert mid not in where and lines[mid] == b"@\n"
    if short > 0:
        lines[mid] = comment(2 + max(short, 3))
    text = b"".join(lines) + (last or b"")
    n_lines = n_headers + (1 if last else 0)
    assert rec_grid(len(text), cus) == grid and batches(n_lines) > 3 * grid, (grid, n_lines)  # more than three trips a workgroup
    got = {li // WG_RECS for li in where}
    assert {0, grid, grid + 1, batches(n_headers) - 1} <= got
    starts = [0]
    for ln in lines:
        starts.append(starts[-1] + len(ln))
    for li, item in where.items():
        assert text[starts[li]:starts[li] + len(item.line)] == item.line
    return dict(text=text, items=list(where.values()), grid=grid, n_batches=batches(n_lines), where=where, n_lines=n_lines)


def taken_trips_text(cus):
    """more than 2 x 16 x RECORD_WGS x cus taken records of at most 64 distinct short ones (10 .. 20 columns), a rejected record
    after every seventh, one record of 300 columns in the last batch of lines.  {text, taken, distinct, n_batches, ...}"""
    distinct = []
    for j in range(60):
        rng = random.Random(500 + j)
        n = 10 + j % 10
        base = _bases(n, rng)
        c = 1 + j % (n - 2)
        ref, qry = [(base, base), (base, base[:c] + OTHER[base[c]] + base[c + 1:]), (base[:c] + "-" + base[c:], base[:c] + "T" + base[c:]),
                    (base, base[:c] + "-" + base[c + 1:])][j % 4]
        distinct.append(from_rows(ref, qry, flag=16 * (j // 4 % 2), qual="*" if j % 3 else None, name=f"s{j}"))
    assert len(set(distinct)) == 60 <= 64 and all(len(x) >= MIN_TAKEN for x in distinct)
    rejected = [(line("ACGTACGT", "8M", None), "skip_no_md"), (line("ACGTACGT", "8M", "8", mapq=0), "skip_mapq0"),
                (line("ACGTACGT", "7M", "7"), "skip_inconsistent"), (line("ACGTACGT", "4M3N4M", "8"), "skip_cigar_op"), (b"@CO\tx\n", "header_lines")]
    n_taken = 2 * WG_RECS * RECORD_WGS * cus + 3 * WG_RECS + 1
    long_one = from_cigar("120M1I100M2D77M", 77, every=13, flag=16, name="long")
    assert sum(int(n) for n in re.findall(r"(\d+)", "120M1I100M2D77M")) == 300
    out, skips = [], dict.fromkeys([r[1] for r in rejected], 0)
    for j in range(n_taken - 1):
        out.append(distinct[(j * 7 + j // 60) % 60])
        if j % 7 == 6:
            r = rejected[j // 7 % len(rejected)]
            out.append(r[0])
            skips[r[1]] += 1
    out.append(long_one)  # the last line: in the last batch of lines
    text = b"".join(out)
    grid = rec_grid(len(text), cus)
    assert grid == RECORD_WGS * cus  # the text is long enough for the full grid
    assert n_taken > 2 * WG_RECS * grid and batches(n_taken) > 2 * grid                 # k_fsam_md, k_fsam_expand: a third trip begun
    assert batches(n_taken) > 3 * min(grid, WINDOWS_WGS * cus)                           # k_fsam_windows: more than three turns
    assert len(out) > n_taken and out.index(rejected[0][0]) < WG_RECS                    # record index and line index part in the first batch
    return dict(text=text, taken=n_taken, skips=skips, grid=grid, n_lines=len(out), distinct=len(set(out)))


def cut(text, n=3):
    """the text in n + 1 pieces cut at line ends of about equal distance, the last piece without its '\\n'"""
    ends = [text.index(b"\n", len(text) * (j + 1) // (n + 1)) + 1 for j in range(n)]
    assert len(set(ends)) == n and ends[-1] < len(text)
    pieces = [text[a:b] for a, b in zip([0] + ends, ends + [len(text)])]
    pieces[-1] = pieces[-1][:-1] if pieces[-1].endswith(b"\n") else pieces[-1]
    assert all(p for p in pieces) and all(p.endswith(b"\n") for p in pieces[:-1]) and not pieces[-1].endswith(b"\n")
    return pieces
