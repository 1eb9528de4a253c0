"""The rules of simmr_mapeval_* (include/simmr_hip.h) restated in plain Python: a line splitter, a CIGAR reader, the key, the
verdict, the tables and the per-entry columns in key order, the report the command line prints from them, and a helper that
derives an "aligner's" SAM from a truth text by listed perturbations.  Test infrastructure: it takes nothing from the library."""
import re

import numpy as np

COUNTS = ("truth_lines", "truth_header", "truth_entries", "truth_skipped", "lines", "header", "records", "secondary", "cigar_op",
          "unknown_read", "unknown_ref", "unmapped", "correct", "wrong", "missing", "multiple", "reads_correct", "reads_wrong",
          "reads_unmapped")
MAX_POS, MAX_END, RNAME_MAX = 2 ** 31 - 1, 2 ** 40, 254
CIGAR = re.compile(rb"(?:[0-9]{1,9}[^0-9])+", re.S)
RUN = re.compile(rb"([0-9]{1,9})([^0-9])", re.S)
NUMBER = re.compile(rb"[0-9]{1,18}")


class Malformed(Exception):
    pass


class DuplicateKey(Exception):
    pass


def lines(text: bytes):
    """the lines of a text: an empty line is none, the last may lack its newline"""
    return [ln for ln in bytes(text).split(b"\n") if ln]


def number(field: bytes):
    return int(field) if NUMBER.fullmatch(field) else None


def cigar_span(cigar: bytes):
    """(M + D, whether another op than M = X I D S H stands in it); "*": the empty interval"""
    if cigar == b"*":
        return 0, False
    if not CIGAR.fullmatch(cigar):
        raise Malformed(cigar)
    span, other = 0, False
    for n, op in RUN.findall(cigar):
        if op in b"M=XD":
            span += int(n)
        elif op not in b"ISH":
            other = True
    return span, other


def record(line: bytes) -> dict:
    """what both sides read of a record; Malformed by the rules every record is checked against"""
    f = line.split(b"\t")
    if len(f) < 11:
        raise Malformed(line)
    flag, pos, mapq = number(f[1]), number(f[3]), number(f[4])
    if flag is None or pos is None or mapq is None or mapq > 255 or pos > MAX_POS:
        raise Malformed(line)
    span, other = cigar_span(f[5])
    if (pos - 1 if pos else 0) + span > MAX_END:
        raise Malformed(line)
    return dict(id=number(f[0]), flag=flag, rname=f[2], pos=pos, mapq=mapq, span=span, other=other)


def verdict(truth, rec, pct: int) -> bool:
    """truth = (row, strand, lo, hi); rec likewise"""
    (trow, tstrand, tlo, thi), (row, strand, lo, hi) = truth, rec
    ov = max(0, min(hi, thi) - max(lo, tlo))
    un = max(hi, thi) - min(lo, tlo)
    return row == trow and strand == tstrand and ov >= 1 and 100 * ov >= pct * un


class Model:
    def __init__(self, names, min_overlap_pct: int = 10):
        names = [n if isinstance(n, bytes) else str(n).encode() for n in names]
        assert len(set(names)) == len(names)
        self.row = {n: i for i, n in enumerate(sorted(names))}
        self.pct = min_overlap_pct
        self.c = dict.fromkeys(COUNTS, 0)
        self.truth = {}
        self.pending = []
        self.planned = False

    def truth_add(self, text: bytes):
        self.planned = False
        for ln in lines(text):
            self.c["truth_lines"] += 1
            if ln[:1] == b"@":
                self.c["truth_header"] += 1
                continue
            r = record(ln)
            if r["flag"] & 0x904 or r["other"]:
                self.c["truth_skipped"] += 1
                continue
            if r["id"] is None or r["rname"] not in self.row or len(r["rname"]) > RNAME_MAX or r["pos"] == 0:
                raise Malformed(ln)
            self.c["truth_entries"] += 1
            lo = r["pos"] - 1
            self.pending.append((r["id"] << 1 | (r["flag"] >> 7 & 1), (self.row[r["rname"]], r["flag"] >> 4 & 1, lo, lo + r["span"])))

    def truth_plan(self) -> int:
        keys = [k for k, _ in self.pending]
        if len(set(keys)) != len(keys):
            raise DuplicateKey()
        self.truth = dict(self.pending)
        self.keys = sorted(self.truth)
        self.best = dict.fromkeys(self.keys, 0)
        self.hits = dict.fromkeys(self.keys, 0)
        self.by_mapq = np.zeros((256, 2), dtype=np.uint64)
        for n in COUNTS[4:]:
            self.c[n] = 0
        self.planned = True
        return len(self.keys)

    def add(self, text: bytes):
        assert self.planned
        c = self.c
        for ln in lines(text):
            c["lines"] += 1
            if ln[:1] == b"@":
                c["header"] += 1
                continue
            c["records"] += 1
            r = record(ln)
            if r["flag"] & 0x900:
                c["secondary"] += 1
                continue
            if r["other"]:
                c["cigar_op"] += 1
                continue
            key = None if r["id"] is None else r["id"] << 1 | (r["flag"] >> 7 & 1)
            if key not in self.truth:
                c["unknown_read"] += 1
                continue
            if r["flag"] & 4 or r["rname"] == b"*":
                cls = 1
                c["unmapped"] += 1
            else:
                if r["pos"] == 0:
                    raise Malformed(ln)
                cls = 2
                if r["rname"] not in self.row or len(r["rname"]) > RNAME_MAX:
                    c["unknown_ref"] += 1
                else:
                    lo = r["pos"] - 1
                    if verdict(self.truth[key], (self.row[r["rname"]], r["flag"] >> 4 & 1, lo, lo + r["span"]), self.pct):
                        cls = 3
                c["correct" if cls == 3 else "wrong"] += 1
                self.by_mapq[r["mapq"], 0 if cls == 3 else 1] += 1
            self.best[key] = max(self.best[key], cls << 8 | r["mapq"])
            self.hits[key] += 1

    def read(self):
        c = dict(self.c)
        if self.planned:
            c["missing"] = sum(1 for k in self.keys if self.hits[k] == 0)
            c["multiple"] = sum(1 for k in self.keys if self.hits[k] > 1)
            for name, cls in (("reads_correct", 3), ("reads_wrong", 2), ("reads_unmapped", 1)):
                c[name] = sum(1 for k in self.keys if self.best[k] >> 8 == cls)
        return c, self.by_mapq.copy()

    def entries(self):
        return (np.array(self.keys, dtype=np.uint64), np.array([self.best[k] for k in self.keys], dtype=np.uint32),
                np.array([self.hits[k] for k in self.keys], dtype=np.uint32))


def evaluate(names, truth_texts, aligned_texts, pct: int = 10) -> Model:
    m = Model(names, pct)
    for t in truth_texts:
        m.truth_add(t)
    m.truth_plan()
    for t in aligned_texts:
        m.add(t)
    return m


# ---- what the command line writes ------------------------------------------------------------------------------------------------
def c_g6(x: float) -> str:
    """C's %.6g (Python's % operator formats as printf does)"""
    return "%.6g" % x


def report(counts: dict, by_mapq) -> bytes:
    out = [f"#{n}\t{counts[n]}\n" for n in COUNTS]
    cum_mapped = cum_wrong = 0
    for q in range(255, -1, -1):
        ok, wrong = int(by_mapq[q][0]), int(by_mapq[q][1])
        if ok + wrong == 0:
            continue
        cum_mapped += ok + wrong
        cum_wrong += wrong
        out.append(f"Q\t{q}\t{ok + wrong}\t{wrong}\t{c_g6(cum_wrong / cum_mapped)}\t{cum_mapped}\n")
    return "".join(out).encode()


def reads_file(key, best, hits) -> bytes:
    out = []
    for k, b, h in zip(key, best, hits):
        if int(b) >> 8 != 3:
            out.append(f"{int(k) >> 1}\t{int(k) & 1}\t{int(b) >> 8}\t{int(b) & 255}\t{int(h)}\n")
    return "".join(out).encode()


def sq_names(text: bytes):
    """the SN: values of a text's @SQ lines, in file order"""
    names = []
    for ln in lines(text):
        if ln.startswith(b"@SQ\t"):
            for f in ln.split(b"\t")[1:]:
                if f.startswith(b"SN:"):
                    names.append(f[3:])
                    break
    return names


# ---- an "aligner's" text from a truth text ----------------------------------------------------------------------------------------
def threshold_shift(length: int, pct: int) -> int:
    """the largest d at which an interval of `length` bases moved by d still passes: 100 (L - d) >= pct (L + d)"""
    return length * (100 - pct) // (100 + pct)


def perturb(line: bytes, what: str, arg=None):
    """the records (a list: none, one or two) an aligner might give for the truth record `line`"""
    f = line.split(b"\t")
    flag, pos = int(f[1]), int(f[3])

    def out(**kw):
        g = list(f)
        for k, v in kw.items():
            g[{"qname": 0, "flag": 1, "rname": 2, "pos": 3, "mapq": 4, "cigar": 5}[k]] = str(v).encode() if not isinstance(v, bytes) else v
        return b"\t".join(g)

    if what == "same":
        return [line]
    if what == "shift":
        return [out(pos=pos + arg)] if pos + arg >= 1 else [line]
    if what == "strand":
        return [out(flag=flag ^ 0x10)]
    if what == "contig":
        return [out(rname=arg)]
    if what == "unmapped":
        return [out(flag=flag | 4, rname=b"*", pos=0, cigar=b"*", mapq=0)]
    if what == "unmapped_flag":
        return [out(flag=flag | 4)]
    if what == "rname_star":
        return [out(rname=b"*", pos=0, cigar=b"*")]
    if what == "drop":
        return []
    if what == "double":
        return [line, out(pos=pos + 7, mapq=arg if arg is not None else 3)]
    if what == "secondary":
        return [line, out(flag=flag | 0x100, pos=pos + 1000)]
    if what == "supplementary":
        return [out(flag=flag | 0x800)]
    if what == "cigar":
        return [out(cigar=arg)]
    if what == "mapq":
        return [out(mapq=arg)]
    if what == "qname":
        return [out(qname=arg)]
    raise ValueError(what)


def derive(truth_text: bytes, plan, seed: int = 0, shuffle: bool = True) -> bytes:
    """record i of the truth gets plan[i % len(plan)] = (what, arg); header lines are kept in front; the records are shuffled"""
    head, recs = [], []
    i = 0
    for ln in lines(truth_text):
        if ln[:1] == b"@":
            head.append(ln)
            continue
        what, arg = plan[i % len(plan)]
        recs += perturb(ln, what, arg(ln) if callable(arg) else arg)
        i += 1
    if shuffle:
        order = np.random.default_rng(seed).permutation(len(recs))
        recs = [recs[j] for j in order]
    return b"".join(ln + b"\n" for ln in head + recs)
