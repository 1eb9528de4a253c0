"""A plain restatement of the rules of simmr_ovleval_* (include/simmr_hip.h): an overlapper's PAF scored against the true overlaps.
Nothing here knows the library: texts in, the counts, by_len, the pair columns, the report and the pair rows out."""
import re

import numpy as np

COUNTS = ("truth_lines", "truth_entries", "truth_reads", "lines", "records", "unknown_read", "self", "no_pair", "wrong_strand", "wrong_interval",
          "correct", "wrong", "pairs_found", "pairs_wrong", "pairs_missed", "pairs_multiple")
LEN_ROWS = 41
NAME = re.compile(rb"([0-9]{1,18})(/[12])?\Z")
NUMBER = re.compile(rb"[0-9]{1,18}\Z")


class Malformed(Exception):
    pass


class DuplicatePair(Exception):
    pass


def lines(text: bytes):
    """the lines of a text: the last may lack its newline, an empty one is no line"""
    return [ln for ln in text.split(b"\n") if ln]


def name_key(name: bytes):
    """id << 1 | mate of a read name, None for any other name"""
    m = NAME.match(name)
    if not m:
        return None
    return int(m.group(1)) << 1 | (1 if m.group(2) == b"/2" else 0)


def key_name(key: int) -> str:
    return f"{key >> 1}" + ("/2" if key & 1 else "")


def parse(line: bytes):
    """(query name, target name, minus, (qs, qe), (ts, te)) of a record; Malformed for anything the header calls so"""
    f = line.split(b"\t")
    if len(f) < 12:
        raise Malformed(line)
    for i in (1, 2, 3, 6, 7, 8, 9, 10, 11):
        if not NUMBER.match(f[i]):
            raise Malformed(line)
    if f[4] not in (b"+", b"-"):
        raise Malformed(line)
    ql, qs, qe, tl, ts, te = (int(f[i]) for i in (1, 2, 3, 6, 7, 8))
    if not (qs <= qe <= ql < 2 ** 40 and ts <= te <= tl < 2 ** 40):
        raise Malformed(line)
    return f[0], f[5], f[4] == b"-", (qs, qe), (ts, te)


def holds(a, b, pct: int) -> bool:
    ov = min(a[1], b[1]) - max(a[0], b[0])
    un = max(a[1], b[1]) - min(a[0], b[0])
    return ov >= 1 and 100 * ov >= pct * un


def shrink_below(iv, pct: int):
    """the longest prefix [s, e') of the interval iv that fails the criterion against iv (None: every prefix with a base holds)"""
    s, e = iv
    ov = (pct * (e - s) - 1) // 100  # the most bases with 100 * ov < pct * un
    return (s, s + ov) if 1 <= ov < e - s else None


class Model:
    def __init__(self, min_pct: int = 10):
        self.pct = min_pct or 10
        self.c = dict.fromkeys(COUNTS, 0)
        self.truth = {}      # (lo, hi) -> [minus, lo interval, hi interval, ov]
        self.order = None
        self.malformed = False

    def truth_add(self, text: bytes):
        self.order = None
        for ln in lines(text):
            self.c["truth_lines"] += 1
            try:
                qn, tn, minus, q, t = parse(ln)
                kq, kt = name_key(qn), name_key(tn)
                if kq is None or kt is None or kq == kt:
                    raise Malformed(ln)
            except Malformed:
                self.malformed = True
                continue
            self.c["truth_entries"] += 1
            pair = (min(kq, kt), max(kq, kt))
            self.truth.setdefault(pair, []).append([minus, q if kq < kt else t, t if kq < kt else q, q[1] - q[0]])

    def truth_plan(self):
        if self.malformed:
            raise Malformed("truth")
        if any(len(v) > 1 for v in self.truth.values()):
            raise DuplicatePair()
        self.order = sorted(self.truth)
        self.row = {p: i for i, p in enumerate(self.order)}
        self.reads = {k for p in self.order for k in p}
        self.c["truth_reads"] = len(self.reads)
        for n in COUNTS[3:]:
            self.c[n] = 0
        self.best = np.zeros(len(self.order), dtype=np.uint32)
        self.hits = np.zeros(len(self.order), dtype=np.uint32)
        return len(self.order), len(self.reads)

    def verdict(self, ln: bytes):
        """('unknown_read' | 'self' | 'no_pair' | 'wrong_strand' | 'wrong_interval' | 'correct', entry row or None)"""
        qn, tn, minus, q, t = parse(ln)
        kq, kt = name_key(qn), name_key(tn)
        if kq is None or kt is None or kq not in self.reads or kt not in self.reads:
            return "unknown_read", None
        if kq == kt:
            return "self", None
        pair = (min(kq, kt), max(kq, kt))
        if pair not in self.row:
            return "no_pair", None
        e_minus, e_lo, e_hi, _ = self.truth[pair][0]
        at = self.row[pair]
        if e_minus != minus:
            return "wrong_strand", at
        lo, hi = (q, t) if kq < kt else (t, q)
        if not holds(lo, e_lo, self.pct) or not holds(hi, e_hi, self.pct):
            return "wrong_interval", at
        return "correct", at

    def add(self, text: bytes):
        assert self.order is not None
        for ln in lines(text):
            self.c["lines"] += 1
            try:
                what, at = self.verdict(ln)
            except Malformed:
                self.malformed = True
                continue
            self.c["records"] += 1
            self.c[what] += 1
            if what not in ("self", "correct"):
                self.c["wrong"] += 1
            if at is not None:
                self.hits[at] += 1
                self.best[at] = max(int(self.best[at]), 3 if what == "correct" else 2)

    def read(self):
        if self.malformed:
            raise Malformed("a record")
        c = dict(self.c)
        by = np.zeros((LEN_ROWS, 2), dtype=np.uint64)
        if self.order is not None:
            c["pairs_found"] = int((self.best == 3).sum())
            c["pairs_wrong"] = int((self.best == 2).sum())
            c["pairs_missed"] = int((self.hits == 0).sum())
            c["pairs_multiple"] = int((self.hits > 1).sum())
            for i, p in enumerate(self.order):
                by[self.truth[p][0][3].bit_length(), 0 if self.best[i] == 3 else 1] += 1
        else:
            c["truth_reads"] = 0
        return c, by

    def pairs(self):
        """key_a, key_b, ov (uint64), best, hits (uint32) ascending by (key_a, key_b)"""
        ka = np.array([p[0] for p in self.order], dtype=np.uint64)
        kb = np.array([p[1] for p in self.order], dtype=np.uint64)
        ov = np.array([self.truth[p][0][3] for p in self.order], dtype=np.uint64)
        return ka, kb, ov, self.best.copy(), self.hits.copy()


def evaluate(truth_texts, cand_texts, min_pct: int = 10) -> Model:
    m = Model(min_pct)
    for t in truth_texts:
        m.truth_add(t)
    m.truth_plan()
    for t in cand_texts:
        m.add(t)
    return m


def report(c: dict, by) -> bytes:
    out = "".join(f"#{n}\t{c[n]}\n" for n in COUNTS)

    def ratio(num, den):
        return "0" if den == 0 else "%.6f" % (num / den)
    out += f"#sensitivity\t{ratio(c['pairs_found'], c['truth_entries'])}\n#precision\t{ratio(c['correct'], c['correct'] + c['wrong'])}\n"
    for b in range(LEN_ROWS):
        if int(by[b, 0]) or int(by[b, 1]):
            out += f"L\t{b}\t{int(by[b, 0])}\t{int(by[b, 1])}\n"
    return out.encode()


def pair_rows(ka, kb, ov, best, hits) -> bytes:
    return "".join(f"{key_name(int(a))}\t{key_name(int(b))}\t{int(o)}\t{int(x)}\t{int(h)}\n" for a, b, o, x, h in zip(ka, kb, ov, best, hits)).encode()


def rec(qn, ql, qs, qe, strand, tn, tl, ts, te, tail=(0, 0, 255)) -> bytes:
    return b"\t".join(str(x).encode() if not isinstance(x, bytes) else x for x in (qn, ql, qs, qe, strand, tn, tl, ts, te) + tuple(tail)) + b"\n"


def derive(truth: bytes, outside_id: int):
    """A candidate from a truth text, on the host: every third record dropped, every fifth with its strand flipped, every seventh
    with its query interval shrunk below the 10 percent criterion (where a prefix can fail it), every eleventh doubled with the
    pair named in reversed order, every thirteenth naming a read outside the run (`outside_id`)."""
    out = []
    for i, ln in enumerate(lines(truth)):
        f = ln.split(b"\t")
        if i % 3 == 2:
            continue
        if i % 5 == 4:
            f[4] = b"-" if f[4] == b"+" else b"+"
        if i % 7 == 6:
            cut = shrink_below((int(f[2]), int(f[3])), 10)
            if cut:
                f[2], f[3] = str(cut[0]).encode(), str(cut[1]).encode()
        if i % 13 == 12:
            f[5] = str(outside_id).encode()
        out.append(b"\t".join(f) + b"\n")
        if i % 11 == 10:
            g = list(f)
            g[0:4], g[5:9] = f[5:9], f[0:4]
            out.append(b"\t".join(g) + b"\n")
    return b"".join(out)
