"""The SAM route of the model fit (include/simmr_hip.h: simmr_fit_add_sam) restated in plain Python — TEST INFRASTRUCTURE ONLY.

Written from the header's rules and from simmrd/src/alignment.rs (expand_cigar, expand_md_tag, reconstruct_alignment) and
simmrd/src/main.rs:110-260 as read: SAM line parsing, the CIGAR / MD expansion, the two rows, the orientation, the filters and
their counts.  The rows feed tests/_fit.py's kmerize_alignment, densities and bin builders.  Nothing here comes from the code
under test."""
import re

import numpy as np

from tests import _fit

COUNTS = ("lines", "header_lines", "records", "taken_quality", "taken_alignment", "skip_no_sequence", "skip_secondary",
          "skip_too_long", "skip_unmapped", "skip_mapq0", "skip_mate_unmapped", "skip_no_md", "skip_insert", "skip_cigar_op",
          "skip_inconsistent")
COMPLEMENT = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}


class Malformed(ValueError):
    pass


def expand_cigar(cigar: str) -> str:
    """alignment.rs expand_cigar: one letter per base of every op, H included ("3H1M2D1I2M" -> "HHHMDDIMM")"""
    return "".join(op * int(n) for n, op in re.findall(r"(\d+)(\D)", cigar))


def expand_md_tag(md: str):
    """alignment.rs expand_md_tag: a pair per base: ("M", "M") a match, ("N", letter) a mismatch, ("D", letter) a deleted base"""
    per_m, deleted = md_tokens(md.encode())
    out, mi, di = [], 0, 0
    for num, run, letter in re.findall(r"(\d+)|\^([A-Z]+)|([A-Z])", md):
        if num:
            out += [("M", "M")] * int(num)
            mi += int(num)
        elif run:
            out += [("D", chr(c)) for c in deleted[di:di + len(run)]]
            di += len(run)
        else:
            out.append(("N", chr(per_m[mi])))
            mi += 1
    return out


def md_tokens(md: bytes):
    """([0 = match | mismatch letter] per M column, [deleted letters]) or None where MD holds a byte it does not have or a number
    of more than nine digits; a letter is deleted when the nearest non-letter before it is '^'"""
    per_m, deleted, i, in_del = [], [], 0, False
    while i < len(md):
        c = md[i]
        if 48 <= c <= 57:
            j = i
            while j < len(md) and 48 <= md[j] <= 57:
                j += 1
            if j - i > 9:
                return None
            per_m += [0] * int(md[i:j])
            i, in_del = j, False
        elif c == ord("^"):
            i, in_del = i + 1, True
        elif 65 <= c <= 90:
            (deleted if in_del else per_m).append(c)
            i += 1
        else:
            return None
    return per_m, deleted


def cigar_runs(cigar: bytes):
    """[(n, op)] of "(<digits><op>)+" with one to nine digits a run, an op being any byte that is no digit; None otherwise"""
    runs, i = [], 0
    if not cigar:
        return None
    while i < len(cigar):
        j = i
        while j < len(cigar) and 48 <= cigar[j] <= 57:
            j += 1
        if j == i or j - i > 9 or j == len(cigar):
            return None
        runs.append((int(cigar[i:j]), chr(cigar[j])))
        i = j + 1
    return runs


def rows(cigar: bytes, md: bytes, seq: bytes):
    """(reference row, query row) in SAM's forward orientation, "cigar_op" or "inconsistent".  S consumes query bases and gives no
    column (the header's departure)."""
    runs = cigar_runs(cigar)
    if runs is None or any(op not in "M=XIDSH" for _, op in runs):
        return "cigar_op"
    toks = md_tokens(md)
    n_q = sum(n for n, op in runs if op in "M=XIS")
    n_m = sum(n for n, op in runs if op in "M=X")
    n_d = sum(n for n, op in runs if op == "D")
    if toks is None or n_q != len(seq) or len(toks[0]) != n_m or len(toks[1]) != n_d:
        return "inconsistent"
    per_m, deleted = toks
    ref, qry, qi, mi, di = bytearray(), bytearray(), 0, 0, 0
    for n, op in runs:
        for _ in range(n):
            if op in "M=X":
                ref.append(per_m[mi] or seq[qi])
                qry.append(seq[qi])
                qi, mi = qi + 1, mi + 1
            elif op == "I":
                ref.append(ord("-"))
                qry.append(seq[qi])
                qi += 1
            elif op == "D":
                ref.append(deleted[di])
                qry.append(ord("-"))
                di += 1
            elif op == "S":
                qi += 1
    return bytes(ref), bytes(qry)


def reverse_complement(row: bytes) -> bytes:
    """reversed, A <-> T and C <-> G; a gap and every other byte keep their byte"""
    return bytes(COMPLEMENT.get(c, c) for c in reversed(row))


def number(field: bytes, sign=False):
    if sign and field[:1] == b"-":
        field = field[1:]
    if not (1 <= len(field) <= 18) or not field.isdigit():
        raise Malformed(field)
    return int(field)


class Tables:
    def __init__(self, k, n_sets):
        self.k, self.n_sets = k, n_sets
        self.counts, self.scores, self.lengths, self.inserts = {}, {}, [], []
        self.c = dict.fromkeys(COUNTS, 0)

    def add_text(self, text: bytes):
        for line in text.split(b"\n"):
            if line:
                self.add_line(line)

    def add_line(self, line: bytes, times=1):
        """the line `times` times over: every table is an integer sum (tests/test_fit_sam_host.py holds this to the repetition)"""
        c = dict.fromkeys(COUNTS, 0)
        try:
            self._add_line(line, times, c)
        finally:
            for name, v in c.items():
                self.c[name] += v * times

    def _add_line(self, line, times, c):
        c["lines"] += 1
        if line[:1] == b"@":
            c["header_lines"] += 1
            return
        c["records"] += 1
        f = line.split(b"\t")
        if len(f) < 11:
            raise Malformed("fields")
        flag, mapq, tlen = number(f[1]), number(f[4]), number(f[8], True)
        cigar, seq, qual = f[5], f[9], f[10]
        if cigar != b"*" and cigar_runs(cigar) is None:
            raise Malformed("cigar")
        L = 0 if seq == b"*" else len(seq)
        if not seq or (qual != b"*" and len(qual) != L) or (qual != b"*" and any(not 33 <= q <= 126 for q in qual)):
            raise Malformed("qual")
        if seq == b"*":
            c["skip_no_sequence"] += 1
            return
        if flag & 0x900:
            c["skip_secondary"] += 1
            return
        if L > _fit.MAX_L:
            c["skip_too_long"] += 1
            return
        rev = bool(flag & 0x10)
        c["taken_quality"] += 1
        self.lengths += [L] * times
        if qual != b"*":
            for i in range(L):
                self.scores.setdefault(i, []).extend([qual[L - 1 - i if rev else i] - 33] * times)
        if flag & 4:
            c["skip_unmapped"] += 1
            return
        if mapq == 0:
            c["skip_mapq0"] += 1
            return
        if self.n_sets == 2 and tlen == 0 and flag & 8:
            c["skip_mate_unmapped"] += 1
            return
        md = next((x[5:] for x in f[11:] if x[:5] == b"MD:Z:"), None)
        if md is None:
            c["skip_no_md"] += 1
            return
        if self.n_sets == 2 and tlen > _fit.MAX_INSERT:
            c["skip_insert"] += 1
            return
        if self.n_sets == 2:
            self.inserts += [tlen] * times
        got = "cigar_op" if cigar == b"*" else rows(cigar, md, seq)
        if isinstance(got, str):
            c["skip_" + got] += 1
            return
        c["taken_alignment"] += 1
        ref, qry = (reverse_complement(r) for r in got) if rev else got
        # a query byte outside ACGTN- skips its window: kmerize_alignment's encoder answers None for it
        for pair, n in _fit.kmerize_alignment(self.k, ref, qry).items():
            self.counts[pair] = self.counts.get(pair, 0) + n * times

    def model(self, max_alt):
        """the dict tests/_fit.model answers, from these tables"""
        lengths, inserts, scores = self.lengths, self.inserts, self.scores
        n_pos = max(lengths) if lengths else 0
        m = {"qual_hist": np.zeros((n_pos, _fit.QUALS), dtype=np.uint64), "qual_density": np.zeros((n_pos, _fit.DENSITIES))}
        for pos in range(n_pos):
            if scores.get(pos):
                m["qual_hist"][pos] = np.bincount(scores[pos], minlength=_fit.QUALS)
                m["qual_density"][pos] = _fit.quality_density(scores[pos])
        probs = _fit.kmer_probabilities(self.counts, max_alt)
        m["kmer_ref"] = np.array([r for r, _ in probs], dtype=np.uint32)
        m["kmer_first"] = np.cumsum([0] + [len(a) for _, a in probs]).astype(np.uint64)
        m["pair_alt"] = np.array([a for _, alts in probs for a, _, _ in alts], dtype=np.uint32)
        m["pair_count"] = np.array([c for _, alts in probs for _, c, _ in alts], dtype=np.uint64)
        m["pair_prob"] = np.array([p for _, alts in probs for _, _, p in alts], dtype=np.float32)
        m["length_hist"] = np.bincount(lengths, minlength=_fit.MAX_L + 1).astype(np.uint64)
        m["insert_hist"] = np.bincount(inserts, minlength=_fit.MAX_INSERT + 1).astype(np.uint64)
        m["read_length_mean"], m["read_length_std"] = (_fit.mean(lengths), _fit.std_deviation(lengths)) if lengths else (0.0, 0.0)
        m["is_long"] = int(m["read_length_mean"] > 400.0)
        m["length_bin_width"], ranges, dens = _fit.bins(sorted(lengths), True) if lengths else (10, [], [])
        m["length_lo"], m["length_hi"] = (np.array([r[i] for r in ranges], dtype=np.uint32) for i in (0, 1))
        m["length_density"] = np.array(dens, dtype=np.float64)
        m["insert_size_mean"], m["insert_size_std"] = (_fit.mean(inserts), _fit.std_deviation(inserts)) if inserts else (0.0, 0.0)
        ranges, dens = [], []
        if inserts and not m["is_long"]:
            m["insert_bin_width"], ranges, dens = _fit.bins(inserts, False)
        m["insert_lo"], m["insert_hi"] = (np.array([r[i] for r in ranges], dtype=np.uint32) for i in (0, 1))
        m["insert_density"] = np.array(dens, dtype=np.float64)
        return m


def fit(texts, n_sets, k, max_alt):
    """(model, counts) of the SAM texts added in turn"""
    t = Tables(k, n_sets)
    for text in texts:
        t.add_text(text)
    return t.model(max_alt), t.c
