"""A plain restatement of the rules of simmr_vcfeval_* (include/simmr_hip.h): a variant caller's VCF scored against the strain's
sites.  Nothing here knows the library: texts in (bytes), integers only; the counts, by_qual, by_ad, the site columns, the report
and the site rows out."""
import re

import numpy as np

COUNTS = ("truth_lines", "truth_header", "truth_entries", "lines", "header", "records", "filtered", "qual_missing", "ref_call", "symbolic",
          "indel", "long_allele", "ref_call_allele", "calls", "unknown_contig", "no_site", "ref_mismatch", "wrong_allele", "correct", "wrong",
          "sites_found", "sites_wrong", "sites_missed", "sites_multiple")
AD_ROWS = 33
QUAL = re.compile(rb"([0-9]+)(?:\.([0-9]*))?(?:[eE]([+-]?)([0-9]{1,3}))?\Z")
NUMBER = re.compile(rb"[0-9]{1,18}\Z")
AD_ITEM = re.compile(rb"AD=([0-9]{1,10}),([0-9]{1,10})\Z")
BASES5 = set(b"ACGTNacgtn")
CLASS = {65: 0, 67: 1, 71: 2, 84: 3}   # A C G T


class Malformed(Exception):
    pass


class DuplicateKey(Exception):
    pass


def lines(text: bytes):
    """the lines of a text: the last may lack its newline, an empty one is no line"""
    return [ln for ln in text.split(b"\n") if ln]


def qual_row(q: bytes):
    """(row, missing) of a QUAL field; Malformed for a text that is neither "." nor a decimal number"""
    if q == b".":
        return 0, True
    m = QUAL.match(q)
    if not m or len(m.group(1)) > 18:
        raise Malformed(q)
    whole, frac = m.group(1), m.group(2) or b""
    e = int(m.group(4) or 0) * (-1 if m.group(3) == b"-" else 1)
    take = len(whole) + e
    digits = whole + frac
    digits = (digits + b"0" * max(0, take - len(digits)))[:max(take, 0)]
    return min(255, int(digits or b"0")), False


def fields(line: bytes):
    """the tab-separated fields of a record after the checks that hold on either side"""
    f = line.split(b"\t")
    if len(f) < 8:
        raise Malformed(line)
    if not NUMBER.match(f[1]) or not 1 <= int(f[1]) <= 2 ** 40:
        raise Malformed(line)
    if not f[3] or not set(f[3]) <= BASES5 or not f[4]:
        raise Malformed(line)
    qual_row(f[5])
    return f


class Model:
    def __init__(self, names, use_filtered=False):
        self.rows = {n if isinstance(n, bytes) else str(n).encode(): i
                     for i, n in enumerate(sorted(n if isinstance(n, bytes) else str(n).encode() for n in names))}
        self.use_filtered = bool(use_filtered)
        self.c = dict.fromkeys(COUNTS, 0)
        self.truth = {}      # key -> [(ref class, alt class, ad_alt), ...]
        self.order = None
        self.malformed = False

    # ---- the truth
    def truth_entry(self, ln: bytes):
        f = fields(ln)
        ref, alt = f[3].upper(), f[4].upper()
        if len(ref) != 1 or len(alt) != 1 or ref[0] not in CLASS or alt[0] not in CLASS or ref == alt or f[0] not in self.rows:
            raise Malformed(ln)
        ad = 0
        for item in f[7].split(b";"):
            if item.startswith(b"AD="):
                m = AD_ITEM.match(item)
                if not m or int(m.group(2)) >= 2 ** 32:
                    raise Malformed(ln)
                ad = int(m.group(2))
                break
        return self.rows[f[0]] << 40 | (int(f[1]) - 1), (CLASS[ref[0]], CLASS[alt[0]], ad)

    def truth_add(self, text: bytes):
        self.order = None
        for ln in lines(text):
            self.c["truth_lines"] += 1
            if ln[:1] == b"#":
                self.c["truth_header"] += 1
                continue
            try:
                key, entry = self.truth_entry(ln)
            except Malformed:
                self.malformed = True
                continue
            self.c["truth_entries"] += 1
            self.truth.setdefault(key, []).append(entry)

    def truth_plan(self):
        if self.malformed:
            raise Malformed("truth")
        if any(len(v) > 1 for v in self.truth.values()):
            raise DuplicateKey()
        self.order = sorted(self.truth)
        self.row_of = {k: i for i, k in enumerate(self.order)}
        for n in COUNTS[3:]:
            self.c[n] = 0
        self.by_qual = np.zeros((256, 2), dtype=np.uint64)
        self.best = np.zeros(len(self.order), dtype=np.uint32)
        self.hits = np.zeros(len(self.order), dtype=np.uint32)
        return len(self.order)

    # ---- the candidate
    def calls_of(self, ln: bytes):
        """What a well-formed record comes to: ('filtered' | 'ref_call', qual missing, []) or ('', qual missing, outcomes), an
        outcome per called allele in ALT order: 'symbolic' | 'indel' | 'long_allele' | 'ref_call_allele' | None (an allele that
        differs from REF in N alone) | a list of calls (CHROM, 0-based position, ref class, alt class)."""
        f = fields(ln)
        if not self.use_filtered and f[6] not in (b".", b"PASS"):
            return "filtered", False, []
        _, missing = qual_row(f[5])
        alts = f[4].split(b",")
        called = list(range(1, len(alts) + 1))
        if len(f) >= 10 and (f[8] == b"GT" or f[8].startswith(b"GT:")):
            named = set()
            for item in re.split(rb"[/|]", f[9].split(b":")[0]):
                if item == b".":
                    continue
                if not NUMBER.match(item) or int(item) > len(alts):
                    raise Malformed(ln)
                named.add(int(item))
            if not any(i >= 1 for i in named):
                return "ref_call", missing, []
            called = [i for i in called if i in named]
        ref, pos, out = f[3].upper(), int(f[1]) - 1, []
        for i in called:
            a = alts[i - 1]
            if a == b"*" or a[:1] == b"<" or b"[" in a or b"]" in a:
                out.append("symbolic")
            elif len(a) != len(ref) or not set(a) <= BASES5:
                out.append("indel")
            elif len(a) > 64:
                out.append("long_allele")
            elif a.upper() == ref:
                out.append("ref_call_allele")
            else:
                a = a.upper()
                out.append([(f[0], pos + j, CLASS[ref[j]], CLASS[a[j]]) for j in range(len(a)) if a[j] != ref[j] and a[j] in CLASS and ref[j] in CLASS] or None)
        return "", missing, out

    def verdict(self, chrom, pos, rc, ac):
        """('unknown_contig' | 'no_site' | 'ref_mismatch' | 'wrong_allele' | 'correct', entry row or None)"""
        if chrom not in self.rows:
            return "unknown_contig", None
        key = self.rows[chrom] << 40 | pos
        if pos >= 2 ** 40 or key not in self.row_of:
            return "no_site", None
        e_rc, e_ac, _ = self.truth[key][0]
        at = self.row_of[key]
        if e_rc != rc:
            return "ref_mismatch", at
        if e_ac != ac:
            return "wrong_allele", at
        return "correct", at

    def add(self, text: bytes):
        assert self.order is not None
        for ln in lines(text):
            self.c["lines"] += 1
            if ln[:1] == b"#":
                self.c["header"] += 1
                continue
            try:
                fields(ln)
            except Malformed:
                self.malformed = True
                continue
            self.c["records"] += 1
            try:
                left_out, missing, outcomes = self.calls_of(ln)
            except Malformed:
                self.malformed = True
                continue
            if left_out == "filtered":
                self.c["filtered"] += 1
                continue
            self.c["qual_missing"] += 1 if missing else 0
            if left_out:
                self.c[left_out] += 1
                continue
            qrow = qual_row(ln.split(b"\t")[5])[0]
            for o in outcomes:
                if isinstance(o, str):
                    self.c[o] += 1
                for call in (o if isinstance(o, list) else []):
                    what, at = self.verdict(*call)
                    self.c["calls"] += 1
                    self.c[what] += 1
                    self.c["wrong"] += 0 if what == "correct" else 1
                    self.by_qual[qrow, 0 if what == "correct" else 1] += 1
                    if at is not None:
                        self.hits[at] += 1
                        self.best[at] = max(int(self.best[at]), (3 if what == "correct" else 2) << 8 | qrow)

    def read(self):
        if self.malformed:
            raise Malformed("a record")
        c = dict(self.c)
        by_ad = np.zeros((AD_ROWS, 2), dtype=np.uint64)
        by_qual = np.zeros((256, 2), dtype=np.uint64)
        if self.order is not None:
            by_qual = self.by_qual.copy()
            cls = self.best >> 8
            c["sites_found"] = int((cls == 3).sum())
            c["sites_wrong"] = int((cls == 2).sum())
            c["sites_missed"] = int((self.hits == 0).sum())
            c["sites_multiple"] = int((self.hits > 1).sum())
            for i, k in enumerate(self.order):
                by_ad[self.truth[k][0][2].bit_length(), 0 if cls[i] == 3 else 1] += 1
        return c, by_qual, by_ad

    def sites(self):
        """key (uint64), alleles, ad, best, hits (uint32) ascending by key"""
        key = np.array(self.order, dtype=np.uint64)
        alleles = np.array([self.truth[k][0][0] << 2 | self.truth[k][0][1] for k in self.order], dtype=np.uint32)
        ad = np.array([self.truth[k][0][2] for k in self.order], dtype=np.uint32)
        return key, alleles, ad, self.best.copy(), self.hits.copy()


def evaluate(truth_texts, cand_texts, names, use_filtered=False) -> Model:
    m = Model(names, use_filtered)
    for t in truth_texts:
        m.truth_add(t)
    m.truth_plan()
    for t in cand_texts:
        m.add(t)
    return m


# ---- the files of the command line --------------------------------------------------------------------------------------------------
def contig_names(text: bytes):
    """the IDs of the ##contig=<ID=...> lines in front of the records, in file order"""
    out = []
    for ln in text.split(b"\n"):
        if ln and ln[:1] != b"#":
            break
        m = re.match(rb"##contig=<ID=([^,>]+)", ln)
        if m:
            out.append(m.group(1))
    return out


def report(c: dict, by_qual, by_ad) -> bytes:
    def frac(num, den):
        return f"{num}/{den}\t" + ("0" if den == 0 else "%.4f" % (100.0 * num / den))
    out = "".join(f"#{n}\t{c[n]}\n" for n in COUNTS)
    out += f"#precision\t{frac(c['correct'], c['calls'])}\n#recall\t{frac(c['sites_found'], c['truth_entries'])}\n"
    correct = calls = 0
    for q in range(255, -1, -1):
        if not int(by_qual[q, 0]) and not int(by_qual[q, 1]):
            continue
        correct += int(by_qual[q, 0])
        calls += int(by_qual[q, 0]) + int(by_qual[q, 1])
        out += f"Q\t{q}\t{int(by_qual[q, 0])}\t{int(by_qual[q, 1])}\t{frac(correct, calls)}\t{frac(correct, c['truth_entries'])}\n"
    for b in range(AD_ROWS):
        if int(by_ad[b, 0]) or int(by_ad[b, 1]):
            out += f"AD\t{b}\t{int(by_ad[b, 0])}\t{int(by_ad[b, 1])}\n"
    return out.encode()


def site_rows(names_sorted, key, alleles, ad, best, hits) -> bytes:
    """contig name, 1-based position, ref, alt, ad_alt, best class, best QUAL row, hits"""
    return "".join(f"{names_sorted[int(k) >> 40].decode()}\t{(int(k) & (2 ** 40 - 1)) + 1}\t{'ACGT'[int(a) >> 2]}\t{'ACGT'[int(a) & 3]}\t{int(d)}\t{int(b) >> 8}\t"
                   f"{int(b) & 255}\t{int(h)}\n" for k, a, d, b, h in zip(key, alleles, ad, best, hits)).encode()


# ---- builders -------------------------------------------------------------------------------------------------------------------------
def rec(chrom, pos, ref, alt, qual=".", filt=".", info=".", fmt=None, sample=None, ident=".") -> bytes:
    f = [chrom, pos, ident, ref, alt, qual, filt, info] + ([fmt] if fmt is not None else []) + ([sample] if sample is not None else [])
    return b"\t".join(x if isinstance(x, bytes) else str(x).encode() for x in f) + b"\n"


def site(chrom, pos, ref, alt, ad_ref=0, ad_alt=0) -> bytes:
    """a truth record as --strain-vcf writes it"""
    return rec(chrom, pos, ref, alt, info=f"DP={ad_ref + ad_alt};AD={ad_ref},{ad_alt};ADF={ad_ref},{ad_alt};ADR=0,0;OTH=0")


def derive(truth: bytes, spurious_chrom: bytes):
    """A candidate from a truth text, on the host: every third site dropped, every fifth with another alt, every seventh position a
    spurious site one base on (where the truth has none), QUALs spread over the rows, a sample column with GT on every other
    record."""
    taken = {(ln.split(b"\t")[0], int(ln.split(b"\t")[1])) for ln in lines(truth) if ln[:1] != b"#"}
    out = []
    for i, ln in enumerate(x for x in lines(truth) if x[:1] != b"#"):
        f = ln.split(b"\t")
        if i % 3 == 2:
            continue
        if i % 5 == 4:
            f[4] = next(bytes([b]) for b in b"ACGT" if bytes([b]) not in (f[3].upper(), f[4].upper()))
        f[5] = (b"%d" % (i * 7 % 300), b"%d.%d" % (i % 97, i % 10), b".", b"%de-1" % (i % 2000))[i % 4]
        f[7] = b"DP=9"
        if i % 2:
            f += [b"GT:GQ", (b"1/1:9", b"0|1:3", b"1:2")[i % 3]]
        out.append(b"\t".join(f) + b"\n")
        if i % 7 == 6 and (f[0], int(f[1]) + 1) not in taken:
            out.append(rec(f[0], int(f[1]) + 1, "A", "C", qual=i % 60))
    out.append(rec(spurious_chrom, 5, "A", "T", qual=11))
    return b"".join(out)
