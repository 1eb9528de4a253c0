"""A plain-Python model of simmr_correval_* (include/simmr_hip.h states the rules): strings, lists and dicts; no tiles, rounds or
hashes, and no code shared with the library.  Every expected value of the correval tests comes from here."""
import re

POS = 512
QUALS = 95
NO_HIT = 0xffffffff
COUNTS = ("truth_lines", "truth_header", "truth_records", "truth_entries", "truth_skipped", "lines", "records", "unknown_read", "scored",
          "trimmed_records", "longer_records", "compared", "kept", "damaged", "fixed", "left", "miscorrected", "ambiguous", "trimmed_error",
          "trimmed_clean", "extra", "missing", "multiple", "clean_kept", "clean_damaged", "fixed_all", "improved", "unchanged", "worse")
VERDICTS = ("kept", "damaged", "fixed", "left", "miscorrected")


class Malformed(Exception):
    pass


def base_class(ch: str) -> int:
    return "ACGT".index(ch.upper()) if ch.upper() in "ACGT" and len(ch) == 1 else 4


def _number(s: str, most: int = 18):
    return int(s) if re.fullmatch(r"[0-9]{1,%d}" % most, s) else None


def _lines_sam(text: bytes):
    return [ln for ln in text.decode("latin-1").split("\n") if ln != ""]


def truth_of(texts):
    """The truth side over a list of SAM texts: (counts of the truth, {key: entry}); an entry is a dict with L, o, t, q (lists in the
    read's orientation) and before.  Raises Malformed."""
    c = dict.fromkeys(COUNTS[:5], 0)
    entries = {}
    bad = dup = False
    for text in texts:
        for ln in _lines_sam(text):
            c["truth_lines"] += 1
            if ln[0] == "@":
                c["truth_header"] += 1
                continue
            c["truth_records"] += 1
            f = ln.split("\t")
            if len(f) < 11:
                bad = True
                continue
            flag, pos, mapq, cigar = _number(f[1]), _number(f[3]), _number(f[4]), f[5]
            if flag is None or pos is None or mapq is None or mapq > 255 or pos > 2**31 - 1 or cigar == "":
                bad = True
                continue
            if cigar != "*":
                if not re.fullmatch(r"([0-9]{1,9}[^0-9])+", cigar):
                    bad = True
                    continue
                span = sum(int(n) for n, op in re.findall(r"([0-9]+)([^0-9])", cigar) if op in "M=XD")
                if max(pos - 1, 0) + span > 2**40:
                    bad = True
                    continue
            seq, qual = f[9], f[10]
            L = len(seq)
            m = re.fullmatch(r"([0-9]{1,18})M", cigar)
            if (flag & 0x904) or seq == "*" or not m or int(m.group(1)) != L or L == 0:
                c["truth_skipped"] += 1
                continue
            rid = _number(f[0])
            md = next((x[5:] for x in f[11:] if x.startswith("MD:Z:")), None)
            if rid is None or pos == 0 or md is None:
                bad = True
                continue
            if qual != "*" and (len(qual) != L or any(not "!" <= ch <= "~" for ch in qual)):
                bad = True
                continue
            if not re.fullmatch(r"[0-9A-Z]*", md) or re.search(r"[0-9]{10}", md):
                bad = True
                continue
            true = []
            at = 0
            for tok in re.findall(r"[0-9]+|[A-Z]", md):
                if tok.isdigit():
                    true += list(seq[at:at + int(tok)])
                    at += int(tok)
                else:
                    true.append(tok)
                    at += 1
            if at != L:
                bad = True
                continue
            o = [base_class(ch) for ch in seq]
            t = [base_class(ch) for ch in true]   # (a matched position of `true` is SEQ's own byte, so its class is o's)
            q = [94] * L if qual == "*" else [ord(ch) - 33 for ch in qual]
            if flag & 0x10:
                o = [x ^ 3 if x < 4 else x for x in reversed(o)]
                t = [x ^ 3 if x < 4 else x for x in reversed(t)]
                q = q[::-1]
            key = rid << 1 | (1 if flag & 0x80 else 0)
            c["truth_entries"] += 1
            if key in entries:
                dup = True
            entries[key] = {"L": L, "o": o, "t": t, "q": q, "before": sum(1 for a, b in zip(o, t) if a != b and b != 4)}
    if bad or dup:
        raise Malformed("truth")
    return c, entries


def name_key(name: str):
    mate = 0
    if len(name) >= 3 and name[-2] == "/" and name[-1] in "12":
        mate = 1 if name[-1] == "2" else 0
        name = name[:-2]
    rid = _number(name)
    return None if rid is None else rid << 1 | mate


def lines_of(text: bytes):
    if text == b"":
        return []
    lines = text.decode("latin-1").split("\n")
    return lines[:-1] if text.endswith(b"\n") else lines


def score(truth_texts, read_texts, lines_per_record=4):
    """(counts, cube[t][o][c], by_qual[q][v], by_pos[p][v], rows) with rows = [(key, L, before, residual, hits)] ascending by key.
    Raises Malformed."""
    c, entries = truth_of(truth_texts)
    c.update(dict.fromkeys(COUNTS[5:], 0))
    cube = [[[0] * 5 for _ in range(5)] for _ in range(5)]
    by_qual = [[0] * 5 for _ in range(QUALS)]
    by_pos = [[0] * 5 for _ in range(POS)]
    hits = dict.fromkeys(entries, 0)
    residual = dict.fromkeys(entries, NO_HIT)
    bad = False
    first = "@" if lines_per_record == 4 else ">"
    for text in read_texts:
        lines = lines_of(text)
        c["lines"] += len(lines)
        if len(lines) % lines_per_record:
            bad = True
        for r in range(len(lines) // lines_per_record):
            rec = lines[r * lines_per_record:(r + 1) * lines_per_record]
            c["records"] += 1
            if not rec[0].startswith(first):
                bad = True
                continue
            if lines_per_record == 4 and (not rec[2].startswith("+") or len(rec[3]) != len(rec[1])):
                bad = True
                continue
            key = name_key(re.split(r"[ \t]", rec[0][1:], maxsplit=1)[0])
            if key is None or key not in entries:
                c["unknown_read"] += 1
                continue
            e = entries[key]
            L, Lc = e["L"], len(rec[1])
            c["scored"] += 1
            c["trimmed_records"] += Lc < L
            c["longer_records"] += Lc > L
            c["compared"] += min(L, Lc)
            res = 0
            for i in range(L):
                o, t, q = e["o"][i], e["t"][i], e["q"][i]
                if i < Lc:
                    cc = base_class(rec[1][i])
                    cube[t][o][cc] += 1
                    if t == 4:
                        c["ambiguous"] += 1
                        continue
                    if o == t:
                        v = "kept" if cc == t else "damaged"
                    else:
                        v = "fixed" if cc == t else "left" if cc == o else "miscorrected"
                    by_qual[q][VERDICTS.index(v)] += 1
                    by_pos[min(i, POS - 1)][VERDICTS.index(v)] += 1
                    res += cc != t
                else:
                    if t == 4:
                        c["ambiguous"] += 1
                        continue
                    v = "trimmed_error" if o != t else "trimmed_clean"
                    res += 1
                c[v] += 1
            extra = max(Lc - L, 0)
            c["extra"] += extra
            res += extra
            hits[key] += 1
            residual[key] = min(residual[key], res)
    if bad:
        raise Malformed("reads")
    rows = []
    for key in sorted(entries):
        b, r, h = entries[key]["before"], residual[key], hits[key]
        rows.append((key, entries[key]["L"], b, r, h))
        c["missing"] += h == 0
        c["multiple"] += h > 1
        if h:
            name = ("clean_kept" if r == 0 else "clean_damaged") if b == 0 else \
                   "fixed_all" if r == 0 else "improved" if r < b else "unchanged" if r == b else "worse"
            c[name] += 1
    return {k: int(v) for k, v in c.items()}, cube, by_qual, by_pos, rows


# ---- builders of the two texts (the tests' inputs; the model above never sees them) -------------------------------------------------
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp(s: str) -> str:
    return s[::-1].translate(_COMP)


def md_of(ref: str, seq: str) -> str:
    out, run = "", 0
    for a, b in zip(ref, seq):
        if a == b:
            run += 1
        else:
            out += "%d%s" % (run, a)
            run = 0
    return out + str(run)


def make_read(rng, rid, L, mate=None, rev=False, errors=(), qual=None, ref=None):
    """A read in SAM's forward orientation: `ref` the true bases, `seq` what was emitted (a substitution at every offset of `errors`)."""
    ref = ref if ref is not None else "".join(rng.choice("ACGT") for _ in range(L))
    seq = list(ref)
    for at in errors:
        seq[at] = rng.choice([b for b in "ACGT" if b != ref[at]])
    qual = qual if qual is not None else "".join(chr(33 + rng.randrange(2, 42)) for _ in range(L))
    return {"rid": rid, "mate": mate, "rev": rev, "ref": ref, "seq": "".join(seq), "qual": qual}


def sam_record(r, pos=7, rname="c1") -> str:
    flag = (0x10 if r["rev"] else 0) | ({None: 0, 0: 0x41, 1: 0x81}[r["mate"]])
    nm = sum(a != b for a, b in zip(r["ref"], r["seq"]))
    return "\t".join([str(r["rid"]), str(flag), rname, str(pos), "60", "%dM" % len(r["seq"]), "*", "0", "0", r["seq"], r["qual"],
                      "NM:i:%d" % nm, "MD:Z:" + md_of(r["ref"], r["seq"])]) + "\n"


def read_name(r) -> str:
    return str(r["rid"]) + ("" if r["mate"] is None else "/%d" % (r["mate"] + 1))


def emitted(r) -> str:
    return revcomp(r["seq"]) if r["rev"] else r["seq"]


def true_read(r) -> str:
    return revcomp(r["ref"]) if r["rev"] else r["ref"]


def fastq_record(r, bases=None, name=None, lines_per_record=4) -> str:
    bases = emitted(r) if bases is None else bases
    name = read_name(r) if name is None else name
    if lines_per_record == 2:
        return ">%s\n%s\n" % (name, bases)
    q = r["qual"][::-1] if r["rev"] else r["qual"]
    q = (q + "I" * len(bases))[:len(bases)] if q != "*" else "I" * len(bases)
    return "@%s\n%s\n+\n%s\n" % (name, bases, q)


def cut_at(text: bytes, ends, pieces):
    """`text` cut behind some of the offsets `ends` into at most `pieces` adds"""
    ends = [e for e in ends if 0 < e < len(text)]
    take = sorted({ends[(k * len(ends)) // pieces] for k in range(1, pieces)}) if ends else []
    out, a = [], 0
    for e in take + [len(text)]:
        if e > a:
            out.append(text[a:e])
            a = e
    return out


# ---- the report of --eval-corrected, restated (integers only) ---------------------------------------------------------------------------
def ratio(num: int, den: int) -> str:
    if den == 0:
        return "NA"
    q = (abs(num) * 2000000 + den) // (2 * den)
    return "%s%d.%06d" % ("-" if num < 0 and q else "", q // 1000000, q % 1000000)


def report(counts: dict, cube, by_qual, by_pos) -> str:
    out = "".join("#%s\t%d\n" % (n, counts[n]) for n in COUNTS)
    errors = counts["fixed"] + counts["left"] + counts["miscorrected"] + counts["trimmed_error"]
    out += "#gain\t%d/%d\t%s\n" % (counts["fixed"] - counts["damaged"], errors, ratio(counts["fixed"] - counts["damaged"], errors))
    out += "#sensitivity\t%d/%d\t%s\n" % (counts["fixed"], errors, ratio(counts["fixed"], errors))
    clean = counts["kept"] + counts["damaged"]
    out += "#specificity\t%d/%d\t%s\n" % (counts["kept"], clean, ratio(counts["kept"], clean))
    for tag, what, table in (("Q", "quality", by_qual), ("P", "position", by_pos)):
        out += "#%s\t%s\tkept\tdamaged\tfixed\tleft\tmiscorrected\n" % (tag, what)
        out += "".join("%s\t%d\t%s\n" % (tag, r, "\t".join(str(int(x)) for x in row)) for r, row in enumerate(table) if any(int(x) for x in row))
    out += "#C\ttrue\toriginal\tA\tC\tG\tT\tN\n"
    for t in range(5):
        for o in range(5):
            out += "C\t%s\t%s\t%s\n" % ("ACGTN"[t], "ACGTN"[o], "\t".join(str(int(x)) for x in cube[t][o]))
    return out


def read_rows(rows) -> str:
    return "".join("%d\t%d\t%d\t%d\t%s\t%d\n" % (k >> 1, k & 1, L, b, r if h else ".", h) for k, L, b, r, h in rows if not (h and r == 0))
