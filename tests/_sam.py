"""The SAM record of include/simmr_hip.h (simmr_sam_plan) restated in plain Python — TEST INFRASTRUCTURE ONLY.

Input: compact host columns (seq_off is a CSR of the lengths), the truth columns of tests/_truth.py::model (or a dict laid
out like them) and {(genome slot, contig): RNAME}.  Nothing here comes from the code under test."""
import re

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def _base(ch, rev):
    """a base as SAM shows it: complemented for a reverse read (ACGTN, other bytes kept), then everything outside ACGTN is N"""
    if rev:
        ch = COMP.get(ch, ch)
    return ch if ch in "ACGTN" else "N"


def _ref_base(ch, rev):
    if rev:
        ch = COMP.get(ch, ch)
    return ch if ch in "ACGT" else "N"


def md_string(L, rev, pos, ref):
    """pos / ref: the read's edits in read orientation, ascending"""
    edits = [(int(p), chr(int(c))) for p, c in zip(pos, ref)]
    if rev:
        edits = [(L - 1 - p, c) for p, c in reversed(edits)]
    out, last = [], -1
    for p, c in edits:
        assert last < p < L
        out.append(str(p - last - 1))
        out.append(_ref_base(c, rev))
        last = p
    out.append(str(L - 1 - last))
    return "".join(out)


def record(o, t, names, r, paired):
    a, b = int(o["start"][r]), int(o["end"][r])
    lo, hi = min(a, b), max(a, b)
    L = hi - lo
    rev = bool(int(o["flags"][r]) & 1)
    if paired:
        m = r ^ 1
        ma, mb = int(o["start"][m]), int(o["end"][m])
        mlo, mhi = min(ma, mb), max(ma, mb)
        mrev = bool(int(o["flags"][m]) & 1)
        flag = 0x1 | 0x2 | (0x10 if rev else 0) | (0x20 if mrev else 0) | (0x80 if r & 1 else 0x40)
        span = max(hi, mhi) - min(lo, mlo)
        positive = lo < mlo or (lo == mlo and not r & 1)
        mate = ["=", str(mlo + 1), str(span if positive else -span)]
    else:
        flag = 16 if rev else 0
        mate = ["*", "0", "0"]
    s0, s1 = int(o["seq_off"][r]), int(o["seq_off"][r + 1])
    assert s1 - s0 == L
    seq = bytes(o["seq"][s0:s1]).decode("latin-1")
    qual = bytes(o["qual"][s0:s1]).decode("latin-1")
    if rev:
        seq, qual = seq[::-1], qual[::-1]
    seq = "".join(_base(ch, rev) for ch in seq)
    e0, e1 = int(t["edit_off"][r]), int(t["edit_off"][r + 1])
    md = md_string(L, rev, t["edit_pos"][e0:e1], t["edit_ref"][e0:e1])
    fields = [str(int(o["read_id"][r])), str(flag), names[(int(o["genome"][r]), int(o["contig"][r]))], str(lo + 1), "255",
              f"{L}M" if L else "*"] + mate + [seq if L else "*", qual if L else "*", f"NM:i:{e1 - e0}", f"MD:Z:{md}"]
    return "\t".join(fields) + "\n"


def sam_text(o, t, names, paired):
    return "".join(record(o, t, names, r, paired) for r in range(len(o["start"]))).encode("latin-1")


def parse(line):
    f = line.rstrip("\n").split("\t")
    assert len(f) == 13 and f[11].startswith("NM:i:") and f[12].startswith("MD:Z:"), line
    return {"qname": f[0], "flag": int(f[1]), "rname": f[2], "pos": int(f[3]), "mapq": int(f[4]), "cigar": f[5], "rnext": f[6],
            "pnext": int(f[7]), "tlen": int(f[8]), "seq": f[9], "qual": f[10], "nm": int(f[11][5:]), "md": f[12][5:]}


def reference_from(seq, md):
    """The reference bases under an alignment of CIGAR <L>M, rebuilt from SEQ and MD alone — an independent second reading
    of the MD string (a parser, where the model above is a writer)."""
    if seq == "*":
        assert md == "0"
        return ""
    out, at = [], 0
    tokens = re.findall(r"\d+|[A-Z]", md)
    assert "".join(tokens) == md and tokens[0].isdigit() and tokens[-1].isdigit(), md
    for k, tok in enumerate(tokens):
        assert tok.isdigit() == (k % 2 == 0), md  # numbers and bases alternate
        if tok.isdigit():
            out.append(seq[at:at + int(tok)])
            at += int(tok)
        else:
            out.append(tok)
            at += 1
    assert at == len(seq), (md, len(seq))
    return "".join(out)
