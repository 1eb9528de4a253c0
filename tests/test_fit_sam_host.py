"""The plain restatement of the SAM route's rules (tests/_fit_sam.py) against the reference's own unit vectors
(tests/golden/fit_sam_vectors.json: the inputs and expected values of simmrd/src/alignment.rs's tests) and against hand-written
lines for the soft-clip rule, the orientation rule and every filter.  No GPU."""
import json
from pathlib import Path

import pytest

from tests import _fit, _fit_sam

VECTORS = json.loads((Path(__file__).parent / "golden" / "fit_sam_vectors.json").read_text())


def sam_line(seq, cigar, md=None, flag=0, mapq=60, tlen=0, qual=None, name="r", extra=()):
    qual = "I" * len(seq) if qual is None else qual
    f = [name, str(flag), "c0", "100", str(mapq), cigar, "=", "300", str(tlen), seq, qual, "NM:i:0", *extra]
    if md is not None:
        f.append("MD:Z:" + md)
    return "\t".join(f).encode() + b"\n"


def test_reference_vectors():
    for cigar, want in VECTORS["expand_cigar"]:
        assert _fit_sam.expand_cigar(cigar) == want
    for md, want in VECTORS["expand_md_tag"]:
        assert _fit_sam.expand_md_tag(md) == [tuple(p) for p in want]
    for v in VECTORS["reconstruct_alignment"]:
        ref, qry = _fit_sam.rows(v["cigar"].encode(), v["md"].encode(), v["query"].encode())
        assert ref.decode() == v["aligned_reference"] and qry.decode() == v["aligned_query"]


def test_soft_and_hard_clips_give_no_column():
    """S consumes query bases; MD does not cover them, so the bases behind the clip keep their MD letters (the departure)"""
    ref, qry = _fit_sam.rows(b"2H3S4M1D2M2S", b"1T2^G2", b"nnnACGTAAnn")
    assert qry == b"ACGT-AA" and ref == b"ATGTGAA"
    assert _fit_sam.rows(b"3S4M", b"4", b"ACGTACGT") == "inconsistent"  # 7 query bases, 8 in SEQ
    assert _fit_sam.rows(b"4M2N4M", b"8", b"ACGTACGT") == "cigar_op"
    assert _fit_sam.rows(b"4M", b"3", b"ACGT") == "inconsistent" and _fit_sam.rows(b"2M1D2M", b"2^AC2", b"ACGT") == "inconsistent"


def test_orientation():
    """FLAG 0x10: both rows reversed and complemented, gaps and other bytes kept; quality offset i is QUAL[L - 1 - i]"""
    assert _fit_sam.reverse_complement(b"AC-GNTR") == b"RANC-GT"
    k = 3
    fwd, rev = _fit_sam.Tables(k, 1), _fit_sam.Tables(k, 1)
    fwd.add_text(sam_line("ACGTTGCA", "8M", "2C5", qual="!\"#$%&'("))
    rev.add_text(sam_line("ACGTTGCA", "8M", "2C5", flag=16, qual="!\"#$%&'("))
    assert [fwd.scores[i][0] for i in range(8)] == list(range(8)) and [rev.scores[i][0] for i in range(8)] == list(range(7, -1, -1))
    want = _fit.kmerize_alignment(k, _fit_sam.reverse_complement(b"ACCTTGCA"), _fit_sam.reverse_complement(b"ACGTTGCA"))
    assert rev.counts == want and rev.counts != fwd.counts


FILTER_LINES = [
    ("skip_no_sequence", dict(seq="*", cigar="*", qual="*")),
    ("skip_secondary", dict(seq="ACGTACGT", cigar="8M", md="8", flag=0x100)),
    ("skip_secondary", dict(seq="ACGTACGT", cigar="8M", md="8", flag=0x800)),
    ("skip_too_long", dict(seq="ACGT" * 16384, cigar="65536M", md="65536", tlen=300, qual="*")),            # 65536 bases
    ("taken_alignment", dict(seq="ACGT" * 16383 + "ACG", cigar="65535M", md="65535", tlen=300, qual="*")),  # 65535: the longest taken
    ("skip_unmapped", dict(seq="ACGTACGT", cigar="*", flag=4)),
    ("skip_mapq0", dict(seq="ACGTACGT", cigar="8M", md="8", mapq=0)),
    ("skip_mate_unmapped", dict(seq="ACGTACGT", cigar="8M", md="8", flag=8)),
    ("skip_no_md", dict(seq="ACGTACGT", cigar="8M", tlen=200)),
    ("skip_insert", dict(seq="ACGTACGT", cigar="8M", md="8", tlen=-5001)),
    ("skip_cigar_op", dict(seq="ACGTACGT", cigar="4M3N4M", md="8", tlen=5000)),
    ("skip_cigar_op", dict(seq="ACGTACGT", cigar="*", md="8", tlen=7)),
    ("skip_inconsistent", dict(seq="ACGTACGT", cigar="7M", md="7", tlen=7)),
    ("taken_alignment", dict(seq="ACGTACGT", cigar="8M", md="8", tlen=-300, mapq=255)),
    ("taken_alignment", dict(seq="ACGTACGT", cigar="8M", md="8", tlen=300, qual="*")),
]


def filter_text():
    return b"@HD\tVN:1.6\n" + b"".join(sam_line(**kw) for _, kw in FILTER_LINES) + b"\n@CO\tlast\n"


def test_every_filter():
    t = _fit_sam.Tables(3, 2)
    for name, kw in FILTER_LINES:
        before = dict(t.c)
        t.add_text(sam_line(**kw))
        changed = {n for n in t.c if t.c[n] != before[n]} - {"lines", "records", "taken_quality"}
        assert changed == {name}, (name, changed)
    assert t.c["records"] == len(FILTER_LINES) and t.c["taken_quality"] == len(FILTER_LINES) - 4 and t.c["skip_too_long"] == 1
    assert sorted(t.inserts) == [7, 7, 300, 300, 300, 5000] and len(t.lengths) == t.c["taken_quality"]
    assert max(t.lengths) == _fit.MAX_L == 65535 and max(t.scores) == 7
    assert len(t.scores[0]) == t.c["taken_quality"] - 2  # QUAL "*" counts for the lengths alone
    one = _fit_sam.Tables(3, 1)
    one.add_text(filter_text())
    assert one.c["skip_mate_unmapped"] == 0 and one.c["skip_insert"] == 0 and not one.inserts and one.c["header_lines"] == 2
    assert one.c["lines"] == len(FILTER_LINES) + 2


@pytest.mark.parametrize("line", [
    b"r\t0\tc0\t1\t60\t4M\t*\t0\t0\tACGT\n",                                   # 10 fields
    sam_line("ACGT", "4M", "4").replace(b"\t0\tc0", b"\tx0\tc0"),               # FLAG
    sam_line("ACGT", "4M", "4", mapq="6o"), sam_line("ACGT", "4M", "4", tlen="+3"),
    sam_line("ACGT", "M4", "4"), sam_line("ACGT", "4", "4"), sam_line("ACGT", "4M2", "4"), sam_line("ACGT", "1234567890M", "4"),
    sam_line("ACGT", "4M", "4", qual="III"), sam_line("ACGT", "4M", "4", qual="II I"), sam_line("*", "*", qual="I"),
])
def test_malformed(line):
    with pytest.raises(_fit_sam.Malformed):
        _fit_sam.Tables(3, 2).add_text(line)
