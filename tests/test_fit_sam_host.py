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


# ---- the cases of the seam tests (tests/_fit_sam_cases.py): where each lands, by the restatement alone ---------------------------
from collections import Counter  # noqa: E402

from tests import _fit_sam_cases as cases  # noqa: E402


def lands(item, n_sets=1, k=3):
    """the counters one line moves, beside those every record moves"""
    t = _fit_sam.Tables(k, n_sets)
    t.add_text(item.line)
    assert t.c["lines"] == t.c["records"] == 1, item.what
    return {n for n, v in t.c.items() if v} - {"lines", "records", "taken_quality"}


def fit_repeated(text, n_sets, k):
    """the tables of a text whose lines repeat, each distinct line added once with its multiplicity"""
    t = _fit_sam.Tables(k, n_sets)
    for ln, n in Counter(x for x in text.split(b"\n") if x).items():
        t.add_line(ln, times=n)
    return t


def test_seam_cases_land_where_they_say():
    items = cases.rounds_items() + [i for k in cases.KS for i in cases.window_rows(k)] + cases.quality_offsets()[0]
    assert len({i.line for i in items}) > 900
    for item in items:
        assert lands(item) == {item.lands}, item.what
    named = {i.what: i.lands for i in items}
    for flag in cases.STRANDS:
        assert named[f"a number of 10 digits over the seam, flag {flag}"] == "skip_inconsistent"
        assert named[f"a number of 9 digits, the last on lane 0, flag {flag}"] == "taken_alignment"
        assert named[f"MD:Z:9 as RNEXT and no MD behind QUAL, flag {flag}"] == "skip_no_md"
        assert named[f"the text ends inside the tag, flag {flag}"] == "skip_no_md"
        assert named[f"the text ends in an empty MD, the CIGAR has no M, flag {flag}"] == "taken_alignment"
        assert named[f"two MD fields: the first is taken, flag {flag}"] == "taken_alignment"
        assert named[f"0D twice in a row, flag {flag}"] == named[f"runs of 9 digits with leading zeros, flag {flag}"] == "taken_alignment"
        for op in "NP":
            assert named[f"{op} on lane 15, flag {flag}"] == named[f"{op} on lane 0, flag {flag}"] == "skip_cigar_op"
        for bad in ("a", "*", " "):
            assert named[f"the byte {bad!r} on lane 0, flag {flag}"] == named[f"the byte {bad!r} on lane 15, flag {flag}"] == "skip_inconsistent"
    # the texts the GPU tests add hold every item once, and the sum of the lines is the sum of the texts
    texts = cases.texts_of(cases.rounds_items())
    _, c = _fit_sam.fit(texts, 1, 7, 20)
    want = Counter(i.lands for i in cases.rounds_items())
    n_last = len(texts) - 1
    assert c["taken_alignment"] == want["taken_alignment"] + n_last and c["records"] == len(cases.rounds_items()) + n_last
    assert all(c[n] == want[n] for n in want if n != "taken_alignment")


def test_seam_rows_mean_what_they_say():
    """the deleted letters of a long '^' run and the adjacent mismatch letters reach the rows as the header says"""
    by = {i.what: i.line for i in cases.md_rounds(0)}
    f = by["^ run of 48 letters, shift 1, flag 0"].split(b"\t")
    ref, qry = _fit_sam.rows(f[5], f[-1][5:].rstrip(b"\n"), f[9])
    assert qry.count(b"-") == 48 and b"-" * 48 in qry and ref[qry.index(b"-"):][:48] == b"ACGGTCATTGCAAGTCCGTAGGCTTAACGTCAGTCAGGTTACGCATGC"
    f = by["40 adjacent mismatch letters, shift 0, flag 0"].split(b"\t")
    ref, qry = _fit_sam.rows(f[5], f[-1][5:].rstrip(b"\n"), f[9])
    assert b"-" not in qry and b"-" not in ref and sum(r != q for r, q in zip(ref, qry)) == 40 + 7 and f[5] == b"%dM" % len(ref)
    f = by["^AC0T, the 0 on lane 15, flag 0"].split(b"\t")
    ref, qry = _fit_sam.rows(f[5], f[-1][5:].rstrip(b"\n"), f[9])
    at = qry.index(b"--")
    assert ref[at:at + 3] == b"ACT" and qry[at + 2:at + 3] == b"A"  # two deleted bases, then the mismatch T
    # a run of zero gives no column and moves no other (the reference's expand_cigar pushes its op zero times)
    assert _fit_sam.rows(b"0I3M0D0M2I0S1M0H", b"4", b"ACGTAC") == _fit_sam.rows(b"3M2I1M", b"4", b"ACGTAC") == (b"ACG--C", b"ACGTAC")


def test_quality_offsets_around_the_lds_limit():
    items, want = cases.quality_offsets()
    m, c = _fit_sam.fit([b"".join(i.line for i in items)], 1, 3, 20)
    assert c["taken_alignment"] == len(items) == 16 and m["qual_hist"].shape[0] == 320
    for off in (158, 159, 160, 161, 319):
        assert {q: int(n) for q, n in enumerate(m["qual_hist"][off]) if n} == want[off], off
    assert len(want[cases.LDS_POS]) == 4 and 60 not in want[cases.LDS_POS]


@pytest.mark.parametrize("what", list(cases.MALFORMED))
def test_seam_malformed_kinds(what):
    with pytest.raises(_fit_sam.Malformed):
        _fit_sam.fit([cases.GOOD + cases.MALFORMED[what] + cases.GOOD], 2, 7, 20)
    with pytest.raises(_fit_sam.Malformed):
        _fit_sam.fit([cases.record_trips_text(4, last=cases.MALFORMED[what])["text"]], 2, 7, 20)
    assert lands(cases.Item("good", cases.GOOD, "taken_alignment", False)) == {"taken_alignment"}


def test_geometry_cases():
    texts, items = cases.line_shift()
    _, c = _fit_sam.fit(texts, 1, 7, 20)
    want = Counter(i.lands for i in items)
    assert all(c[n] == cases.LANES * want[n] for n in want) and c["records"] == cases.LANES * len(items)
    for case in cases.scan_chunk_texts() + [cases.index_trips_text(3)]:
        _, c = _fit_sam.fit([case["text"]], 1, 7, 20)
        assert c["taken_alignment"] == c["records"] == case["taken"] and c["header_lines"] > case["n_tiles"]
    for cus in (4, 304):
        case = cases.record_trips_text(cus)
        _, c = _fit_sam.fit([case["text"]], 1, 7, 20)
        want = Counter(i.lands for i in case["items"])
        assert c["lines"] == case["n_lines"] and c["records"] == len(case["items"]) and all(c[n] == want[n] for n in want)
        assert case["grid"] == (32 if cus == 4 else case["grid"]) and want["taken_alignment"] > 20 and want["skip_inconsistent"] > 2
        assert b"".join(cases.cut(case["text"])) == case["text"].rstrip(b"\n")


def test_times_is_repetition():
    """Tables.add_line(line, times=n) against n repetitions, table for table: the expected side of the taken-trips test"""
    case = cases.taken_trips_text(2)
    plain = _fit_sam.Tables(8, 2)
    plain.add_text(case["text"])
    fast = fit_repeated(case["text"], 2, 8)
    assert plain.c == fast.c and plain.counts == fast.counts and sorted(plain.lengths) == sorted(fast.lengths)
    assert sorted(plain.inserts) == sorted(fast.inserts) and plain.scores.keys() == fast.scores.keys()
    assert all(sorted(plain.scores[i]) == sorted(fast.scores[i]) for i in plain.scores)
    assert plain.c["taken_alignment"] == case["taken"] and all(plain.c[n] == v for n, v in case["skips"].items())
    assert case["distinct"] <= 64 + 6 and plain.c["lines"] == case["n_lines"] > case["taken"]
    _fit.assert_model(fast.model(20), plain.model(20), "times against repetition")
    bad = _fit_sam.Tables(3, 1)
    with pytest.raises(_fit_sam.Malformed):
        bad.add_line(cases.MALFORMED["CIGAR M10"], times=5)
    assert bad.c["records"] == 5
