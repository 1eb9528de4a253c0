"""The fast restatements of tests/_seams.py against the plain model of tests/_overlap.py on a few hundred reads: the pairs by
index equal _overlap.pairs entry for entry, and every vectorised record length equals the length of the line _overlap.record
formats; and the index from columns (bai_from_columns) against the plain index of tests/_bai.py, byte for byte, on the records of
the sorted-BAM tests and on every shape of tests/test_gpu_bai_seams.py at a small size; and the mapeval tables from columns (mapeval_from_columns) against the
plain model of tests/_mapeval.py, table for table, on random columns that hold every class and on every case of
tests/test_gpu_mapeval_seams.py at a small size; and the pileup from columns (pileup_keys, pileup_from_columns) against the
plain model of tests/_pileup.py, cell for cell, on a few hundred reads over the three genomes of the GPU suite and on the small
cases of tests/test_gpu_pileup_seams.py.  Runs without a GPU."""
import numpy as np
import pytest

from tests import _bai, _bai_cases, _mapeval, _mapeval_cases, _overlap, _pileup, _pileup_cases, _seams

DIGITS = [9, 10, 99, 100, 999_999_999, 1_000_000_000, 4_294_967_295]


def random_reads(n, seed, paired, n_rows=4, span=3000, lmax=260):
    """the model's read tuples: several rows, one read in four on the (row, lo) of an earlier one, one in five shorter than
    any threshold used here, both strands, ids of one to ten digits"""
    rng = np.random.default_rng(seed)
    reads = []
    for r in range(n):
        row, lo = int(rng.integers(0, n_rows)), int(rng.integers(0, span))
        if r and r % 4 == 0:
            row, lo = reads[int(rng.integers(0, r))][:2]
        L = int(rng.integers(0, 12)) if r % 5 == 0 else int(rng.integers(12, lmax))
        rid = int(rng.integers(0, 10 ** int(rng.integers(1, 11)))) % 2**32
        reads.append((row, lo, lo + L, int(rng.integers(0, 2)), rid, 1 + (r & 1) if paired else 0))
    return reads


def lengths_of(reads, ps, paired):
    col = lambda k: [r[k] for r in reads]
    a, b, s, e = ([p[k] for p in ps] for k in range(4))
    return _seams.record_lengths(col(1), col(2), col(3), col(4), a, b, s, e, paired)


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "paired"])
@pytest.mark.parametrize("min_overlap", [1, 12, 100])
def test_restatements_equal_the_model(paired, min_overlap):
    reads = random_reads(400, 5 + min_overlap, paired)
    text, ps = _overlap.paf(reads, min_overlap)
    assert len(ps) > 300 and len({(r[0], r[1]) for r in reads}) < len(reads)  # (records, and ties in (row, lo))
    assert any(r[2] - r[1] < min_overlap for r in reads) or min_overlap == 1
    assert _seams.pairs_by_index(reads, min_overlap) == ps
    want = [len(_overlap.record(reads, p)) for p in ps]
    got = lengths_of(reads, ps, paired)
    assert got.tolist() == want and int(got.sum()) == len(text)
    assert {len(str(r[4])) for r in reads} == set(range(1, 11))


def test_a_pile_and_an_empty_set():
    """every read on one interval: the order among equal (row, lo) is the ordinals'"""
    reads = [(2, 500, 900 + (i % 7), i & 1, 10 ** (i % 10), 0) for i in range(60)]
    assert _seams.pairs_by_index(reads, 1) == _overlap.pairs(reads, 1) and len(_overlap.pairs(reads, 1)) == 60 * 59 // 2
    assert _seams.pairs_by_index([], 1) == [] and _seams.pairs_by_index([(0, 5, 9, 0, 1, 0)], 5) == []
    assert all(c.shape == (0,) and c.dtype == np.int64 for c in _seams.pair_columns([], [], [], 3))


def test_digit_counts_at_every_power_of_ten():
    v = [0, 1] + [10 ** k - 1 for k in range(1, 20)] + [10 ** k for k in range(1, 20)] + DIGITS + [2**40 - 1, 2**63 - 1]
    assert _seams.dec_digits(np.array(v, dtype=np.uint64)).tolist() == [len(str(x)) for x in v]
    # a record whose every number sits on a power of ten: ids, lengths, coordinates
    reads = [(0, 0, 100_000, 0, 9, 0), (0, 0, 100_000, 1, 1_000_000_000, 0), (0, 99_990, 100_000, 1, 10, 0), (0, 99_999, 100_009, 0, 4_294_967_295, 0)]
    for paired in (False, True):
        rs = [r[:5] + ((1 + (i & 1)) if paired else 0,) for i, r in enumerate(reads)]
        ps = _overlap.pairs(rs, 1)
        assert len(ps) == 6
        assert lengths_of(rs, ps, paired).tolist() == [len(_overlap.record(rs, p)) for p in ps]


# ---- the BAI index from columns (tests/_seams.py:bai_from_columns) against tests/_bai.py:bai_bytes --------------------------------
def same_index(n_ref, ref, lo, end, rec_off, records, base):
    """bai_from_columns equals bai_bytes byte for byte, and the counts it reports are those of the parsed index"""
    counts = {}
    got = _seams.bai_from_columns(n_ref, ref, lo, end, rec_off, base, counts)
    want = _bai.bai_bytes(n_ref, records, base)
    i = next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), min(len(got), len(want)))
    assert got == want, f"{len(got)} bytes against {len(want)}; first difference at byte {i}: {got[i:i + 16].hex()} / {want[i:i + 16].hex()}"
    refs, n_no_coor = _bai.parse_bai(want)
    real = [(b, len(r["bins"][b])) for r in refs for b in r["order"] if b != _bai.META_BIN]
    assert n_no_coor == 0 and counts["bins"].tolist() == [b for b, _ in real] and counts["n_bins"] == len(real)
    assert counts["n_runs"] == sum(c for _, c in real) and counts["max_chunks"] == max([c for _, c in real], default=0)
    assert counts["n_intv"].tolist() == [len(r["ioffset"]) for r in refs]
    return counts, refs


def from_records(n_ref, records, base):
    cols, total = _bai.record_columns(records)
    ref, lo, end, off = (np.array([c[k] for c in cols], dtype=np.int64) for k in range(4))
    return same_index(n_ref, ref, lo, end, np.concatenate([off, [total]]), records, base)


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "paired"])
def test_index_from_columns_on_the_mixed_and_level_records(paired):
    o, t = _bai_cases.columns(_bai_cases.mixed_specs() + _bai_cases.level_specs(), seed=31)
    records, _ = _bai_cases.sorted_records(o, t, paired)
    counts, _ = from_records(len(_bai_cases.REFS), records, len(_bai_cases.header()))
    assert {9, 73, 585} <= set(counts["bins"].tolist()) and set(_seams.bin_level(counts["bins"]).tolist()) >= {2, 3, 4, 5}


def test_index_from_columns_on_three_hundred_references_with_gaps():
    o, t = _bai_cases.columns(_bai_cases.many_specs(), seed=3, contigs=_bai_cases.MANY_CONTIGS)
    records, _ = _bai_cases.sorted_records(o, t, False, _bai_cases.MANY_RNAMES)
    counts, refs = from_records(300, records, len(_bai_cases.header(_bai_cases.MANY_REFS)))
    assert [bool(r["order"]) for r in refs] == [c % 3 != 0 and 0 < c < 299 for c in range(300)]


SMALL_SHAPES = {
    "bin_changes": dict(m=300, big=200, n_ref=1),
    "bin_changes-3": dict(m=300, big=200, n_ref=3),
    "ties": dict(k=9),
    "ties-2": dict(k=2),
    "linear": dict(n_intvs=(255, 256, 257, 512, 513, 32768), long=40),
    "strides": dict(n_ref=21, n=3000),
    "sparse_refs": dict(n_ref=600),
}


@pytest.mark.parametrize("name", SMALL_SHAPES)
def test_index_from_columns_on_every_shape_at_a_small_size(name):
    """the shape builder of tests/test_gpu_bai_seams.py with small sizes, as plain records; the stream starts a few records in
    front of a block edge, so virtual offsets on both sides of one occur"""
    s = _bai_cases.index_shape(name.split("-")[0], **SMALL_SHAPES[name])
    ref, lo, end = s["ref"], s["lo"], s["end"]
    records = b"".join(_bai_cases.plain(r, p, e - p) for r, p, e in zip(ref.tolist(), lo.tolist(), end.tolist()))
    rec_off = _bai_cases.plain_offsets(lo, end)
    assert int(rec_off[-1]) == len(records) and ref.size <= 5000
    counts, refs = same_index(s["n_ref"], ref, lo, end, rec_off, records, 3 * 65280 - 100)
    if name.startswith("bin_changes"):
        assert counts["n_runs"] == ref.size and set(_seams.bin_level(counts["bins"]).tolist()) == {0, 1, 2, 3, 4, 5} and counts["max_chunks"] == 200 + 3  # (bin 0: edge 4096 and edge 8192)
    if name.startswith("ties"):
        assert counts["n_runs"] == ref.size and counts["n_bins"] == 2
    if name == "linear":
        assert counts["n_intv"].tolist() == [255, 256, 257, 512, 513, 32768, 0, 40]
        assert len(set(refs[7]["ioffset"])) == 1 and refs[5]["ioffset"][:511] == [0] * 511 and refs[5]["ioffset"][511] != 0
    if name == "strides":
        assert counts["n_runs"] == ref.size and [bool(r["order"]) for r in refs] == [c % 3 != 0 and 0 < c < 20 for c in range(21)]
    if name == "sparse_refs":
        assert [c for c, r in enumerate(refs) if r["order"]] == [0, 300, 599]


def test_virtual_offsets_of_columns_up_to_the_last_one_of_48_bits():
    """the vectorised virtual offset against _bai.voff around block edges, where the block's file offset passes 2^32, and at the
    largest position whose block starts below 2^48"""
    edge = -(-2**32 // _bai.FRAMED)  # the first block whose file offset is 2^32 or more
    top = (2**48 - 1) // _bai.FRAMED * _bai.BLOCK + _bai.BLOCK - 1
    ps = [0, 1, 65279, 65280, 65281, edge * 65280 - 1, edge * 65280, edge * 65280 + 1, top - 65280, top]
    assert (edge - 1) * _bai.FRAMED < 2**32 <= edge * _bai.FRAMED and _bai.voff(top) < 2**64 <= _bai.voff(top + 1)
    assert _seams.virtual_offsets(np.array(ps, dtype=np.uint64)).tolist() == [_bai.voff(p) for p in ps]
    r0, r1 = _bai_cases.plain(1, 3, 7), _bai_cases.plain(1, 5, 5)
    for base in (100, edge * 65280 - 20, top - len(r0) - len(r1)):
        got = _seams.bai_from_columns(2, [1, 1], [3, 5], [10, 10], [0, len(r0), len(r0) + len(r1)], base)
        assert got == _bai.bai_bytes(2, r0 + r1, base), base


# ---- mapeval from columns (tests/_seams.py:mapeval_from_columns) against tests/_mapeval.py:evaluate ------------------------------------
def same_tables(case, pct, pad, header=b""):
    """both texts of the builder through the plain model: every count, by_mapq, and key / best / hits with their dtypes"""
    res = _seams.mapeval_from_columns(case["names"], case["truth"], case["aligned"], pct, pad, header, case["n_present"])
    m = _mapeval.evaluate(case["names"][:case["n_present"]], [res["truth"]], [res["aligned"]], pct)
    counts, by = m.read()
    assert tuple(res["counts"]) == _mapeval.COUNTS == _seams.MEV_COUNTS
    assert res["counts"] == counts, {n: (res["counts"][n], counts[n]) for n in counts if counts[n] != res["counts"][n]}
    assert res["by_mapq"].dtype == by.dtype and np.array_equal(res["by_mapq"], by)
    for name, want in zip(("key", "best", "hits"), m.entries()):
        assert res[name].dtype == want.dtype and np.array_equal(res[name], want), name
    return res


@pytest.mark.parametrize("pad", [False, True], ids=["unpadded", "padded"])
@pytest.mark.parametrize("pct", [10, 50])
def test_mapeval_from_random_columns(pct, pad):
    """every class: correct, wrong by position, strand and contig, unmapped by flag and by "*", unknown read and reference,
    secondary and supplementary, doubles and drops; overlaps on both sides of the threshold"""
    rng = np.random.default_rng(pct + pad)
    n = 400
    ids = rng.permutation(np.unique(rng.integers(0, 10 ** rng.integers(1, 11, 3 * n))))[:n]  # 1 to 10 digits, distinct
    assert ids.size == n
    truth = dict(id=ids, mate=rng.integers(1, 3, n), strand=rng.integers(0, 2, n), row=rng.integers(0, 3, n), pos=rng.integers(1, 5000, n),
                 span=rng.integers(1, 300, n), mapq=rng.integers(0, 256, n))
    pick = np.concatenate([rng.permutation(n)[:300], rng.integers(0, n, 500)])  # a hundred dropped, many doubled
    m = pick.size
    kind = rng.integers(0, len(_mapeval_cases.KINDS), m)
    is_ = lambda name: kind == _mapeval_cases.KINDS.index(name)
    span = truth["span"][pick]
    shift = np.where(is_("wrong_pos"), span + rng.integers(0, 50, m), np.where(is_("correct"), rng.integers(0, 2, m) * rng.integers(0, 300, m), 0))
    aligned = dict(id=np.where(is_("unknown_read"), 10 ** 11 + np.arange(m), truth["id"][pick]), mate=truth["mate"][pick],
                   strand=truth["strand"][pick] ^ is_("wrong_strand"),
                   row=np.where(is_("wrong_contig"), (truth["row"][pick] + 1) % 3, np.where(is_("unknown_ref"), 3, np.where(is_("unmapped_star"), _seams.MEV_STAR, truth["row"][pick]))),
                   pos=np.where(is_("unmapped_star"), 0, truth["pos"][pick] + shift), span=np.maximum(span + rng.integers(-3, 4, m), 1),
                   mapq=rng.integers(0, 256, m), bits=np.where(is_("unmapped_flag"), 4, np.where(is_("secondary"), 0x100, np.where(is_("supplementary"), 0x800, 0))))
    # the other mate of a known id is an unknown read too
    aligned["mate"] = np.where(rng.integers(0, 20, m) == 0, 3 - aligned["mate"], aligned["mate"])
    case = dict(names=[b"chr1", b"chr10", b"c", b"chrUn"], n_present=3, truth=truth, aligned=aligned)
    res = same_tables(case, pct, pad, b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:9\n")
    c = res["counts"]
    for name in ("secondary", "unknown_read", "unknown_ref", "unmapped", "correct", "wrong", "missing", "multiple", "reads_correct", "reads_wrong", "reads_unmapped"):
        assert c[name] >= 5, name
    assert c["truth_header"] == c["header"] == 2 and c["truth_entries"] == n and c["records"] == m
    width = {len(ln) for ln in res["truth"].split(b"\n")[2:-1]}
    assert len(width) > 1  # (names of three lengths)
    # the threshold is on both sides among the records the builder calls wrong and correct
    assert 0 < (res["by_mapq"][:, 0] > 0).sum() and 0 < (res["by_mapq"][:, 1] > 0).sum()


def test_mapeval_text_is_a_byte_matrix_when_padded():
    case = _mapeval_cases.search(33)
    padded = _seams.mapeval_from_columns(case["names"], case["truth"], case["aligned"], n_present=3)
    plain = _seams.mapeval_from_columns(case["names"], case["truth"], case["aligned"], pad=False, n_present=3)
    assert len({len(ln) for ln in padded["truth"].split(b"\n")[:-1]}) == 1 and len({len(ln) for ln in plain["truth"].split(b"\n")[:-1]}) > 1
    assert padded["truth"].startswith(b"01\t64\ta\t001\t255\t50M\t*\t0\t0\t*\t*\n") and plain["truth"].startswith(b"1\t64\ta\t1\t255\t50M\t*\t0\t0\t*\t*\n")
    for name in ("key", "best", "hits", "by_mapq"):
        assert np.array_equal(padded[name], plain[name])
    assert padded["counts"] == plain["counts"]


SMALL_CASES = {
    "search-1": lambda: _mapeval_cases.search(1),
    "search-17": lambda: _mapeval_cases.search(17),
    "search-257": lambda: _mapeval_cases.search(257),
    "trips": lambda: _mapeval_cases.trips(n=5000, edge=2560, grid_lines=2560, extra=300),
    "trips-tiny": lambda: _mapeval_cases.trips(n=7, edge=4, grid_lines=16, extra=5),
    "every_mapq": _mapeval_cases.every_mapq,
    "many-all": lambda: _mapeval_cases.many_records("all", 700),
    "many-no_correct": lambda: _mapeval_cases.many_records("no_correct", 700),
    "many-unmapped": lambda: _mapeval_cases.many_records("unmapped", 700),
    "names-1": lambda: _mapeval_cases.names(1),
    "names-3": lambda: _mapeval_cases.names(3),
    "names-65": lambda: _mapeval_cases.names(65),
}


@pytest.mark.parametrize("pad", [False, True], ids=["unpadded", "padded"])
@pytest.mark.parametrize("pct", [10, 50])
@pytest.mark.parametrize("name", SMALL_CASES)
def test_mapeval_from_columns_on_every_case_at_a_small_size(name, pct, pad):
    case = SMALL_CASES[name]()
    res = same_tables(case, pct, pad)
    c, best, hits = res["counts"], res["best"], res["hits"]
    if name.startswith("search"):
        assert (hits == 1).all() and np.array_equal(best, 3 << 8 | case["mapq"]) and c["unknown_read"] == case["absent"]
    if name == "trips":
        assert set(case["kind"].tolist()) == set(range(len(_mapeval_cases.KINDS))) and (hits[case["special"]] >= 1).all()
        assert {0, 1, 2, 3} <= set(hits.tolist()) and (res["by_mapq"] > 0).all()
        assert c["reads_correct"] + c["reads_wrong"] + c["reads_unmapped"] + c["missing"] == c["truth_entries"]
        assert (best[-300:] >> 8 == 3).sum() > 50 and (hits[-300:] > 1).sum() > 50
    if name == "every_mapq":
        assert np.array_equal(res["by_mapq"][:, 0], case["right"]) and np.array_equal(res["by_mapq"][:, 1], case["wrong"])
    if name.startswith("many"):
        assert best[37] == case["best"] and hits[37] == case["hits"] == 700
    if name.startswith("names"):
        assert c["unknown_ref"] == case["absent"] and c["wrong"] == case["absent"] + case["moved"] and c["correct"] == c["truth_entries"]


def test_the_lane_round_lines_fall_where_they_are_meant_to():
    """the text case of tests/test_gpu_mapeval_seams.py:test_fields_at_the_lane_rounds holds its edges, and the plain model reads it"""
    lines = _mapeval_cases.lane_lines()
    facts = _mapeval_cases.lane_facts(lines)
    assert facts["first_tab"] >= set(range(1, 19)) and facts["tabs"] == set(range(16)) and facts["newline"] == set(range(16))
    assert facts["cigar_start"] == set(range(16)) and facts["op"] == set(range(16)) and facts["digits"] == set(range(1, 10))
    assert sum(1 for f in lines if len(f) == 11) > 100 and sum(1 for f in lines if len(f) == 12) > 100 and sum(1 for f in lines if len(f) == 41) > 100
    assert lines[-1][10] == b"" and b"\t".join(lines[-1]).count(b"\t") == 10
    truth = b"".join(b"\t".join(f) + b"\n" for f in lines)
    aligned = b"".join(b"\t".join(_mapeval_cases.lane_aligned(f, i)) + b"\n" for i, f in enumerate(lines))
    c, by = _mapeval.evaluate(_mapeval_cases.LANE_NAMES, [truth], [aligned]).read()
    assert c["truth_entries"] == c["records"] == len(lines) == c["correct"] + c["wrong"] and c["correct"] > 100 and c["wrong"] > 80 and (by.sum(axis=1) > 0).sum() == 256
    for o in range(16):
        assert len(_mapeval_cases.pad_line(o)) % 16 == o
    for total in (1, 999_999_999, 10 ** 9, 2 ** 40, 2 ** 40 + 1):
        assert _mapeval.cigar_span(_mapeval_cases.runs_summing_to(total)) == (total, False)


# ---- the pileup from columns (tests/_seams.py:pileup_from_columns) against tests/_pileup.py:pileup -----------------------------------
def same_pileup(cols, sites, lens, chunk_pairs=1 << 24):
    got = _seams.pileup_from_columns(cols, sites, lens, chunk_pairs)
    want = _pileup.pileup(cols, sites, lens)
    assert got.dtype == want.dtype == np.uint32 and got.shape == want.shape == (len(sites[2]), 2, 5)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(_seams.pileup_keys(sites, lens), _pileup.site_keys(sites, lens))
    return got


def mixed_reads(layout, seed):
    """three hundred reads of L in [0, 300) over the three genomes, both strands, some of L = 0, and four that end at their
    contig's last base; the sites: one position in fifty of every contig, and position 0 of the contigs behind those four"""
    rng = np.random.default_rng(seed)
    lens = _pileup_cases.LENS
    g, c, lo, L, rev = _pileup_cases.spread_reads(300, lens, rng, lmax=300)
    L[::17] = 0
    at_end = [(1, 0, 150, 0), (1, 0, 1, 1), (1, 2, 40, 1), (1, 3, 150, 0)]  # (slot, contig, L, reverse)
    g = np.concatenate([g, [a[0] for a in at_end]])
    c = np.concatenate([c, [a[1] for a in at_end]])
    lo = np.concatenate([lo, [lens[a[0]][a[1]] - a[2] for a in at_end]])
    L = np.concatenate([L, [a[2] for a in at_end]])
    rev = np.concatenate([rev, [a[3] for a in at_end]])
    cols = _pileup_cases.read_columns(g, c, lo, L, rev, layout, rng)
    triples = {(s, k, int(p)) for s in lens for k, n in enumerate(lens[s]) for p in np.flatnonzero(rng.random(n) < 0.02)}
    triples |= {(1, 1, 0), (1, 3, 0), (1, 4, 0), (1, 0, lens[1][0] - 1), (1, 2, lens[1][2] - 1)}
    t = sorted(triples)
    return cols, _pileup_cases.site_columns(*([x[i] for x in t] for i in range(3))), lens


@pytest.mark.parametrize("chunk_pairs", [1, 7, 1 << 24])
@pytest.mark.parametrize("layout", [0, 16], ids=["compact", "slot16"])
def test_pileup_from_columns_on_mixed_reads(layout, chunk_pairs):
    cols, sites, lens = mixed_reads(layout, 40 + layout)
    got = same_pileup(cols, sites, lens, chunk_pairs)
    keys = _pileup.site_keys(sites, lens)
    f = _pileup.firsts(lens)
    lo = np.minimum(cols["start"], cols["end"]).astype(np.int64)
    L = np.abs(cols["end"].astype(np.int64) - cols["start"].astype(np.int64))
    klo = np.array([f[(int(a), int(b))] for a, b in zip(cols["genome"], cols["contig"])]) + lo
    n_pairs = np.searchsorted(keys, klo + L) - np.searchsorted(keys, klo)
    # what the reads hold: both strands, L = 0, reads without a site, reads of more pairs than a chunk of 7, all three genomes
    assert set(cols["flags"].tolist()) == {0, 1} and (L == 0).sum() >= 15 and (n_pairs[L > 0] == 0).sum() >= 10 and (n_pairs > 7).sum() >= 10
    assert set(cols["genome"].tolist()) == {0, 1, 3} and int(got.sum()) == int(n_pairs.sum()) > 500
    assert got[:, 0].sum() > 0 and got[:, 1].sum() > 0 and got[:, :, 4].sum() > 0 and (got[:, :, :4].sum(axis=(0, 1)) > 0).all()
    # a read that ends at its contig's last base covers that base and not position 0 of the next contig
    key = {t: i for i, t in enumerate(zip(*(x.tolist() for x in sites)))}
    assert got[key[(1, 0, lens[1][0] - 1)]].sum() >= 2 and got[key[(1, 2, lens[1][2] - 1)]].sum() >= 1
    for first_of_next, behind in (((1, 1, 0), 300), ((1, 3, 0), 302), ((1, 4, 0), 303)):
        assert n_pairs[behind] > 0 and got[key[first_of_next]].sum() == ((klo <= keys[key[first_of_next]]) & (keys[key[first_of_next]] < klo + L)).sum()
    if layout == 16:
        assert (cols["seq_off"][:-1] % 16 != 0).any() and (np.diff(cols["seq_off"].astype(np.int64)) != L).any()


@pytest.mark.parametrize("n_sites", [0, 1])
def test_pileup_from_columns_on_no_site_and_one_site(n_sites):
    cols, sites, lens = mixed_reads(0, 3)
    cover = _pileup_cases.read_columns([1, 1, 1], [1, 1, 1], [500, 520, 601], [150, 150, 9], [0, 1, 1], 0, np.random.default_rng(1))
    one = tuple(x[:n_sites] for x in _pileup_cases.site_columns([1], [1], [600]))
    assert same_pileup(cols, one, lens).shape == (n_sites, 2, 5)
    assert int(same_pileup(cover, one, lens, 1).sum()) == 2 * n_sites


def test_pileup_from_columns_takes_the_tail_of_seq():
    """seq_base: the bytes in front of the first read's are not given, and seq_off counts from the buffer's start"""
    cols, sites, lens = mixed_reads(0, 5)
    want = _pileup.pileup(cols, sites, lens)
    base = 2**32 - 1000
    moved = dict(cols, seq_off=cols["seq_off"] + np.uint64(base))
    assert np.array_equal(_seams.pileup_from_columns(moved, sites, lens, 7, seq_base=base), want) and int(moved["seq_off"].max()) >= 2**32
    cut = int(cols["seq_off"][100])
    tail = dict(cols, seq=cols["seq"][cut:])
    for name in ("start", "end", "contig", "genome", "flags", "seq_off"):
        tail[name] = cols[name][100:]
    assert np.array_equal(_seams.pileup_from_columns(tail, sites, lens, seq_base=cut), want - _pileup.pileup({k: v[:100] if k != "seq" else v for k, v in cols.items() if k not in ("total_bases", "layout")}, sites, lens))
    with pytest.raises(AssertionError):  # bytes that lie in front of the part given
        _seams.pileup_from_columns(tail, sites, lens, seq_base=cut + 1)


BAD_LISTS = {
    "out of order": [(1, 0, 10), (1, 0, 30), (1, 0, 20), (1, 1, 0)],
    "contigs out of order": [(1, 1, 10), (1, 0, 30)],
    "slots out of order": [(0, 0, 5), (3, 0, 5), (1, 0, 5)],
    "a repeat": [(0, 0, 5), (1, 2, 7), (1, 2, 7)],
    "pos == len": [(1, 0, 5), (1, 1, 90_001)],
    "pos == len of the last contig": [(3, 0, 30_000)],
    "an unstaged slot": [(1, 0, 5), (2, 0, 0)],
    "a slot beyond the table": [(77, 0, 0)],
    "a contig that does not exist": [(0, 0, 1), (1, 5, 0)],
}


@pytest.mark.parametrize("name", BAD_LISTS)
def test_pileup_keys_refuses_what_the_model_refuses(name):
    bad = _pileup_cases.site_columns(*([t[i] for t in BAD_LISTS[name]] for i in range(3)))
    for keys_of in (_pileup.site_keys, _seams.pileup_keys):
        with pytest.raises(AssertionError):
            keys_of(bad, _pileup_cases.LENS)
    good = tuple(x[:1] for x in bad) if name not in ("pos == len of the last contig", "a slot beyond the table") else _pileup_cases.site_columns([3], [0], [29_999])
    assert _seams.pileup_keys(good, _pileup_cases.LENS).tolist() == _pileup.site_keys(good, _pileup_cases.LENS).tolist()
    none = _pileup_cases.site_columns([], [], [])
    assert _seams.pileup_keys(none, _pileup_cases.LENS).shape == (0,) and _seams.pileup_keys(none, {}).shape == (0,)


def test_pileup_constants_come_from_the_kernel_file():
    wg, round_pairs, per_cu = _pileup.constants()
    assert all(isinstance(v, int) and v > 0 for v in (wg, round_pairs, per_cu))
    assert wg % 64 == 0 and 64 * round_pairs < 2**31


# ---- the small cases of tests/test_gpu_pileup_seams.py through the plain model ------------------------------------------------------
def pairs_per_read(cols, sites, lens):
    """how many sites every read covers, from the model's keys and the model's two searchsorted calls"""
    keys = _pileup.site_keys(sites, lens)
    f = _pileup.firsts(lens)
    lo = np.minimum(cols["start"], cols["end"]).astype(np.int64)
    L = np.abs(cols["end"].astype(np.int64) - cols["start"].astype(np.int64))
    klo = np.array([f[(int(a), int(b))] for a, b in zip(cols["genome"], cols["contig"])], dtype=np.int64) + lo
    s0 = np.searchsorted(keys, klo, side="left")
    return np.searchsorted(keys, klo + L, side="left") - s0, s0


@pytest.mark.parametrize("which", _pileup_cases.STRANDS)
@pytest.mark.parametrize("name", _pileup_cases.STEP_COUNTS)
def test_step_cases_hold_their_counts(name, which):
    reads, sites, counts = _pileup_cases.step_case(name, which)
    cols = _pileup_cases.read_columns(*reads, 0, np.random.default_rng(2))
    got = same_pileup(cols, sites, _pileup_cases.LENS, 64)
    n_pairs, _ = pairs_per_read(cols, sites, _pileup_cases.LENS)
    assert np.array_equal(n_pairs, counts) and np.array_equal(counts[:64], counts[128:]) and not counts[64:128].any()
    assert int(got.sum()) == int(counts.sum()) and int((got.sum(axis=(1, 2)) == 0).sum()) == 96  # (the sites in front of every other read)
    prefix = np.cumsum(_pileup_cases.STEP_COUNTS[name])
    if name == "edges_64_128_256":
        assert {64, 128, 256} <= set(prefix.tolist()) and prefix[-1] == 321 and prefix[8] == 321
    if name == "edges_reversed":  # (the first pairs belong to lane 55, the last 64 to lane 63; one edge stays on a step's end)
        assert not prefix[:55].any() and prefix[55:].tolist() == [65, 65, 65, 193, 256, 257, 257, 257, 321]
    if name == "lanes_31_32":
        assert prefix[-1] % 64 == 1 and prefix[30] == 0 and 0 < prefix[31] < prefix[32] == prefix[63]


@pytest.mark.parametrize("before", [0, 3])
@pytest.mark.parametrize("m", [149, 150, 151, 152])
def test_list_end_cases_end_where_they_say(m, before):
    reads, sites, = _pileup_cases.list_end_case(m, before)
    cols = _pileup_cases.read_columns(*reads, 0, np.random.default_rng(3))
    got = same_pileup(cols, sites, _pileup_cases.LENS, 100)
    n_pairs, s0 = pairs_per_read(cols, sites, _pileup_cases.LENS)
    n, L = len(sites[2]), _pileup_cases.END_L
    assert n - s0[0] == n - s0[1] == m and n_pairs[0] == n_pairs[1] == min(m, L)
    assert n_pairs.tolist() == [min(m, L)] * 2 + [0] * 4 + [n] * 2 + [min(m - 75, L)] * 2 + [before] * 2 + [1] * 2 + [0] * 2
    assert got[:, 0].sum() == got[:, 1].sum() == n_pairs.sum() // 2


@pytest.mark.parametrize("pos", [(40_000,), (40_000, 40_001), (40_000, 40_149), (40_000, 40_150)], ids=lambda p: f"{len(p)}-{p[-1] - p[0]}")
def test_short_list_cases(pos):
    reads, sites = _pileup_cases.short_list_case(np.array(pos))
    cols = _pileup_cases.read_columns(*reads, 16, np.random.default_rng(4))
    got = same_pileup(cols, sites, _pileup_cases.LENS, 3)
    n_pairs, _ = pairs_per_read(cols, sites, _pileup_cases.LENS)
    two = len(pos) - 1
    second = lambda lo, L: int(two and lo <= pos[-1] < lo + L)
    p = pos[0]
    want = [1 + second(p, 150), 1 + second(p - 149, 150), 0, second(p + 1, 150), 0, 0, 1 + two, 1, 0]
    assert n_pairs.tolist() == [x for x in want for _ in range(2)] and int(got.sum()) == 2 * sum(want)


@pytest.mark.parametrize("identical", [False, True], ids=["every offset", "one read"])
def test_deep_case_at_a_small_depth(identical):
    rng = np.random.default_rng(6)
    reads, sites = _pileup_cases.deep_case(700, identical, rng)
    cols = _pileup_cases.read_columns(*reads, 0, rng, shared=identical)
    got = same_pileup(cols, sites, _pileup_cases.LENS, 50)
    assert got[2].sum() == 700 and got[0].sum() == got[4].sum() == 0
    if identical:
        assert got[2].max() == 700 and got[1].sum() == 0 and got[3].sum() == 0
    else:
        assert got[2, 0].sum() == got[2, 1].sum() == 350 and got[1].sum() > 0 and got[3].sum() > 0
