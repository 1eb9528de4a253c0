"""The fast restatements of tests/_seams.py against the plain model of tests/_overlap.py on a few hundred reads: the pairs by
index equal _overlap.pairs entry for entry, and every vectorised record length equals the length of the line _overlap.record
formats.  Runs without a GPU."""
import numpy as np
import pytest

from tests import _overlap, _seams

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
