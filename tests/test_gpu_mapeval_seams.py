"""The mapeval unit (simmr_mapeval_*; mapeval.hip, mapeval_kernels.hip) past its first batch, search round, name round and grid
trip.  Every test compares every table and column with its reference — the counts, by_mapq, and key / best / hits of every entry —
and asserts that its edge was entered.  The reference is the plain model (tests/_mapeval.py:evaluate) wherever a few thousand
lines do, and tests/_seams.py:mapeval_from_columns, which tests/test_seams_host.py holds to that model table for table, where the
sizes follow from the grids.  The cases are those of tests/_mapeval_cases.py, which the host test runs at a small size.

Which loop each test is the first to enter:
  test_the_search_at_every_size_and_position
      mev_lower_bound at n = 16^k and 16^k +- 1 (the step changes, the last pivot falls on b), every position looked up, every
      gap between two keys, below the first and behind the last key looked up, and keys that differ from a present one in bit 0;
  test_second_trips_of_records_entries_and_tiles
      the second trip of k_mev_gather (more than 256 x 32 x CUs entries), the second and third of k_mev_reduce (256 x 16 x CUs:
      l_sum zeroed between trips), k_mev_index past 16 x CUs tiles, the second trip of k_mev_record's batch loop (more than
      16 x 8 x CUs lines): l_mapq carried across batches, every MAPQ twice in one workgroup; the truth's k_mev_truth loops too;
  test_every_mapq_in_both_columns
      rows 61 .. 254 of l_mapq and of its flush, with counts that differ per row and column;
  test_one_entry_many_records
      atomicMax on best[] and atomicAdd on hits[] with 40 000 records on one entry: the order of the classes settled among many;
  test_the_name_table_at_its_rounds_and_sizes
      mev_name_row over 2^k and 2^k +- 1 names, mev_compare where names share 15 .. 48 and 253 bytes (a difference in the first
      and the last lane of a round, a name and its extension), absent names between two present ones;
  test_nothing_and_keys_without_bits
      truth_plan without entries (n1 = 1, no sort, no gather) and with key_bits == 0 (k_mev_gather with perm == nullptr);
  test_fields_at_the_lane_rounds
      mev_read_line with the first tab at offsets 1 .. 18, every later tab, the newline, the CIGAR's start and its op bytes on
      every lane, runs of 1 .. 9 digits read back across a round, 0, 1 and 30 optional fields, ten tabs and an empty QUAL, the
      line's start at each of 16 offsets, and CIGAR sums beyond 2^32;
  test_limits_accepted_and_refused
      POS 2^31 - 1 and an end of 2^40 on the accepted side, an end of 2^40 + 1 refused on either side."""
import re
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import SimmrError, _abi
from tests import _mapeval, _mapeval_cases, _seams
from tests.test_gpu_mapeval import against_model, line, same

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def _define(name, macro):
    return int(re.search(rf"^#define\s+{macro}\s+(\d+)u?\b", (CSRC / name).read_text(), re.M).group(1))


MEV_WG_RECS = _define("mapeval_kernels.hip", "MEV_WG_RECS")
MEV_MIN_LINE = _define("mapeval_kernels.hip", "MEV_MIN_LINE")
FSAM_TILE = _define("fit_sam_kernels.hip", "FSAM_TILE")
SAM_RNAME_MAX = _define("sam_kernels.hip", "SAM_RNAME_MAX")
SAMSORT_PAIRS_TILE = int(re.search(r"SAMSORT_PAIRS_TILE = (\d+)", (CSRC / "engine_internal.hpp").read_text()).group(1))
WG = 256          # threads of a workgroup of k_mev_gather and k_mev_reduce: an entry a thread
RECORD_WGS = 8    # workgroups per CU of k_mev_record and k_mev_truth (mapeval.hip: enqueue_index)
REDUCE_WGS = 16   # of k_mev_reduce (simmr_mapeval_read)
GATHER_WGS = 32   # of k_mev_gather (simmr_mapeval_truth_plan)
INDEX_WGS = 16    # of k_mev_index, a tile of FSAM_TILE bytes a trip
LANES = 16        # lanes that share a line, a search round and a comparison round


def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


class Tables:
    """the builder's tables with the reading methods of the plain model (what test_gpu_mapeval.py:same compares)"""

    def __init__(self, res):
        self.res = res

    def read(self):
        return self.res["counts"], self.res["by_mapq"]

    def entries(self):
        return self.res["key"], self.res["best"], self.res["hits"]


def run_case(engine, case, what, pct=10, pad=True, model=False):
    """the case's texts through the device against the builder's tables, and against the plain model too where asked"""
    res = _seams.mapeval_from_columns(case["names"], case["truth"], case["aligned"], pct, pad, n_present=case["n_present"])
    table = case["names"][:case["n_present"]]
    ev = engine.mapeval(table, pct)
    ev.truth_add(res["truth"])
    assert ev.truth_plan() == res["key"].size, what
    ev.add(res["aligned"])
    same(ev, Tables(res), what)
    if model:
        same(ev, _mapeval.evaluate(table, [res["truth"]], [res["aligned"]], pct), what + " (the plain model)")
    ev.close()
    return res


SEARCH_SIZES = [1, 2, 15, 16, 17, 18, 31, 32, 33, 255, 256, 257, 272, 4095, 4096, 4097, 65535, 65536, 65537]


@pytest.mark.parametrize("n", SEARCH_SIZES)
def test_the_search_at_every_size_and_position(engine, n):
    """up to 4097 entries against the plain model (and the builder), beyond against the builder; up to 33 with unpadded numbers"""
    case = _mapeval_cases.search(n)
    res = run_case(engine, case, f"search over {n} entries", pad=n > 33, model=n <= 4097)
    c = res["counts"]
    assert any(n in (LANES ** k - 1, LANES ** k, LANES ** k + 1) for k in range(5)) or n in (2, 18, 31, 32, 33, 272)
    assert c["truth_entries"] == n and (res["hits"] == 1).all() and np.array_equal(res["best"], 3 << 8 | case["mapq"])  # every position found, once
    assert c["unknown_read"] == case["absent"] == 2 * n + 1 + (n + 6) // 7 and c["correct"] == n and c["missing"] == 0
    ids = np.asarray(case["aligned"]["id"])
    assert ids.min() == 0 and ids.max() > int(res["key"][-1] >> 1) and np.isin(np.asarray(case["truth"]["id"]) + 1, ids).all()


def test_second_trips_of_records_entries_and_tiles(engine):
    cus = n_cu()
    grid = RECORD_WGS * cus
    n, edge, grid_lines = WG * GATHER_WGS * cus + 300, WG * REDUCE_WGS * cus, MEV_WG_RECS * grid
    case = _mapeval_cases.trips(n, edge, grid_lines, extra=300, tail=300)
    res = run_case(engine, case, f"{n} entries, {grid_lines + 300} records")
    c, hits, best, by = res["counts"], res["hits"], res["best"], res["by_mapq"]
    assert c["truth_entries"] == n > WG * GATHER_WGS * cus and n > 2 * WG * REDUCE_WGS * cus         # k_mev_gather's second trip, k_mev_reduce's third
    assert n > SAMSORT_PAIRS_TILE * WG                                                              # the sort's histogram scan past 256 tiles
    assert len(res["truth"]) > FSAM_TILE * INDEX_WGS * cus                                           # k_mev_index loops
    assert len(res["truth"]) // (MEV_WG_RECS * MEV_MIN_LINE) + 1 >= grid and c["truth_lines"] > MEV_WG_RECS * grid  # k_mev_truth loops
    assert len(res["aligned"]) // (MEV_WG_RECS * MEV_MIN_LINE) + 1 >= grid                           # the grid is 8 x CUs workgroups
    assert c["records"] == grid_lines + 300 > MEV_WG_RECS * grid                                     # k_mev_record's second trip
    mapq, kind = case["mapq"], case["kind"]
    assert np.array_equal(mapq[:300], mapq[grid_lines:]) and np.array_equal(kind[:300], kind[grid_lines:]) and set(mapq[:300].tolist()) == set(range(256))
    assert (by > 0).all() and set(kind.tolist()) == set(range(len(_mapeval_cases.KINDS)))             # every MAPQ in both columns, every class
    assert (hits[case["special"]] >= 1).all() and case["special"].tolist() == [n - 1, edge - 2, edge - 1, edge, edge + 1, 0]
    assert {0, 1, 2, 3} <= set(hits.tolist())
    assert c["missing"] == int((hits == 0).sum()) and c["multiple"] == int((hits > 1).sum()) > 100
    assert c["reads_correct"] + c["reads_wrong"] + c["reads_unmapped"] + c["missing"] == n
    assert min(c["reads_correct"], c["reads_wrong"], c["reads_unmapped"]) > 1000 and c["missing"] > n - grid_lines - 300
    for lo, hi in ((0, edge), (edge, 2 * edge), (2 * edge, n)):  # every trip of k_mev_reduce has entries of every class
        assert {0, 1, 2, 3} <= set((best[lo:hi] >> 8).tolist())
    assert 2 * edge == WG * GATHER_WGS * cus and (best[2 * edge:] >> 8 == 3).sum() > 50 and (hits[2 * edge:] > 1).sum() > 50  # k_mev_gather's second trip brought entries that records hit


@pytest.mark.parametrize("pad", [False, True], ids=["unpadded", "padded"])
def test_every_mapq_in_both_columns(engine, pad):
    case = _mapeval_cases.every_mapq()
    res = run_case(engine, case, "every MAPQ", pad=pad, model=True)
    q = np.arange(256)
    assert np.array_equal(res["by_mapq"][:, 0], 1 + q % 5) and np.array_equal(res["by_mapq"][:, 1], 1 + q % 3) and 1000 < res["counts"]["records"] < 5000


@pytest.mark.parametrize("which,best,m", [("all", 3 << 8 | 17, 2_000), ("all", 3 << 8 | 17, 40_000), ("no_correct", 2 << 8 | 200, 40_000), ("unmapped", 1 << 8 | 255, 40_000)],
                         ids=["all-2000-unpadded", "all", "no_correct", "unmapped"])
def test_one_entry_many_records(engine, which, best, m):
    case = _mapeval_cases.many_records(which, m)
    res = run_case(engine, case, f"{m} records on one entry ({which})", pad=m > 2_000, model=m <= 2_000)
    assert res["best"][37] == best == case["best"] and res["hits"][37] == m and res["counts"]["multiple"] == 1
    mapq, entry = np.asarray(case["aligned"]["mapq"]), np.asarray(case["aligned"]["id"]) == case["truth"]["id"][37]
    assert int(mapq[entry].max()) == 255 and (which == "unmapped" or best & 255 < 255)  # the class decides, not the MAPQ


@pytest.mark.parametrize("n", [1, 2, 3, 1023, 1024, 1025, 5000])
def test_the_name_table_at_its_rounds_and_sizes(engine, n):
    case = _mapeval_cases.names(n)
    table = sorted(case["names"][:n])
    absent = case["names"][n:]
    res = run_case(engine, case, f"{n} names", pad=n != 3, model=True)
    c = res["counts"]
    assert c["unknown_ref"] == len(absent) == case["absent"] and c["wrong"] == len(absent) + case["moved"] and c["correct"] == c["truth_entries"] >= n
    assert np.isin(np.arange(n), np.asarray(case["truth"]["row"])).all() and 0 < c["records"] < 9000
    assert min(absent) < table[0] and max(absent) > table[-1] and max(map(len, absent)) == SAM_RNAME_MAX + 1
    between = sum(1 for x in absent if table[0] < x < table[-1])
    assert between >= (2 if n > 1 else 0)
    if n >= 35:
        shared = {_mapeval_cases.shared_prefix(a, b) for a, b in zip(table, table[1:])}
        assert set(_mapeval_cases.SHARED) <= shared and {p + 1 for p in _mapeval_cases.SHARED if p < 253} <= shared  # (+ 1: a name and its extension)
        assert between > 100 and max(map(len, table)) == SAM_RNAME_MAX


def test_nothing_and_keys_without_bits(engine):
    names = ["c0", "c1"]
    nothing = (b"@HD\tVN:1.6\n@SQ\tSN:c0\tLN:1000\n" + line(5, 4, "c0", 10, 60, "20M") + line(6, 0x100, "c0", 10, 60, "20M") +
               line(7, 0x800, "c0", 10, 60, "20M") + line(8, 0, "c0", 10, 60, "5M9N5M"))
    records = line(0, 0, "c0", 10, 60, "20M") + line(5, 0, "c0", 10, 7, "20M") + line(8, 0x80, "c1", 10, 0, "20M") + line(9, 4, "*", 0, 0, "*")
    ev = engine.mapeval(names)
    ev.truth_add(nothing)
    assert ev.truth_plan() == 0
    ev.add(records)
    model = _mapeval.evaluate(names, [nothing], [records])
    counts, by = same(ev, model, "no entries")
    assert counts["truth_lines"] == 6 and counts["truth_header"] == 2 and counts["truth_skipped"] == 4 and counts["truth_entries"] == 0
    assert counts["unknown_read"] == counts["records"] == 4 and counts["missing"] == 0 and by.sum() == 0
    key, best, hits = ev.entries()
    assert (key.shape, best.shape, hits.shape) == ((0,),) * 3 and (key.dtype, best.dtype, hits.dtype) == (np.uint64, np.uint32, np.uint32)
    ev.close()
    # one entry whose key is 0: no bit to sort over; its own record, the other mate, id 1
    zero = line(0, 16, "c1", 10, 60, "20M")
    lookups = line(0, 16, "c1", 12, 33, "20M") + line(0, 0x80 | 16, "c1", 12, 34, "20M") + line(1, 16, "c1", 12, 35, "20M") + line(0, 0, "c1", 12, 36, "20M")
    counts, _ = against_model(engine, names, [nothing, zero], [lookups], "one entry of key 0")
    assert counts["truth_entries"] == 1 and counts["correct"] == 1 and counts["wrong"] == 1 and counts["unknown_read"] == 2 and counts["multiple"] == 1
    # both mates of id 0: keys 0 and 1, one bit
    both = zero + line(0, 0x80, "c0", 50, 60, "20M")
    counts, _ = against_model(engine, names, [both], [lookups], "keys 0 and 1")
    assert counts["truth_entries"] == 2 and counts["correct"] == 1 and counts["wrong"] == 2 and counts["unknown_read"] == 1 and counts["missing"] == 0


def test_fields_at_the_lane_rounds(engine):
    lines = _mapeval_cases.lane_lines()
    facts = _mapeval_cases.lane_facts(lines)
    assert facts["first_tab"] >= set(range(1, 19)) and facts["tabs"] == set(range(LANES)) and facts["newline"] == set(range(LANES))
    assert facts["cigar_start"] == set(range(LANES)) and facts["op"] == set(range(LANES)) and facts["digits"] == set(range(1, 10))
    assert {len(f) - 11 for f in lines} == {0, 1, 30} and lines[-1][10] == b"" and len(lines[-1]) == 11
    assert max(map(len, _mapeval_cases.LANE_NAMES)) == 40
    text = lambda fs: b"\t".join(fs) + b"\n"
    # sixteen adds a side: a comment line in front puts the first record at each offset of a round
    step = -(-len(lines) // LANES)
    truth = [_mapeval_cases.pad_line(o) + b"".join(text(f) for f in lines[o * step:(o + 1) * step]) for o in range(LANES)]
    aligned = [_mapeval_cases.pad_line(o) + b"".join(text(_mapeval_cases.lane_aligned(f, i)) for i, f in list(enumerate(lines))[o * step:(o + 1) * step])
               for o in range(LANES)]
    assert {t.index(b"\n") + 1 for t in truth} == set(range(LANES, 2 * LANES))
    for pct in (10, 50):
        counts, by = against_model(engine, _mapeval_cases.LANE_NAMES, truth, aligned, f"lane rounds, {pct} per cent", pct)
        assert counts["truth_entries"] == counts["records"] == len(lines) == counts["correct"] + counts["wrong"] and counts["header"] == LANES
        assert counts["correct"] > 100 and counts["wrong"] > 80 and (by.sum(axis=1) > 0).sum() == 256
    # a span beyond 2^32.  POS ends at 2^31 - 1, so an interval cannot start 2^32 further on; its END can lie 2^32 further on:
    # five runs of 999999999 against the same less 2^32, from one POS.  The two spans are equal in their low 32 bits; the overlap
    # is 14.1 per cent of the union: correct at 10 per cent, wrong at 50, either way round.
    long_cigar = _mapeval_cases.runs_summing_to(5 * 999_999_999)
    short_cigar = _mapeval_cases.runs_summing_to(5 * 999_999_999 - 2 ** 32)
    assert long_cigar == b"999999999M" * 5 and 5 * 999_999_999 > 2 ** 32 and 10 * (5 * 999_999_999 - 2 ** 32) < 5 * 5 * 999_999_999
    names = ["c0"]
    truth = line(1, 0, "c0", 7, 255, long_cigar) + line(2, 0, "c0", 7, 255, short_cigar)
    aligned = line(1, 0, "c0", 7, 11, long_cigar) + line(1, 0, "c0", 7, 12, short_cigar) + line(2, 0, "c0", 7, 13, long_cigar) + line(2, 0, "c0", 7, 14, short_cigar)
    for pct, correct in ((10, 4), (50, 2)):
        counts, by = against_model(engine, names, [truth], [aligned], f"spans beyond 2^32, {pct} per cent", pct)
        assert counts["correct"] == correct and counts["wrong"] == 4 - correct and by[11, 0] == by[14, 0] == 1 and by[12, 1] == by[13, 1] == (pct == 50)


END = _mapeval.MAX_END
AT_END = {
    "POS 2^31 - 1": (2 ** 31 - 1, b"100M"),
    "end 2^40 from POS 1": (1, _mapeval_cases.runs_summing_to(END)),
    "end 2^40 from POS 2^31 - 1": (2 ** 31 - 1, _mapeval_cases.runs_summing_to(END - (2 ** 31 - 2))),
}
PAST_END = {
    "end 2^40 + 1 from POS 1": (1, _mapeval_cases.runs_summing_to(END + 1)),
    "end 2^40 + 1 from POS 2^31 - 1": (2 ** 31 - 1, _mapeval_cases.runs_summing_to(END + 1 - (2 ** 31 - 2))),
    "end 2^40 + 1 with D and =": (2, _mapeval_cases.runs_summing_to(END - 2).replace(b"M", b"=") + b"1D1M"),
}


def test_limits_accepted_and_refused(engine):
    names = ["c0", "c1"]
    assert END == 2 ** 40 and _mapeval.MAX_POS == 2 ** 31 - 1
    for k, (pos, cigar) in enumerate(AT_END.values()):
        assert pos - 1 + _mapeval.cigar_span(cigar)[0] in (END, 2 ** 31 + 98)
    truth = b"".join(line(k + 1, 16, "c1", pos, 255, cigar) for k, (pos, cigar) in enumerate(AT_END.values()))
    aligned = b"".join(line(k + 1, 16, "c1", pos, 40 + k, cigar) + line(k + 1, 16, "c1", pos - 1, 50 + k, cigar) + line(k + 1, 16, "c1", 1, 60 + k, b"1M")
                       for k, (pos, cigar) in enumerate(AT_END.values()) if pos > 1)
    aligned += line(2, 16, "c1", 1, 45, AT_END["end 2^40 from POS 1"][1]) + line(2, 16, "c1", 2 ** 31 - 1, 46, b"1M")
    for pct in (10, 100):
        counts, by = against_model(engine, names, [truth], [aligned], f"at the limits, {pct} per cent", pct)
        assert counts["truth_entries"] == 3 and counts["records"] == 8 and counts["correct"] + counts["wrong"] == 8
        moved = 0 if pct == 10 else 1  # a base to the left: correct unless the whole union has to overlap
        assert by[40, 0] == by[42, 0] == by[45, 0] == 1 and by[46, 1] == by[60, 1] == by[62, 1] == 1 and by[50, moved] == by[52, moved] == 1
    good = line(9, 0, "c0", 10, 60, "20M")
    for what, (pos, cigar) in PAST_END.items():
        bad = line(7, 0, "c0", pos, 60, cigar)
        assert pos - 1 + _mapeval.cigar_span(cigar)[0] == END + 1, what
        with pytest.raises(_mapeval.Malformed):
            _mapeval.Model(names).truth_add(bad)
        with pytest.raises(_mapeval.Malformed):
            _mapeval.evaluate(names, [good], [bad])
        ev = engine.mapeval(names)
        ev.truth_add(good + bad)
        with pytest.raises(SimmrError) as ei:
            ev.truth_plan()
        assert ei.value.code == _abi.EINVAL and "malformed" in ei.value.msg, what
        ev.reset(names)
        ev.truth_add(good)
        assert ev.truth_plan() == 1
        ev.add(good + bad + good)
        with pytest.raises(SimmrError) as ei:
            ev.read()
        assert ei.value.code == _abi.EINVAL and "malformed" in ei.value.msg, what
        ev.close()
