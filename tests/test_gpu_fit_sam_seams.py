"""The SAM route of the model fit (simmr_fit_add_sam; fit_sam.hip, fit_sam_kernels.hip) past its first round, tile, scan chunk
and grid trip.  Every test takes its texts from tests/_fit_sam_cases.py, whose builders assert that each byte sits on the lane,
tile or trip it is for, runs them through test_gpu_fit_sam.py's against_restatement — the device model against the plain
restatement of the header's rules (tests/_fit_sam.py) table for table, and fit_sam_counts() against its counts — and then
asserts that the case did what it is for.  tests/test_fit_sam_host.py pins where every case lands without a GPU.

Which path each test is the first to enter:
  test_md_rounds
      fsam_md_lane's letters-only round (non == 0): a '^' run of 33 and 48 letters and 40 adjacent mismatch letters carry in_del
      through whole rounds, in k_fsam_record and in k_fsam_md; '^' on lane 15, a 0 on lane 15 and on lane 0 between a '^' run and a
      mismatch; numbers of 1, 2 and 9 digits read back over the seam, 10 digits refused; MD of 15 .. 33 bytes at every place
      among the optional fields; MD's end at the text's end;
  test_cigar_rounds
      fsam_cigar_lane with an op on lane 0 and its digits in the round before, runs of nine digits, runs of zero of every op
      under k_fsam_expand's run search, rounds of 15, 16 and 17 columns, a run of 1000 columns dealt to 16 lanes;
  test_rows_and_tables
      k_fsam_windows where a changed column stands on either side of columns 16, 256 and 512 (the lane's group, carry_w / carry_h
      from lane 15 to lane 0), with the dense table in LDS (k <= 7) and in HBM (k = 8, 10); k_fsam_record's quality table where
      offset 160 leaves LDS, on both strands;
  test_line_shift
      every tab and newline on every lane of the field scan, every line start on every byte of an index thread's 16;
  test_record_trips, test_malformed_kinds
      k_fsam_record's batch loop past three trips a workgroup, the sticky error word set from a late trip;
  test_scan_chunk
      k_fsam_scan's second iteration (more than 256 tiles), a line start on both sides of its seam;
  test_index_trips
      k_fsam_index's second trip (more than 16 x CUs tiles), both launches;
  test_taken_trips
      k_fsam_md and k_fsam_expand past two trips, k_fsam_windows past three turns of its two-slot column counter;
  test_split_invariance
      the same tables from one add and from four."""
from collections import Counter

import ctypes as C
import numpy as np
import pytest

from simmr_amd import SimmrError, _abi
from tests import _fit, _fit_sam
from tests import _fit_sam_cases as cases
from tests.test_fit_sam_host import fit_repeated
from tests.test_gpu_fit_sam import against_restatement, fit_sam, same_model

pytestmark = pytest.mark.gpu


def n_cu():
    """the count fit_sam.hip sizes its grids from: hipDeviceProp_t::multiProcessorCount, which the binding does not expose"""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def landed(counts, items, extra_taken=0):
    """every counter holds what the builder says its items land in"""
    want = Counter(i.lands for i in items)
    want["taken_alignment"] += extra_taken
    for name in _fit_sam.COUNTS:
        if name.startswith("skip_") or name == "taken_alignment":
            assert counts[name] == want[name], name
    assert counts["records"] == len(items) + extra_taken


def only(engine, item, k=7):
    """the counters of one line between two good records"""
    fit_sam(engine, [cases.GOOD + item.line + (b"" if item.last else cases.GOOD)], 1, k)
    c = engine.fit_sam_counts()
    assert c["taken_alignment"] == (1 if item.last else 2) + (item.lands == "taken_alignment")
    return c


def test_md_rounds(engine):
    items = [i for flag in cases.STRANDS for i in cases.md_rounds(flag)]
    texts = cases.texts_of(items)
    _, counts = against_restatement(engine, texts, 1, 7, "MD rounds")
    landed(counts, items, extra_taken=len(texts) - 1)
    by = {i.what: i for i in items}
    for flag in cases.STRANDS:
        assert only(engine, by[f"a number of 10 digits over the seam, flag {flag}"])["skip_inconsistent"] == 1
        assert only(engine, by[f"MD:Z:9 as RNEXT and no MD behind QUAL, flag {flag}"])["skip_no_md"] == 1
        assert only(engine, by[f"the text ends inside the tag, flag {flag}"])["skip_no_md"] == 1
        assert only(engine, by[f"the text ends in an empty MD, the CIGAR has 4M, flag {flag}"])["skip_inconsistent"] == 1
        only(engine, by[f"the text ends in an empty MD, the CIGAR has no M, flag {flag}"])
        # the letters-only rounds, alone: a record and the model of its 48 deleted and 40 changed bases
        for what in (f"^ run of 48 letters, shift 1, flag {flag}", f"40 adjacent mismatch letters, shift 0, flag {flag}"):
            got, c = against_restatement(engine, [by[what].line], 1, 3, what)
            assert c["taken_alignment"] == 1 and got["n_pairs"] > got["n_ref_kmers"] > 0


def test_cigar_rounds(engine):
    items = [i for flag in cases.STRANDS for i in cases.cigar_rounds(flag)]
    got, counts = against_restatement(engine, cases.texts_of(items), 1, 7, "CIGAR rounds")
    landed(counts, items)
    assert counts["skip_cigar_op"] == 8 and counts["skip_inconsistent"] == 0 and got["n_positions"] >= 1000
    by = {i.what: i for i in items}
    for what in ("0D twice in a row, flag 16", "0M: the 0 on lane 15, the op on lane 0, flag 0", "a round of 16 columns ending on its last op, flag 16",
                 "eight one-digit ops, then one run of 1000 columns, flag 16"):
        _, c = against_restatement(engine, [by[what].line], 1, 3, what)
        assert c["taken_alignment"] == 1


@pytest.mark.parametrize("k", cases.KS)
def test_rows_and_tables(engine, k):
    items, (q_items, q_want) = cases.window_rows(k), cases.quality_offsets()
    text = b"".join(i.line for i in items + q_items)
    got, counts = against_restatement(engine, [text], 1, k, f"rows at the columns {cases.EDGES}, k {k}")
    assert counts["taken_alignment"] == counts["records"] == len(items) + len(q_items)
    assert (k <= cases.LDS_K) == (k in (3, 7)) and got["n_pairs"] > got["n_ref_kmers"] > 0
    assert got["n_positions"] == max(cases.EDGES) + k + 3 and got["length_hist"][cases.LDS_POS] == 4 and got["length_hist"][cases.LDS_POS - 1] == 4
    for off in (158, 159, 160, 161):  # the qualities of their own at the offsets around FIT_LDS_POS, both strands
        assert {q: int(n) for q, n in enumerate(got["qual_hist"][off]) if n} == q_want[off], off


def test_line_shift(engine):
    texts, items = cases.line_shift()
    _, counts = against_restatement(engine, texts, 1, 7, "QNAMEs of 1 .. 16 bytes")
    want = Counter(i.lands for i in items)
    assert counts["records"] == cases.LANES * len(items) and all(counts[n] == cases.LANES * want[n] for n in want)


def test_record_trips(engine):
    case = cases.record_trips_text(n_cu())
    assert case["n_batches"] > 3 * case["grid"] and case["grid"] == cases.rec_grid(len(case["text"]), n_cu())
    _, counts = against_restatement(engine, [case["text"]], 1, 7, "records among two-byte header lines")
    landed(counts, case["items"])
    assert counts["lines"] == case["n_lines"] and counts["header_lines"] == case["n_lines"] - len(case["items"])


def test_scan_chunk(engine):
    made = cases.scan_chunk_texts()
    assert all(c["n_tiles"] > cases.SCAN_CHUNK + 1 for c in made)
    _, counts = against_restatement(engine, [c["text"] for c in made], 1, 7, "a record on both sides of the scan's seam")
    assert counts["taken_alignment"] == counts["records"] == sum(c["taken"] for c in made)


def test_index_trips(engine):
    cus = n_cu()
    case = cases.index_trips_text(cus)
    assert case["n_tiles"] == cases.INDEX_WGS * cus + 2 > cases.INDEX_WGS * cus
    import torch
    try:
        text = torch.from_numpy(np.frombuffer(case["text"], dtype=np.uint8).copy()).to(engine.device)
        engine.fit_reset(7, 20, 1 << 18)
        engine.fit_add_sam(text, 1)
        got = engine.fit_model()
    except (SimmrError, MemoryError, torch.cuda.OutOfMemoryError) as e:
        if isinstance(e, SimmrError) and e.code != _abi.ENOMEM:
            raise
        pytest.skip("the memory cannot be had")
    counts = engine.fit_sam_counts()
    want, want_counts = _fit_sam.fit([case["text"]], 1, 7, 20)
    assert counts == want_counts
    _fit.assert_model(got, want, "more tiles than the index's grid")
    assert counts["taken_alignment"] == counts["records"] == case["taken"] and counts["header_lines"] > case["n_tiles"]


@pytest.mark.parametrize("k", [3, 8])
def test_taken_trips(engine, k):
    cus = n_cu()
    case = cases.taken_trips_text(cus)
    assert case["taken"] > 2 * cases.WG_RECS * cases.RECORD_WGS * cus and cases.batches(case["taken"]) > 3 * cases.WINDOWS_WGS * cus
    got = fit_sam(engine, [case["text"]], 2, k)
    counts = engine.fit_sam_counts()
    want = fit_repeated(case["text"], 2, k)  # (tests/test_fit_sam_host.py holds the multiplicity to the repetition)
    assert counts == want.c
    _fit.assert_model(got, want.model(20), f"taken trips, k {k}")
    assert counts["taken_alignment"] == case["taken"] and counts["lines"] == case["n_lines"] and got["n_positions"] == 298
    assert all(counts[n] == v for n, v in case["skips"].items())


@pytest.mark.parametrize("what", list(cases.MALFORMED))
def test_malformed_kinds(engine, what):
    info = _abi.FitInfo()
    trips = cases.record_trips_text(n_cu(), last=cases.MALFORMED[what])
    assert trips["text"].endswith(cases.MALFORMED[what]) and (trips["n_lines"] - 1) // cases.WG_RECS >= 3 * trips["grid"]  # its batch: a late trip
    for text in (cases.GOOD + cases.MALFORMED[what] + cases.GOOD, trips["text"]):
        engine.fit_reset(7, 20, 1 << 18)
        engine.fit_add_sam(text, 2)  # returns: the add only enqueues
        assert engine.lib.simmr_fit_plan(engine._h, C.byref(info)) == _abi.EINVAL and b"malformed" in engine.lib.simmr_last_error(engine._h)
        with pytest.raises(_fit_sam.Malformed):
            _fit_sam.fit([text], 2, 7, 20)
        engine.fit_add_sam(cases.GOOD, 2)  # sticky until the reset
        with pytest.raises(SimmrError) as ei:
            engine.fit_model()
        assert ei.value.code == _abi.EINVAL
    assert fit_sam(engine, [cases.GOOD], 2)["n_reads"] == 1


def test_split_invariance(engine):
    for what, text in (("the scan-chunk text", cases.scan_chunk_texts()[2]["text"]), ("the record-trips text", cases.record_trips_text(n_cu())["text"])):
        pieces = cases.cut(text)
        assert len(pieces) == 4 and not pieces[-1].endswith(b"\n")
        whole, whole_counts = against_restatement(engine, [text], 1, 7, what)
        parts = fit_sam(engine, pieces, 1)
        assert engine.fit_sam_counts() == whole_counts, what
        same_model(parts, whole, what + " in four adds")
