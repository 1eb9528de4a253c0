"""The BAI index of the device (Engine.bai; simmr_bai_plan / simmr_bai_emit, bam_index_kernels.hip) past the first tile, chunk and
grid trip of its kernels, byte for byte against tests/_seams.py:bai_from_columns, which tests/test_seams_host.py holds to the plain
index of tests/_bai.py.  The columns are hand-made on the device (Engine.bai takes the caller's own: no genome, no reads, no record
bytes; a reference of 2^29 - 1 bases costs four bytes); the offsets are those of tests/_bai_cases.py:plain records.

Which loop each test is the first to enter:
  test_the_bin_changes_at_every_record
      samsort_sort_pairs over the RUNS with more than one tile of SAMSORT_TILE pairs; the second round of k_bai_count / k_bai_scan /
      k_bai_compact (over the sorted run keys) with more than one chunk of SAM_CHUNK runs, and k_bai_compact's prefix[chunk] on the
      record side with every record a run; k_bai_write_chunks' search over more than SAM_CHUNK bins; a bin with more than SAM_CHUNK
      chunks, interleaved in file order with another bin's (the stability of the run sort);
  test_ties_on_one_position
      equal keys next to each other (k_bai_check lets them pass) whose bins alternate: every record a run, two bins of k / 2 chunks,
      at k around SAM_CHUNK and past SAMSORT_TILE;
  test_the_linear_index_past_its_first_tile
      k_bai_write_refs: the loop over tiles of 256 windows and its carry (the lds[0] / lds[1] hand-off), with a first tile without a
      record, tiles with a record in lane 255 alone and in lane 0 alone, two tiles without any in the middle, a partial last tile
      and a last tile of one window; k_bai_windows: one thread that walks 32 768 windows;
  test_grid_strides_of_records_runs_and_references
      the second trip of k_bai_windows and of k_bai_write_chunks (more than 256 x 32 x CUs records and runs), the second and third
      trip of k_bai_write_refs (more than 2 x 8 x CUs references), k_bai_layout's third and later tiles of 256 references,
      sam_scan_chunks through k_bai_scan past 256 chunk sums for the records and for the runs, and k_bai_check's chunks that hold
      more than one reference;
  test_more_references_than_the_reference_grid_has_threads
      the second trip of k_bai_refs (more than 256 x 32 x CUs references);
  test_virtual_offsets_around_2_to_the_32_and_up_to_48_bits
      bai_voff where the block's file offset passes 2^32, and the plan's limit on both sides;
  test_nothing_and_next_to_nothing
      no record on 0, 1 and 257 references, one record of one base, and a record that ends beyond 2^29."""
import re
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from simmr_amd.engine import Engine
from tests import _bai, _bai_cases, _seams
from tests._bai_cases import WINDOW, index_shape

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def _define(name, macro):
    return int(re.search(rf"^#define\s+{macro}\s+(\d+)u?\b", (CSRC / name).read_text(), re.M).group(1))


TILE = int(re.search(r"SAMSORT_PAIRS_TILE = (\d+)", (CSRC / "engine_internal.hpp").read_text()).group(1))
CHUNK = _define("sam_kernels.hip", "SAM_CHUNK")
SCAN = 256        # chunk sums a pass of sam_scan_chunks takes, windows and references a tile takes: the workgroup's threads
ITEM_WGS = 32     # workgroups per CU of k_bai_windows, k_bai_write_chunks and k_bai_refs (a thread per item)
REF_WGS = 8       # workgroups per CU of k_bai_write_refs (a workgroup per reference)
BASE = 3 * 65280 - 100  # the bytes in front of record 0: a few records in front of a block edge


def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def same_bytes(got, want, what):
    g, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    if g.size != w.size or not np.array_equal(g, w):
        m = min(g.size, w.size)
        d = np.flatnonzero(g[:m] != w[:m])
        i = int(d[0]) if d.size else m
        raise AssertionError(f"{what}: index of {g.size} bytes against {w.size}; first difference at byte {i}: "
                             f"{got[i:i + 16].hex()} / {want[i:i + 16].hex()}")


def device_index(eng, n_ref, ref, lo, end, rec_off, base, ref_len=None):
    import torch
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64).astype(dt))).to(eng.device)
    key = (np.asarray(ref, dtype=np.int64) << 40) | np.asarray(lo, dtype=np.int64)
    return bytes(eng.bai(to(key, np.int64), to(end, np.int32), to(rec_off, np.int64), n_ref, base, ref_len=ref_len).cpu().numpy())


def check_shape(eng, shape, what, base=BASE):
    """the device's index of the shape's columns equals the model's; returns (the model's counts, its bytes)"""
    ref, lo, end = shape["ref"], shape["lo"], shape["end"]
    rec_off = _bai_cases.plain_offsets(lo, end)
    counts = {}
    want = _seams.bai_from_columns(shape["n_ref"], ref, lo, end, rec_off, base, counts)
    same_bytes(device_index(eng, shape["n_ref"], ref, lo, end, rec_off, base, shape["ref_len"]), want, what)
    return counts, want


def real_bins(parsed_ref):
    return [(b, parsed_ref["bins"][b]) for b in parsed_ref["order"] if b != _bai.META_BIN]


@pytest.mark.parametrize("n_ref", [1, 3], ids=["one-reference", "three-references"])
def test_the_bin_changes_at_every_record(eng, n_ref):
    """the run sort past a tile, the run-side count / scan / compact past a chunk, more than SAM_CHUNK bins, a bin of more than
    SAM_CHUNK chunks; over three references (row, bin) order differs from file order across references too"""
    shape = index_shape("bin_changes", m=CHUNK + 76, big=CHUNK + 1, n_ref=n_ref)
    counts, want = check_shape(eng, shape, f"bin changes on {n_ref} reference(s)")
    refs, _ = _bai.parse_bai(want)
    bins = [bc for r in refs for bc in real_bins(r)]
    n_runs = sum(len(c) for _, c in bins)
    assert n_runs == shape["ref"].size == counts["n_runs"] and n_runs > TILE + CHUNK
    assert len(bins) == counts["n_bins"] and len(bins) > CHUNK
    assert max(len(c) for _, c in bins) > CHUNK and len(refs[n_ref - 1]["bins"][0]) > CHUNK  # (bin 0 of the last reference)
    assert all({int(l) for l in _seams.bin_level([b for b, _ in real_bins(r)])} == {0, 1, 2, 3, 4, 5} for r in refs)
    # a bin's chunks are in file order although another bin's lie between any two of them
    assert all(x[1] < y[0] for _, c in bins for x, y in zip(c, c[1:]))


@pytest.mark.parametrize("k", [2, CHUNK - 1, CHUNK, CHUNK + 1, TILE + 1], ids=lambda k: f"{k}-records")
def test_ties_on_one_position(eng, k):
    """k equal keys, intervals of 1 and of 16385 bases in turn: every record is a run of its own, two bins of k / 2 chunks"""
    shape = index_shape("ties", k=k)
    assert np.unique((shape["ref"] << 40) | shape["lo"]).size == 1
    counts, want = check_shape(eng, shape, f"{k} ties")
    (ref0,), _ = _bai.parse_bai(want)
    bins = real_bins(ref0)
    assert counts["n_runs"] == k and sorted(len(c) for _, c in bins) == [k // 2, (k + 1) // 2] and len(ref0["ioffset"]) == 7
    assert sorted(int(l) for l in _seams.bin_level([b for b, _ in bins])) == [4, 5]


def test_the_linear_index_past_its_first_tile(eng):
    """k_bai_write_refs' tile loop and carry on references of 255, 256, 257, 512, 513 and 32768 windows (the last one's last record
    ends at 2^29 exactly), and a record over all 32768 windows of another reference with shorter ones inside it"""
    n_intvs = (255, 256, 257, 512, 513, 32768)
    shape = index_shape("linear", n_intvs=n_intvs, long=32768)
    assert int(shape["end"].max()) == 1 << 29 and max(shape["ref_len"]) == (1 << 29) - 1
    counts, want = check_shape(eng, shape, "linear index")
    refs, _ = _bai.parse_bai(want)
    assert [len(r["ioffset"]) for r in refs] == list(n_intvs) + [0, 32768] == counts["n_intv"].tolist()
    assert any(n > SCAN and n % SCAN == 0 for n in n_intvs) and any(n % SCAN == 1 for n in n_intvs) and any(n % SCAN == SCAN - 1 for n in n_intvs)
    io = refs[5]["ioffset"]
    tiles = [io[t * SCAN:(t + 1) * SCAN] for t in range(32768 // SCAN)]
    changes = [[w for w in range(SCAN) if (tile[w] != tile[w - 1] if w else tile[0] != (tiles[t - 1][-1] if t else 0))] for t, tile in enumerate(tiles)]
    assert tiles[0] == [0] * SCAN                                  # the first tile has no record: the front shows 0
    assert changes[1] == [SCAN - 1] and changes[2] == [0]          # a record in lane 255 alone, then one in lane 0 alone
    assert changes[3] == [] and changes[4] == [] and changes[5]    # two tiles without any in the middle show the carry
    assert changes[-1] == [SCAN - 1] and io == sorted(io)          # the last window is filled
    for k in range(5):  # the shorter references: a filled last window behind a stretch without records
        assert refs[k]["ioffset"][-1] != refs[k]["ioffset"][-2] and refs[k]["ioffset"][:3] == [0, 0, 0]
    long_io = refs[7]["ioffset"]
    first = int(np.flatnonzero(shape["ref"] == 7)[0])
    assert int((shape["ref"] == 7).sum()) > 3 and set(long_io) == {_bai.voff(BASE + int(_bai_cases.plain_offsets(shape["lo"], shape["end"])[first]))}


def test_grid_strides_of_records_runs_and_references(eng):
    """more records and runs than 256 x 32 x CUs, more references than 2 x 8 x CUs, chunks that hold several references"""
    cus = n_cu()
    n_ref, n = 2 * REF_WGS * cus + 5, SCAN * ITEM_WGS * cus + 300
    shape = index_shape("strides", n_ref=n_ref, n=n)
    ref = shape["ref"]
    counts, want = check_shape(eng, shape, f"{n} records on {n_ref} references")
    assert ref.size == n and counts["n_runs"] == n > SCAN * ITEM_WGS * cus            # a second trip of k_bai_windows and k_bai_write_chunks
    assert n_ref > 2 * REF_WGS * cus and -(-n_ref // SCAN) >= 3                       # a third trip of k_bai_write_refs, a third tile of k_bai_layout
    assert -(-n // CHUNK) > SCAN and -(-counts["n_runs"] // CHUNK) > SCAN             # k_bai_scan past 256 chunk sums, twice
    firsts = np.arange(0, n, CHUNK)
    mixed = np.flatnonzero(ref[firsts] != ref[np.minimum(firsts + CHUNK, n) - 1])
    assert mixed.size > SCAN and mixed[-1] > 0                                        # k_bai_check's atomic per record: chunks of several references all along
    with_records = counts["n_intv"] > 0
    assert with_records.tolist() == [c % 3 != 0 and 0 < c < n_ref - 1 for c in range(n_ref)]
    assert counts["n_bins"] > CHUNK and len(want) > 16 * n


def test_more_references_than_the_reference_grid_has_threads(eng):
    """k_bai_refs' second trip: records on the first reference, on one in the middle and on the last of 256 x 32 x CUs + 1"""
    cus = n_cu()
    n_ref = SCAN * ITEM_WGS * cus + 1
    shape = index_shape("sparse_refs", n_ref=n_ref)
    assert n_ref + 1 > SCAN * ITEM_WGS * cus and sorted(set(shape["ref"].tolist())) == [0, n_ref // 2, n_ref - 1]
    counts, want = check_shape(eng, shape, f"{n_ref} references")
    assert np.flatnonzero(counts["n_intv"]).tolist() == [0, n_ref // 2, n_ref - 1] and len(want) > 8 * n_ref


def test_virtual_offsets_around_2_to_the_32_and_up_to_48_bits(eng):
    """A block's offset in the file is 65311 x its number: it passes 2^32 between two records here.  The plan takes a stream as
    long as the offset behind the block that holds its end, (bytes / 65280 + 1) x 65311, stays below 2^48 (the 48 bits of
    simmr_bai_plan's contract): the largest `base` on this side is taken, the next one and one beyond 2^62 are SIMMR_ERANGE."""
    r0, r1 = _bai_cases.plain(1, 3, 7), _bai_cases.plain(1, 5, 5)
    rec_off = [0, len(r0), len(r0) + len(r1)]
    index = lambda base: device_index(eng, 2, [1, 1], [3, 5], [10, 10], rec_off, base)
    edge = -(-2**32 // 65311)  # the first block whose offset in the file is 2^32 or more
    base = edge * 65280 - 20
    below, above = _bai.voff(base + rec_off[0]) >> 16, _bai.voff(base + rec_off[1]) >> 16
    assert below == (edge - 1) * 65311 < 2**32 < edge * 65311 == above and above - 2**32 < 65311
    largest = (2**48 - 1) // 65311 * 65280 - 1 - rec_off[2]
    refused = lambda b: ((b + rec_off[2]) // 65280 + 1) * 65311 >= 2**48
    assert not refused(largest) and refused(largest + 1) and largest < 2**62
    for b in (base, largest):
        want = _bai.bai_bytes(2, r0 + r1, b)
        assert want == _seams.bai_from_columns(2, [1, 1], [3, 5], [10, 10], rec_off, b)
        same_bytes(index(b), want, f"base {b}")
        (first, last), _ = _bai.parse_bai(want)[0][1]["bins"][_bai.META_BIN]
        assert (first, last) == (_bai.voff(b), _bai.voff(b + rec_off[2]))
    for b in (largest + 1, 2**62 + 1):
        with pytest.raises(_abi.SimmrError) as err:
            index(b)
        assert err.value.code == _abi.ERANGE, b


def test_nothing_and_next_to_nothing(eng):
    for n_ref in (0, 1, 257):
        want = _seams.bai_from_columns(n_ref, [], [], [], [0], 100)
        assert want == b"BAI\1" + n_ref.to_bytes(4, "little") + bytes(8 * n_ref + 8) == _bai.bai_bytes(n_ref, b"", 100)
        same_bytes(device_index(eng, n_ref, [], [], [], [0], 100), want, f"no record, {n_ref} references")
    one = _bai_cases.plain(0, 0, 1)
    want = _bai.bai_bytes(1, one, 100)
    assert want == _seams.bai_from_columns(1, [0], [0], [1], [0, len(one)], 100)
    same_bytes(device_index(eng, 1, [0], [0], [1], [0, len(one)], 100), want, "one record of one base")
    with pytest.raises(_abi.SimmrError) as err:  # a record that ends one base beyond what the six levels cover
        device_index(eng, 1, [0], [(1 << 29) - WINDOW], [(1 << 29) + 1], [0, 40], 100)
    assert err.value.code == _abi.ERANGE
