"""The coordinate-sorted BAM and its BAI index of the device (Engine.bam_sorted, Engine.bai; simmr_bam_sort_*, simmr_bai_* of
include/simmr_hip.h) against the plain-Python models: the records of tests/_bam.py stably sorted by (row, lo), the index of
tests/_bai.py byte for byte, and region queries through the device's own index against reading every record.  The columns are
hand-built (the passes read the columns, never the genome)."""
import gzip
import re
from pathlib import Path

import pytest

from simmr_amd import _abi
from simmr_amd.engine import Engine
from simmr_amd.sam import BGZF_EOF
from tests import _bai, _bai_cases, _bam
from tests._bai_cases import CONTIGS, MANY, MANY_CONTIGS, MANY_REFS, MANY_RNAMES, MANY_SLOT, REFS, RNAMES, SLOTS, WINDOW, columns
from tests.test_gpu_sam_seams import device_columns

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def _define(name, macro):
    return int(re.search(rf"^#define\s+{macro}\s+(\d+)u?\b", (CSRC / name).read_text(), re.M).group(1))


TILE = _define("sam_sort_kernels.hip", "SAMSORT_TILE")
CHUNK = _define("sam_kernels.hip", "SAM_CHUNK")
WG_READS = _define("sam_kernels.hip", "SAM_WG_READS")
WGS_PER_CU = _define("sam_kernels.hip", "SAM_WGS_PER_CU")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    for slot, lens in SLOTS.items():
        e.stage_synthetic(slot, lens, 10 + slot)
    e.stage_synthetic(MANY_SLOT, MANY, 99)
    yield e
    e.close()


def check(eng, specs, paired, what, layout=0, rnames=RNAMES, refs=REFS, contigs=CONTIGS, seed=3):
    """the file is header + the model's records in coordinate order, the index is the model's; returns (file, base, bai)"""
    o, t = columns(specs, seed=seed, contigs=contigs)
    reads, truth = device_columns(o, t, layout, eng.device)
    want, order = _bai_cases.sorted_records(o, t, paired, rnames)
    head = _bai_cases.header(refs)
    blocks, bai = eng.bam_sorted(reads, rnames, paired, truth)
    file_bytes = bytes(blocks.cpu().numpy()) + BGZF_EOF
    stream = gzip.decompress(file_bytes)
    assert stream[:len(head)] == head, what
    got = stream[len(head):]
    if got != want:
        i = next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} record bytes against {len(want)}; first difference at byte {i}")
    text, refs2, recs = _bam.parse_bam(stream)
    assert "SO:coordinate" in text.splitlines()[0] and refs2 == refs and len(recs) == len(specs), what
    assert b"".join(_bam.bgzf_blocks(file_bytes[:-len(BGZF_EOF)])) == stream, what
    got_bai = bytes(bai.cpu().numpy())
    want_bai = _bai.bai_bytes(len(refs), want, len(head))
    if got_bai != want_bai:
        i = next((k for k in range(min(len(got_bai), len(want_bai))) if got_bai[k] != want_bai[k]), min(len(got_bai), len(want_bai)))
        raise AssertionError(f"{what}: index of {len(got_bai)} bytes against {len(want_bai)}; first difference at byte {i}: "
                             f"{got_bai[i:i + 16].hex()} / {want_bai[i:i + 16].hex()}")
    return file_bytes, len(head), got_bai, order


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "unpaired"])
@pytest.mark.parametrize("layout", [0, 16], ids=["compact", "slot16"])
def test_mixed_lengths_strands_and_ties(eng, layout, paired):
    _, _, _, order = check(eng, _bai_cases.mixed_specs(), paired, f"mixed layout={layout} paired={paired}", layout=layout)
    assert order != sorted(order)
    assert eng.last_bam_sort_ms() > 0


def count_specs(n):
    """n reads of 0 to 3 bases scattered over every contig, far from read order; pairs share a contig"""
    return [((r // 2) % len(CONTIGS), (r * 7919) % 251, (r * 7 + r // CHUNK) % 4, (r >> 1 ^ r) & 1, r, [0] if (r * 7 + r // CHUNK) % 4 and r % 3 == 0 else [])
            for r in range(n)]


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, TILE + CHUNK + 3], ids=lambda n: f"{n}-reads")
def test_read_counts_where_the_passes_change_shape(eng, n):
    """the largest count is past a sort tile and past a scan chunk in the RECORDS.  The runs and the bins stay at five: every read
    lies below position 251, in the first window of its contig; test_reads_whose_runs_pass_a_chunk takes the runs past a chunk"""
    assert TILE + CHUNK + 3 > max(TILE, 2 * CHUNK)
    check(eng, count_specs(n), n % 2 == 0, f"{n} reads")


def spread_specs(n):
    """the reads of count_specs on contig 0 alone, two bases in front of the 67 window edges of its 1.1 Mbases, far from read order:
    on one position a read of three bases reaches over the edge (a bin one level up or more), the shorter ones stay in the leaf,
    and the stable order leaves them in read order — the bin changes with every second sorted read"""
    edges = (SLOTS[0][0] - 1) // WINDOW
    return [(0, (1 + (r * 7919) % edges) * WINDOW - 2, (r * 7 + r // CHUNK) % 4, (r >> 1 ^ r) & 1, r, [0] if (r * 7 + r // CHUNK) % 4 and r % 3 == 0 else [])
            for r in range(n)]


def test_reads_whose_runs_pass_a_chunk(eng):
    """Engine.bam_sorted past a sort tile and a scan chunk in the records AND past a scan chunk in the runs: the second round of
    k_bai_count / k_bai_scan / k_bai_compact takes more than one chunk of run keys"""
    n = TILE + CHUNK + 3
    assert n > max(TILE, 2 * CHUNK)
    _, _, bai, order = check(eng, spread_specs(n), False, f"{n} reads around the window edges")
    refs, _ = _bai.parse_bai(bai)
    chunks = [len(refs[0]["bins"][b]) for b in refs[0]["order"] if b != _bai.META_BIN]
    assert sum(chunks) > CHUNK and len(chunks) > (SLOTS[0][0] - 1) // WINDOW and len(refs[0]["ioffset"]) == 1 + (SLOTS[0][0] - 1) // WINDOW
    assert order != sorted(order) and all(not r["order"] for r in refs[1:])


def test_more_batches_of_reads_than_the_write_grid_has_workgroups(eng):
    """k_bamsort_write's batch loop: 16 reads a workgroup and trip, SAM_WGS_PER_CU workgroups per CU — a second trip for 17 reads"""
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    n = WG_READS * WGS_PER_CU * cus + 17
    assert -(-n // WG_READS) > WGS_PER_CU * cus
    specs = [((r // 2) % len(CONTIGS), (r * 7919) % 251, r % 3, (r >> 1 ^ r) & 1, r, []) for r in range(n)]
    check(eng, specs, False, f"{n} reads of 0 to 2 bases")


def test_a_names_set_whose_key_has_no_bits():
    """one contig without a base: pos_bits = row_bits = 0, nothing is sorted and place i holds read i (perm == nullptr in
    k_bamsort_gather and k_bamsort_write); every read is one without bases on position 0.  That the plan is on that path is
    asserted on what it decides from: the staged length of the one row it reports is 0, and the routine it asks for the key's
    widths (simmr_sam_sort_key_bits) answers no bit for one row of that length"""
    import ctypes as C
    e = Engine(0)
    try:
        e.stage_synthetic(0, [0], 5)
        specs = [(0, 0, 0, r & 1, 10 * r, []) for r in range(CHUNK + 37)]
        for paired in (False, True):
            _, _, bai, order = check(e, specs[:len(specs) - paired], paired, f"no key bits, paired={paired}", rnames=[(0, ["z"])], refs=[("z", 0)], contigs=[(0, 0)])
            assert order == list(range(len(specs) - paired))
            lens, n_rows, p, r = (C.c_uint64 * 4)(7, 7, 7, 7), C.c_uint64(7), C.c_uint32(7), C.c_uint32(7)
            assert e.lib.simmr_bam_sort_ref_lengths(e._bam_sort_handle(), lens, 4, C.byref(n_rows)) == 0 and (n_rows.value, lens[0]) == (1, 0)
            assert e.lib.simmr_sam_sort_key_bits(n_rows.value, lens[0], C.byref(p), C.byref(r)) == 0 and (p.value, r.value) == (0, 0)
            (ref0,), _ = _bai.parse_bai(bai)
            assert ref0["order"] == [4681, _bai.META_BIN] and len(ref0["bins"][4681]) == 1 and len(ref0["ioffset"]) == 1
    finally:
        e.close()


def test_every_read_on_one_position(eng):
    """one key: the stable sort keeps read order, one bin, one chunk, one window"""
    specs = [(4, 77, 1 + r % 3, r & 1, r, []) for r in range(600)]
    _, _, bai, order = check(eng, specs, True, "one position")
    assert order == list(range(600))
    refs, _ = _bai.parse_bai(bai)
    assert refs[4]["order"] == [4681, _bai.META_BIN] and len(refs[4]["bins"][4681]) == 1 and len(refs[4]["ioffset"]) == 1


def test_three_hundred_references_with_gaps(eng):
    """one read per reference, none on every third and none on the first and the last: empty references at both ends and between"""
    used = [c for c in range(1, 299) if c % 3]
    specs = _bai_cases.many_specs()
    _, _, bai, _ = check(eng, specs, False, "300 references", rnames=MANY_RNAMES, refs=MANY_REFS, contigs=MANY_CONTIGS)
    refs, _ = _bai.parse_bai(bai)
    assert [bool(r["order"]) for r in refs] == [c in used for c in range(300)]


def test_the_bin_levels_and_queries_through_the_device_index(eng):
    specs = _bai_cases.mixed_specs() + _bai_cases.level_specs()
    file_bytes, base, bai, _ = check(eng, specs, True, "levels")
    parsed, stream = _bai.parse_bai(bai), _bai.Stream(file_bytes)
    assert {9, 73, 585} <= set(parsed[0][0]["order"])
    found = 0
    for ref, beg, end in _bai_cases.edges():
        got = _bai.query(parsed, stream, ref, beg, end)
        assert got == _bai.brute(stream, base, ref, beg, end), (ref, beg, end)
        found += len(got)
    assert found >= len(specs)  # (not vacuous: the whole-reference queries alone return every record once)


def record_size(L, id_digits=1):
    """an unpaired record without edits: fixed fields, name, cigar, seq, qual, NM:C, MD:Z:<L>"""
    return 36 + id_digits + 1 + (4 if L else 0) + (L + 1) // 2 + L + 4 + 3 + len(str(L)) + 1


@pytest.mark.parametrize("target", [65280 - 1, 65280, 65280 + 1, 2 * 65280], ids=lambda t: f"{t}-bytes")
def test_streams_that_end_at_a_block_edge(eng, target):
    """header + records of exactly `target` bytes: fillers of 100 bases and two reads whose lengths make up the rest"""
    head = len(_bai_cases.header())
    filler = record_size(100)
    k = (target - head) // filler - 3
    rest = target - head - k * filler
    la, lb = next((a, b) for a in range(1, 600) for b in range(1, 600) if record_size(a) + record_size(b) == rest)
    lengths = [100] * k + [la, lb]
    specs = [(0, 900_000 - 1000 * i, L, i & 1, 7, []) for i, L in enumerate(lengths)]
    o, t = columns(specs, seed=3)
    want, _ = _bai_cases.sorted_records(o, t, False)
    assert head + len(want) == target == head + sum(record_size(L) for L in lengths)
    file_bytes, _, bai, _ = check(eng, specs, False, f"{target} bytes")
    payloads = _bam.bgzf_blocks(file_bytes[:-len(BGZF_EOF)])
    assert [len(p) for p in payloads] == [65280] * (target // 65280) + ([target % 65280] if target % 65280 else [])
    (first, last), _ = _bai.parse_bai(bai)[0][0]["bins"][_bai.META_BIN]
    assert last == _bai.voff(target) and _bai.Stream(file_bytes).upos(last) == target  # (at a block edge: the EOF block's start)


def test_an_index_of_columns_the_caller_holds(eng):
    import torch
    dev = eng.device
    r0, r1 = _bai_cases.plain(1, 3, 7), _bai_cases.plain(1, 5, 5)
    up, down = [(1 << 40) | 3, (1 << 40) | 5], [(1 << 40) | 5, (1 << 40) | 3]
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    end = torch.tensor([10, 10], dtype=torch.int32, device=dev)
    rec_off = i64([0, len(r0), len(r0) + len(r1)])
    with pytest.raises(_abi.SimmrError) as err:
        eng.bai(i64(down), end, rec_off, 2, 100)
    assert err.value.code == _abi.EINVAL
    with pytest.raises(_abi.SimmrError) as err:  # offsets that decrease
        eng.bai(i64(up), end, i64([0, 40, 39]), 2, 100)
    assert err.value.code == _abi.EINVAL
    with pytest.raises(_abi.SimmrError) as err:  # a reference that n_ref does not cover
        eng.bai(i64(up), end, rec_off, 1, 100)
    assert err.value.code == _abi.EINVAL
    with pytest.raises(_abi.SimmrError) as err:  # a contig of 2^29 bases: only the length is needed, nothing that large is staged
        eng.bai(i64(up), end, rec_off, 2, 100, ref_len=[1000, 1 << 29])
    assert err.value.code == _abi.ERANGE
    got = bytes(eng.bai(i64(up), end, rec_off, 2, 100, ref_len=[1000, (1 << 29) - 1]).cpu().numpy())
    assert got == _bai.bai_bytes(2, r0 + r1, 100)
