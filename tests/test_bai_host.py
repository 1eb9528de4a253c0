"""CPU-only checks of the sorted BAM and its BAI index: the plain-Python index (tests/_bai.py) written by hand once, its writer
against its separately written reader on region queries, the invariants of the format, the new symbols and the build."""
import gzip
import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _bai, _bai_cases, _bam

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "simmr_amd" / "csrc"
NAMES = ("simmr_bam_sort_create", "simmr_bam_sort_plan", "simmr_bam_sort_emit", "simmr_last_bam_sort_ms", "simmr_bam_sort_ref_lengths",
         "simmr_bai_plan", "simmr_bai_emit")


def plain_record(ref_id, pos, L):
    """a record without tags: 57 bytes for L == 10"""
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, 2, 255, _bam.reg2bin(pos, pos + max(L, 1)), 1, 0, L, -1, -1, 0) + b"a\0" + \
        struct.pack("<I", L << 4) + bytes([0x11] * ((L + 1) // 2)) + bytes([30] * L)
    return struct.pack("<i", len(body)) + body


def test_an_index_written_by_hand():
    """two references, the first empty; two records in one leaf bin and one across position 16384; the second record lies
    across the first block's end"""
    recs = plain_record(1, 100, 10) + plain_record(1, 200, 10) + plain_record(1, 16380, 10)
    assert len(recs) == 3 * 57
    base = 65280 - 57 - 20
    a, b, c, e = base, base + 57, base + 114, base + 171
    assert b < 65280 < c
    vc, ve = (65311 << 16) | (c - 65280), (65311 << 16) | (e - 65280)
    want = b"BAI\1" + struct.pack("<i", 2)
    want += struct.pack("<ii", 0, 0)                                    # reference 0: no bin, no window
    want += struct.pack("<i", 3)                                        # reference 1: two bins and the metadata bin
    want += struct.pack("<IiQQ", 585, 1, vc, ve)                        #   the record across 16384, one level up
    want += struct.pack("<IiQQ", 4681, 1, a, vc)                        #   the two records of the first leaf, one chunk
    want += struct.pack("<IiQQQQ", 37450, 2, a, ve, 3, 0)
    want += struct.pack("<iQQ", 2, a, vc)                               #   windows 0 and 1
    want += struct.pack("<Q", 0)
    assert _bai.bai_bytes(2, recs, base) == want
    refs, n_no_coor = _bai.parse_bai(want)
    assert n_no_coor == 0 and refs[0] == {"bins": {}, "order": [], "ioffset": []} and refs[1]["order"] == [585, 4681, 37450]


def test_virtual_offsets_at_the_block_edges():
    assert [_bai.voff(p) for p in (0, 65279, 65280, 65281, 2 * 65280)] == [0, 65279, 65311 << 16, (65311 << 16) | 1, (2 * 65311) << 16]
    data = bytes(range(251)) * 600
    stream = _bai.Stream(_bam.bgzf_frame(data) + _bam.BGZF_EOF)
    for p in (0, 1, 65279, 65280, 65281, 2 * 65280 - 1, 2 * 65280, len(data) - 1, len(data)):
        assert stream.upos(_bai.voff(p)) == p


@pytest.fixture(scope="module", params=[True, False], ids=["paired", "unpaired"])
def indexed(request):
    o, t = _bai_cases.columns(_bai_cases.mixed_specs() + _bai_cases.level_specs(), seed=31)
    records, order = _bai_cases.sorted_records(o, t, request.param)
    file_bytes, base = _bai_cases.file_of(records)
    return records, order, file_bytes, base, _bai.bai_bytes(len(_bai_cases.REFS), records, base)


def test_the_file_is_a_bam_in_coordinate_order(indexed):
    records, order, file_bytes, base, _ = indexed
    text, refs, recs = _bam.parse_bam(gzip.decompress(file_bytes))
    assert "SO:coordinate" in text.splitlines()[0] and refs == _bai_cases.REFS and len(recs) == len(order)
    keys = [(r["ref_id"], r["pos"]) for r in recs]
    assert keys == sorted(keys) and len(set(keys)) < len(keys)


def test_queries_through_the_index_find_what_reading_everything_finds(indexed):
    records, _, file_bytes, base, bai = indexed
    stream, parsed = _bai.Stream(file_bytes), _bai.parse_bai(bai)
    rng = np.random.default_rng(17)
    queries = _bai_cases.edges()
    for _ in range(200):
        ref = int(rng.integers(0, len(_bai_cases.REFS)))
        length = _bai_cases.REFS[ref][1]
        beg = int(rng.integers(0, length))
        queries.append((ref, beg, beg + 1 + int(rng.integers(0, min(length, 70_000)))))
    found = 0
    for ref, beg, end in queries:
        got = _bai.query(parsed, stream, ref, beg, end)
        assert got == _bai.brute(stream, base, ref, beg, end), (ref, beg, end)
        found += len(got)
    assert found >= len(_bam.parse_records(records))  # (not vacuous: the whole-reference queries alone return every record once)


def test_invariants_of_the_index(indexed):
    records, _, file_bytes, base, bai = indexed
    refs, n_no_coor = _bai.parse_bai(bai)
    cols, total = _bai.record_columns(records)
    recs = _bam.parse_records(records)
    assert n_no_coor == 0 and len(refs) == len(_bai_cases.REFS)
    n_mapped = 0
    for ref, idx in enumerate(refs):
        mine = [i for i, c in enumerate(cols) if c[0] == ref]
        if not mine:
            assert idx["order"] == [] and idx["ioffset"] == []
            continue
        assert idx["order"][-1] == _bai.META_BIN and idx["order"][:-1] == sorted(idx["order"][:-1])
        (first, last), (mapped, unmapped) = idx["bins"][_bai.META_BIN]
        assert (first, last, mapped, unmapped) == (_bai.voff(base + cols[mine[0]][3]), _bai.voff(base + (cols[mine[-1] + 1][3] if mine[-1] + 1 < len(cols) else total)), len(mine), 0)
        n_mapped += mapped
        assert idx["ioffset"] == sorted(idx["ioffset"]) and len(idx["ioffset"]) == 1 + ((max(cols[i][2] for i in mine) - 1) >> 14)
        for b in idx["order"][:-1]:
            chunks = idx["bins"][b]
            assert all(c0 < c1 for c0, c1 in chunks) and all(x[1] <= y[0] for x, y in zip(chunks, chunks[1:])), (ref, b)
        for i in mine:  # exactly one chunk of the bin the record itself names holds its start
            v = _bai.voff(base + cols[i][3])
            holders = [(b, c) for b in idx["order"][:-1] for c in idx["bins"][b] if c[0] <= v < c[1]]
            assert len(holders) == 1 and holders[0][0] == recs[i]["bin"], (ref, i, holders)
    assert n_mapped == len(cols)
    bins = {b for idx in refs for b in idx["order"]}
    assert {9, 73, 585} <= bins and any(4681 <= b < _bai.META_BIN for b in bins)  # the straddlers of 2^20, 2^17 and 2^14, and leaves


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, re.M) and name in _abi.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"^void simmr_bam_sort_destroy\(", header, re.M) and "simmr_bam_sort_destroy" in _abi.SYMBOLS
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)]).decode()
    for name in NAMES + ("simmr_bam_sort_destroy", "k_bamsort_write", "k_bai_write_refs"):
        assert name in dyn, name
    assert "samsort_sort_pairs" not in dyn and "SIMMR_ABI_VERSION 1" in header


def test_the_unit_is_built_without_a_slot_of_the_engine():
    make = (CSRC / "Makefile").read_text()
    assert make.count(" bam_index.hip bam.hip fit_sam.hip fit.hip overlap.hip sam_sort.hip sam.hip pileup.hip engine.hip depth.hip strain.hip regions.hip\n") == 2
    srcs = re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
    assert {"bam_index.hip", "bam_index_kernels.hip"} <= set(srcs)
    internal = (CSRC / "engine_internal.hpp").read_text()
    assert "ENG_EXT_BAM = 9," in internal and "ENG_EXT_COUNT = 12" in internal
    unit = (CSRC / "bam_index.hip").read_text()
    assert "eng_ext_slot" not in unit and '#include "engine.hip"' not in unit and '#include "kernels.hip"' not in unit
    k = (CSRC / "bam_index_kernels.hip").read_text()
    assert "#define BAM_ROUTINES_ONLY" in k and "samsort_sort_pairs" in unit
    # the sorted unit sizes and writes through the record policy of the unsorted unit and carries no record routine of its own:
    # BamRec is bam_record<false> and bam_record<true>, and bam_record is defined once in the library
    code = re.sub(r"//.*", "", k)
    assert "rec_size_keyed<BamRec, true>" in code and "rec_write_places<BamRec, true>" in code and "bam_record" not in code
    bk = (CSRC / "bam_kernels.hip").read_text()
    policy = bk.split("struct BamRec {")[1].split("};")[0]
    assert bk.count("struct BamRec {") == 1 and "bam_record<false>" in policy and "bam_record<true>" in policy
    assert sum(len(re.findall(r"^SIMMR_DEV uint32_t bam_record\(", f.read_text(), re.M)) for f in CSRC.iterdir() if f.suffix in (".hip", ".hpp")) == 1
    assert "#ifndef BAM_ROUTINES_ONLY" in bk


@pytest.fixture(scope="module")
def host_exe():
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "simmr_amd" / "host")])
    return str(ROOT / "simmr_amd" / "host" / "simmr-hip")


USAGE_ROWS = [
    (["--genome", "a.fna", "--output", "x.fq", "--bam-sorted"], 2, "error: --bam-sorted needs --bam"),
    (["--genome", "a.fna", "--output", "x.fq", "--bam", "x.bam", "--bam-index", "x.idx"], 2, "error: --bam-index needs --bam-sorted"),
    (["--genome", "a.fna", "--output", "x.fq", "--bam", "x.bam", "--bam-sorted", "--bam-index"], 2, "error: a value is required for '--bam-index'"),
    # refused exactly as --bam is: that refusal comes first
    (["--genome", "a.fna", "--output", "x.fq", "--bam", "x.bam", "--bam-sorted", "--devices", "0,1"], 1,
     "ERROR simmr-hip: --bam does not combine with --devices: use --device"),
]


@pytest.mark.parametrize("argv,status,line", USAGE_ROWS, ids=[" ".join(r[0]) for r in USAGE_ROWS])
def test_cli_usage_rows(host_exe, argv, status, line):
    r = subprocess.run([host_exe] + argv, capture_output=True, text=True)
    assert r.returncode == status and r.stderr.splitlines()[0] == line, r.stderr


def test_help_describes_the_flag(host_exe):
    helptext = subprocess.check_output([host_exe, "--help"]).decode()
    row = helptext.split("--bam-sorted")[1].split("--overlaps <FILE>")[0]
    assert helptext.index("--bam <FILE>") < helptext.index("--bam-sorted") < helptext.index("--overlaps <FILE>")
    for needle in ("coordinate order", ".bai", "beside", "not compressed", "2^29", "not with --devices", "--bam-index"):
        assert needle in row, needle


def test_a_contig_of_two_to_the_29_ends_the_run_before_any_device_work(host_exe, tmp_path):
    """the bytes of the body are what counts: a sparse file stands for 2^29 of them"""
    big = tmp_path / "big.fna"
    with open(big, "wb") as f:
        f.write(b">small\nACGT\n>big one\n")
        f.seek((1 << 29) - 1, 1)
        f.write(b"A\n")
    r = subprocess.run([host_exe, "--genome", str(big), "--output", str(tmp_path / "x.fq"), "--bam", str(tmp_path / "x.bam"), "--bam-sorted"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.splitlines() == [
        f"ERROR simmr-hip: --bam-sorted: sequence 'big one' of {big} has 2^29 bases or more: a BAI index does not reach there (CSI is not written)"]
    assert not (tmp_path / "x.bam").exists() and not (tmp_path / "x.bam.bai").exists() and not (tmp_path / "x.fq").exists()


def test_the_framing_pieces_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """BgzfPieces of simmr_host.hpp, which carries what does not fill a piece into the next: every piece but the last is a whole
    number of blocks, the pieces laid end to end are the input, for appends of every kind of size"""
    exe = tmp_path / "bgzf_pieces_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "bgzf_pieces_main.cpp")])
    cases = [(1, [1]), (1, [65279, 1]), (1, [65280]), (1, [65281]), (2, [65280] * 5), (2, [1, 130559, 1, 65280 * 3 + 7]), (3, [100_000] * 9),
             (1, []), (4, [0, 0, 5]), (2, [65280 * 2] * 3), (1024, [300_000, 7])]
    text = f"{len(cases)}\n" + "".join(f"{blocks} {len(sizes)} {' '.join(map(str, sizes))}\n" for blocks, sizes in cases)
    r = subprocess.run([str(exe)], input=text.encode(), capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    rows = [list(map(int, l.split())) for l in r.stdout.decode().splitlines()]
    assert len(rows) == len(cases)
    for (blocks, sizes), got in zip(cases, rows):
        total, piece = sum(sizes), blocks * 65280
        assert got == [piece] * (total // piece) + ([total % piece] if total % piece else []), (blocks, sizes, got)


def test_calls_need_a_handle():
    import ctypes as C
    lib = _abi.load()
    total, ms, h = C.c_uint64(), C.c_float(), C.c_void_p()
    names, reads, truth = _abi.SamNames(0, None, None, None), _abi.ReadsOut(), _abi.TruthOut()
    assert lib.simmr_bam_sort_create(None, C.byref(h)) == _abi.EINVAL
    assert lib.simmr_bam_sort_plan(None, C.byref(names), C.byref(reads), C.byref(truth), 0, 0, C.byref(total)) == _abi.EINVAL
    assert lib.simmr_bam_sort_emit(None, C.byref(reads), C.byref(truth), None, 0, None, None, None) == _abi.EINVAL
    assert lib.simmr_last_bam_sort_ms(None, C.byref(ms)) == _abi.EINVAL
    assert lib.simmr_bai_plan(None, None, None, None, 0, 0, None, 0, C.byref(total)) == _abi.EINVAL
    assert lib.simmr_bai_emit(None, None, 0) == _abi.EINVAL
    lib.simmr_bam_sort_destroy(None)
