"""CPU-only checks of the sorted-SAM surface: the symbols, the key widths and their limits, the header writers, the command
line's rows, and the host's merge of sorted runs — through libsimmr_host.so, and once more in a stand-alone program built with
the address and undefined-behaviour sanitizers."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from simmr_amd.sam import sam_header
from tests import _sam_sort

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"
NAMES = ("simmr_sam_sort_plan", "simmr_sam_sort_emit", "simmr_last_sam_sort_ms", "simmr_sam_sort_key_bits")


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, re.M) and name in _abi.SYMBOLS and hasattr(lib, name), name
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)]).decode()
    assert "simmr_sam_sort_emit" in dyn and "k_samsort_scatter" in dyn and "eng_ext_slot" not in dyn
    assert "row << 40" in header and "SIMMR_ERANGE" in header.split("simmr_sam_sort_key_bits")[0].split("coordinate order")[-1]


def test_calls_need_an_engine():
    lib = _abi.load()
    ms, total = C.c_float(), C.c_uint64()
    names, reads, truth = _abi.SamNames(0, None, None, None), _abi.ReadsOut(), _abi.TruthOut()
    assert lib.simmr_sam_sort_plan(None, C.byref(names), C.byref(reads), C.byref(truth), 0, 0, C.byref(total)) == _abi.EINVAL
    assert lib.simmr_sam_sort_emit(None, C.byref(reads), C.byref(truth), None, 0, None, None) == _abi.EINVAL
    assert lib.simmr_last_sam_sort_ms(None, C.byref(ms)) == _abi.EINVAL


def test_key_widths_and_limits():
    """the counterfeit names sets: more rows and longer contigs than can be staged"""
    lib = _abi.load()
    p, r = C.c_uint32(), C.c_uint32()
    for rows, longest, want in ((1, 4_641_652, (23, 0)), (0, 0, (0, 0)), (1, 0, (0, 0)), (2, 1, (1, 1)), (300, 255, (8, 9)), (256, 256, (9, 8)),
                                (257, 2**32 + 4096, (33, 9)), (2**24, 2**40 - 1, (40, 24))):
        assert lib.simmr_sam_sort_key_bits(rows, longest, C.byref(p), C.byref(r)) == 0 and (p.value, r.value) == want, (rows, longest)
    assert lib.simmr_sam_sort_key_bits(2**24 + 1, 10, C.byref(p), C.byref(r)) == _abi.ERANGE
    assert lib.simmr_sam_sort_key_bits(1, 2**40, C.byref(p), C.byref(r)) == _abi.ERANGE
    assert lib.simmr_sam_sort_key_bits(1, 2**40 - 1, None, None) == 0


def test_kernel_constants():
    k = (ROOT / "simmr_amd" / "csrc" / "sam_sort_kernels.hip").read_text()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(SAMSORT_\w+)\s+(\d+)u?\b", k, re.M)}
    assert d["SAMSORT_TILE"] == 4 * 64 * d["SAMSORT_ROUNDS"] and d["SAMSORT_DIGIT_BITS"] == 8 and d["SAMSORT_KEY_POS_BITS"] == 40


def test_model_orders_by_row_then_lo_then_read():
    o = {"start": np.array([9, 5, 5, 0, 7], np.uint64), "end": np.array([3, 8, 5, 2, 7], np.uint64),
         "genome": np.array([0, 0, 0, 2, 0], np.uint32), "contig": np.array([1, 1, 1, 0, 0], np.uint32)}
    rn = [(2, ["x"]), (0, ["a", "b"])]
    perm, key = _sam_sort.order(o, rn)
    assert key == [(2 << 40) | 3, (2 << 40) | 5, (2 << 40) | 5, 0, (1 << 40) | 7] and perm == [3, 4, 0, 1, 2]


def test_header_writer():
    assert sam_header(["chr1"], [10], sort_order="coordinate") == "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:10\n@PG\tID:simmr-hip\tPN:simmr-hip\n"
    assert sam_header(["chr1"], [10]) == sam_header(["chr1"], [10], "unsorted") == sam_header(["chr1"], [10], "coordinate").replace("coordinate", "unsorted")
    with pytest.raises(ValueError):
        sam_header(["chr1"], [10], sort_order="queryname")


@pytest.fixture(scope="module")
def host_lib():
    subprocess.check_call(["make", "-s", "-C", str(HOST)])
    lib = C.CDLL(str(HOST / "libsimmr_host.so"))
    lib.simmr_host_sam_header_sorted.restype = C.c_void_p
    lib.simmr_host_sam_header_sorted.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p]
    lib.simmr_host_sam_merge.restype = C.c_int64
    lib.simmr_host_sam_merge.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
    lib.simmr_host_free.argtypes = [C.c_void_p]
    return lib


def test_host_header_writer_agrees(host_lib):
    for rnames, lengths in ((["chr1", "plasmid|2", "x=*"], [1000, 2**33, 1]), ([], [])):
        lens = np.array(lengths, dtype=np.uint64)
        p = host_lib.simmr_host_sam_header_sorted(len(rnames), (C.c_char_p * max(len(rnames), 1))(*[r.encode() for r in rnames]), lens.ctypes.data)
        text = C.string_at(p).decode()
        host_lib.simmr_host_free(p)
        assert text == sam_header(rnames, lengths, sort_order="coordinate")


# hand-made runs of (key, line); the expected output is the stable sort of the runs laid end to end
RUNS = {
    "one run": [[(1, "a"), (1, "b"), (7, "c")]],
    "an empty run among others": [[(3, "r0.0"), (9, "r0.1")], [], [(1, "r2.0"), (3, "r2.1"), (10, "r2.2")], []],
    "equal keys inside a run and across runs": [[(5, "r0.0"), (5, "r0.1"), (5, "r0.2")], [(5, "r1.0"), (5, "r1.1")], [(4, "r2.0"), (5, "r2.1"), (6, "r2.2")]],
    "a run's last key is the next run's first": [[(1, "r0.0"), (8, "r0.1")], [(8, "r1.0"), (9, "r1.1")], [(9, "r2.0")]],
    "lines of many lengths, keys above 2^40": [[((3 << 40) | i, "x" * (i % 7) + f"r0.{i}") for i in range(0, 600, 3)],
                                               [((3 << 40) | i, "y" * (i % 5) + f"r1.{i}") for i in range(0, 600, 2)], [((2 << 40) | 999, "z")]],
    "no run": [],
}


def expected(runs):
    flat = [(key, k, i, text) for k, run in enumerate(runs) for i, (key, text) in enumerate(run)]
    assert all(run == sorted(run, key=lambda x: x[0]) for run in runs)
    return "".join(text + "\n" for _, _, _, text in sorted(flat, key=lambda x: x[:3])).encode()


@pytest.mark.parametrize("case", list(RUNS))
def test_merge_of_sorted_runs(host_lib, case):
    runs = RUNS[case]
    src = "".join(text + "\n" for run in runs for _, text in run).encode()
    lines = np.array([len(run) for run in runs] + [0], dtype=np.uint64)
    key = np.array([k for run in runs for k, _ in run] + [0], dtype=np.uint64)
    ln = np.array([len(t) + 1 for run in runs for _, t in run] + [0], dtype=np.uint64)
    offs, at = [], 0
    for run in runs:
        offs.append(at)
        at += sum(len(t) + 1 for _, t in run)
    off = np.array(offs + [0], dtype=np.uint64)
    dst = C.create_string_buffer(len(src) + 8)
    n = host_lib.simmr_host_sam_merge(len(runs), lines.ctypes.data, off.ctypes.data, key.ctypes.data, ln.ctypes.data, src, len(src), dst, len(src))
    assert n == len(src) and dst.raw[:n] == expected(runs)
    if src:  # a destination one byte short, and a run that leaves the source: refused, nothing past the capacity
        assert host_lib.simmr_host_sam_merge(len(runs), lines.ctypes.data, off.ctypes.data, key.ctypes.data, ln.ctypes.data, src, len(src), dst, len(src) - 1) == -1
        assert host_lib.simmr_host_sam_merge(len(runs), lines.ctypes.data, off.ctypes.data, key.ctypes.data, ln.ctypes.data, src, len(src) - 1, dst, len(src)) == -1


def test_merge_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = tmp_path / "sam_merge_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "sam_merge_main.cpp"), str(HOST / "host.cpp")])
    for case, runs in RUNS.items():
        text = f"{len(runs)}\n" + "".join(f"{len(run)}\n" + "".join(f"{k} {t}\n" for k, t in run) for run in runs)
        r = subprocess.run([str(exe)], input=text.encode(), capture_output=True)
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == expected(runs), (case, r.stderr[-2000:])


# one run (no file), two and three runs with equal keys inside and across them: the order is (key, run, place)
SPILL_RUNS = {
    "one run": [[(1, "a"), (1, "b"), (7, "c")]],
    "no run": [],
    "two runs, equal keys": [[(5, "r0.0"), (5, "r0.1"), (9, "r0.2")], [(5, "r1.0"), (9, "r1.1"), (9, "r1.2")]],
    "three runs, equal keys": RUNS["equal keys inside a run and across runs"],
    "three runs, the first one empty": [[], [(2, "r1.0"), (4, "r1.1")], [(2, "r2.0"), (3, "r2.1")]],
    # more than the merge's window of 2^20 bytes: the sink is called more than once
    "three runs past a window": [[(i // 2, f"r{k}.{i}." + "x" * 2000) for i in range(200)] for k in range(3)],
}


def test_sorted_run_spill_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """SortedRunSpill of simmr_host.hpp, what --sam-sorted and --bam-sorted keep their ranges in: the merged bytes, a temporary
    file only from the second run on, and none left behind, also when the sink refuses its second call"""
    exe = tmp_path / "sam_merge_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "sam_merge_main.cpp"), str(HOST / "host.cpp")])
    out = tmp_path / "spill" / "x.sam"
    out.parent.mkdir()
    for case, runs in SPILL_RUNS.items():
        text = f"{len(runs)}\n" + "".join(f"{len(run)}\n" + "".join(f"{k} {t}\n" for k, t in run) for run in runs)
        r = subprocess.run([str(exe), "spill", str(out)], input=text.encode(), capture_output=True)
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == expected(runs), (case, r.returncode, r.stderr[-2000:])
        assert list(out.parent.iterdir()) == [], case
        want = expected(runs)
        r = subprocess.run([str(exe), "spill", str(out), "2"], input=text.encode(), capture_output=True)
        if len(want) > 1 << 20:  # the second call is refused: the first window's bytes, status 1, and still no file
            assert r.returncode == 1 and r.stderr == b"" and 0 < len(r.stdout) < len(want) and want.startswith(r.stdout), case
        else:
            assert r.returncode == 0 and r.stdout == want, case
        assert list(out.parent.iterdir()) == [], case
    assert len(expected(SPILL_RUNS["three runs past a window"])) > 1 << 20


USAGE_ROWS = [
    (["--genome", "a.fna", "--output", "x.fq", "--sam-sorted"], 2, "error: --sam-sorted needs --sam"),
    (["--genome", "a.fna", "--output", "x.fq", "--sam", "x.sam", "--sam-sorted", "--devices", "0"], 2,
     "error: --sam-sorted does not combine with --devices: use --device"),
    (["--genome", "a.fna", "--sam", "x.sam", "--sam-sorted"], 2, "error: --output is required"),
    # without the new flag the rows that were there stay
    (["--genome", "a.fna", "--output", "x.fq", "--sam", "x.sam", "--devices", "0,1"], 1, "ERROR simmr-hip: --sam does not combine with --devices: use --device"),
]


@pytest.mark.parametrize("argv,status,line", USAGE_ROWS, ids=[" ".join(r[0]) for r in USAGE_ROWS])
def test_cli_usage_rows(host_lib, argv, status, line):
    r = subprocess.run([str(HOST / "simmr-hip")] + argv, capture_output=True, text=True)
    assert (r.returncode, r.stderr.splitlines()[0]) == (status, line)
    if status == 2:
        assert "--sam-sorted" in r.stderr.split("\n", 2)[2]  # the usage message follows


def test_help_describes_the_flag(host_lib):
    helptext = subprocess.check_output([str(HOST / "simmr-hip"), "--help"]).decode()
    row = helptext.split("--sam-sorted")[1].split("--stats <FILE>")[0]
    assert "SO:coordinate" in row and "needs --sam" in row and "not with --devices" in row
