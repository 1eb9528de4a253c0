"""The overlap model of tests/_overlap.py against hand-written PAF lines, and the ABI struct of simmr_amd/_abi.py against the
header: runs without a GPU."""
import ctypes as C
import subprocess
from pathlib import Path

from simmr_amd import _abi
from tests import _overlap

ROOT = Path(__file__).resolve().parent.parent

# (row, lo, hi, rev, read_id, mate)
READS = [
    (0, 100, 600, 0, 1, 0),    # 0
    (0, 300, 800, 1, 2, 0),    # 1
    (0, 300, 350, 0, 3, 0),    # 2: inside 0 and 1
    (0, 600, 900, 0, 4, 0),    # 3: abuts 0
    (1, 0, 1000, 1, 5, 0),     # 4
    (1, 0, 1000, 1, 6, 0),     # 5: the same interval, a later ordinal
    (1, 990, 1200, 0, 7, 0),   # 6
    (0, 50, 50, 0, 8, 0),      # 7: L == 0
    (1, 400, 449, 0, 4000000000, 0),  # 8: 49 bases
]
LINES_1 = [
    "1\t500\t200\t500\t-\t2\t500\t200\t500\t300\t300\t255",
    "1\t500\t200\t250\t+\t3\t50\t0\t50\t50\t50\t255",
    "2\t500\t450\t500\t-\t3\t50\t0\t50\t50\t50\t255",
    "2\t500\t0\t200\t-\t4\t300\t0\t200\t200\t200\t255",
    "5\t1000\t0\t1000\t+\t6\t1000\t0\t1000\t1000\t1000\t255",
    "5\t1000\t551\t600\t-\t4000000000\t49\t0\t49\t49\t49\t255",
    "5\t1000\t0\t10\t-\t7\t210\t0\t10\t10\t10\t255",
    "6\t1000\t551\t600\t-\t4000000000\t49\t0\t49\t49\t49\t255",
    "6\t1000\t0\t10\t-\t7\t210\t0\t10\t10\t10\t255",
]


def test_the_model_against_hand_written_lines():
    text, ps = _overlap.paf(READS, 1)
    assert text.decode().split("\n") == LINES_1 + [""]
    assert [(p[0], p[1]) for p in ps] == [(0, 1), (0, 2), (1, 2), (1, 3), (4, 5), (4, 8), (4, 6), (5, 8), (5, 6)]
    assert {(p[0], p[1]) for p in ps} == _overlap.brute(READS, 1)
    # min_overlap 50: read 8 (49 bases) leaves, and so do the pairs that share 10 bases
    text50, ps50 = _overlap.paf(READS, 50)
    assert text50.decode().split("\n") == [LINES_1[0], LINES_1[1], LINES_1[2], LINES_1[3], LINES_1[4], ""]
    assert _overlap.paf(READS, 51)[0].decode().split("\n") == [LINES_1[0], LINES_1[3], LINES_1[4], ""]


def test_paired_names_and_reverse_coordinates():
    o = {"start": [0, 270, 100], "end": [150, 120, 250], "contig": [0, 0, 0], "genome": [2, 2, 2], "read_id": [9, 9, 10], "flags": [0, 1, 0]}
    reads = _overlap.reads_of(o, {(2, 0): 0}, True, [2, 1])
    assert [r[5] for r in reads] == [1, 2, 1] and reads[1][1:4] == (120, 270, 1)
    assert _overlap.paf(reads, 1)[0].decode().split("\n") == [
        "9/1\t150\t100\t150\t+\t10/1\t150\t0\t50\t50\t50\t255",
        "9/1\t150\t120\t150\t-\t9/2\t150\t120\t150\t30\t30\t255",
        "10/1\t150\t20\t150\t-\t9/2\t150\t20\t150\t130\t130\t255", ""]


def test_overlap_cols_matches_the_header(tmp_path):
    T, ctype = _abi.OverlapCols, "simmr_overlap_cols"
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "simmr_hip.h"\nint main(void){\n' + f' printf("%zu ", sizeof({ctype}));\n'
    want = [C.sizeof(T)]
    for f, _ in T._fields_:
        src += f' printf("%zu %zu ", offsetof({ctype}, {f}), sizeof((({ctype}*)0)->{f}));\n'
        want += [getattr(T, f).offset, getattr(T, f).size]
    (tmp_path / "s.c").write_text(src + " return 0; }\n")
    subprocess.check_call(["cc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")], text=True).split()]
    assert got == want and C.sizeof(T) == 48
    assert [f for f, _ in T._fields_] == ["a", "b", "ref_start", "ref_end", "row", "capacity"]
    for name in ("simmr_overlap_reset", "simmr_overlap_add", "simmr_overlap_plan", "simmr_overlap_window", "simmr_overlap_emit", "simmr_last_overlap_ms"):
        assert name in _abi.SYMBOLS and f"int {name}(" in (ROOT / "include" / "simmr_hip.h").read_text()
