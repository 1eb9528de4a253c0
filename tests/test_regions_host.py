"""CPU-only checks of the gold-standard-assembly surface: the struct as gcc lays it out against _abi, the new symbols in the
library, the numpy model of the definition (tests/_regions.py) against its position-by-position twin and a hand-worked
example, the FASTA and TSV writers of libsimmr_host.so against the Python formatters, and the options on the command line."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _regions

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"
NAMES = ("simmr_regions_plan", "simmr_regions_emit", "simmr_last_regions_ms")


@pytest.fixture(scope="module")
def host_lib():
    subprocess.check_call(["make", "-s", "-C", str(HOST)])
    lib = C.CDLL(str(HOST / "libsimmr_host.so"))
    lib.simmr_host_gold_files.restype = C.c_void_p
    lib.simmr_host_gold_files.argtypes = [C.c_uint64] + [C.c_void_p] * 7 + [C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32),
                                                                            C.POINTER(C.c_char_p), C.c_char_p, C.c_char_p]
    lib.simmr_host_free.argtypes = [C.c_void_p]
    return lib


def test_struct_layout_matches_header():
    T, ctype = _abi.RegionsOut, "simmr_regions_out"
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "simmr_hip.h"\nint main(void){\n' + f' printf("%zu ", sizeof({ctype}));\n'
    want = [C.sizeof(T)]
    for f, _ in T._fields_:
        src += f' printf("%zu %zu ", offsetof({ctype}, {f}), sizeof((({ctype}*)0)->{f}));\n'
        want += [getattr(T, f).offset, getattr(T, f).size]
    src += " return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "t.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/t", f"{d}/t.c"])
        got = list(map(int, subprocess.check_output([f"{d}/t"]).decode().split()))
    assert got == want and C.sizeof(T) == 72
    assert [f for f, _ in T._fields_] == [n for n, _ in _regions.COLUMNS] + ["capacity", "seq", "seq_capacity"]


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, re.M) and name in _abi.SYMBOLS and hasattr(lib, name), name
    # the accessor between depth.hip and regions.hip stays inside the library
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)]).decode()
    assert "simmr_regions_emit" in dyn and "depth_layout" not in dyn and "eng_ext_slot" not in dyn
    internal = (ROOT / "simmr_amd" / "csrc" / "engine_internal.hpp").read_text()
    assert "SIMMR_HIDDEN bool depth_layout(" in internal and "ENG_EXT_REGIONS" in internal
    make = (ROOT / "simmr_amd" / "csrc" / "Makefile").read_text()
    assert make.count("engine.hip depth.hip strain.hip regions.hip\n") == 2 and "regions.hip regions_kernels.hip" in make


def test_regions_calls_need_an_engine():
    lib = _abi.load()
    n, ms = C.c_uint64(), C.c_float()
    assert lib.simmr_regions_plan(None, None, 1, 1, C.byref(n), C.byref(n)) == _abi.EINVAL
    assert lib.simmr_regions_emit(None, None, None) == _abi.EINVAL and lib.simmr_last_regions_ms(None, C.byref(ms)) == _abi.EINVAL


def test_hand_worked_example():
    # two genomes; slot 0: contigs of 6 and 3 positions, slot 2: one of 4.  '|' marks the contig boundaries:
    #   depth  0 2 2 0 1 3 | 3 1 0 | 5 5 5 5
    lens = {0: [6, 3], 2: [4]}
    d = np.array([0, 2, 2, 0, 1, 3, 3, 1, 0, 5, 5, 5, 5], dtype=np.uint32)
    r = _regions.regions(d, lens)
    assert r["genome"].tolist() == [0, 0, 0, 2] and r["contig"].tolist() == [0, 0, 1, 0]
    assert r["start"].tolist() == [1, 4, 0, 0] and r["len"].tolist() == [2, 2, 2, 4]  # (the run 4 .. 7 is cut at the boundary)
    assert r["depth_sum"].tolist() == [4, 4, 4, 20] and r["seq_off"].tolist() == [0, 2, 4, 6, 10]
    r = _regions.regions(d, lens, min_depth=2)
    assert r["start"].tolist() == [1, 5, 0, 0] and r["len"].tolist() == [2, 1, 1, 4] and r["seq_off"].tolist() == [0, 2, 3, 4, 8]
    r = _regions.regions(d, lens, min_depth=2, min_len=2)
    assert r["start"].tolist() == [1, 0] and r["genome"].tolist() == [0, 2] and r["seq_off"].tolist() == [0, 2, 6]
    r = _regions.regions(d, lens, min_depth=6)
    assert r["start"].size == 0 and r["seq_off"].tolist() == [0]
    contigs = {0: [np.frombuffer(b"ACGTNA", dtype=np.uint8), np.frombuffer(b"GG-", dtype=np.uint8)], 2: [np.frombuffer(b"TTAA", dtype=np.uint8)]}
    assert _regions.bases(_regions.regions(d, lens), contigs).tobytes() == b"CGNAGGTTAA"


def test_model_equals_a_position_by_position_loop():
    rng = np.random.default_rng(5)
    lens = {0: [700, 1, 37], 2: [5, 0, 300, 1], 5: [64]}
    n = sum(sum(v) for v in lens.values())
    for p in (0.05, 0.5, 0.95):
        d = (rng.random(n) < p).astype(np.uint32) * rng.integers(1, 6, n).astype(np.uint32)
        for md, ml in ((1, 1), (3, 1), (1, 2), (2, 7)):
            a, b = _regions.regions(d, lens, md, ml), _regions.regions_loop(d, lens, md, ml)
            _regions.assert_regions(a, b, (p, md, ml))
            assert int(a["seq_off"][-1]) == int(a["len"].sum()) and (a["len"] >= ml).all()
            if ml == 1:
                assert int(a["len"].sum()) == int((d >= md).sum()) and int(a["depth_sum"].sum()) == int(d[d >= md].sum())
    full = _regions.regions(np.ones(n, dtype=np.uint32), lens)
    assert full["len"].tolist() == [700, 1, 37, 5, 300, 1, 64] and full["contig"].tolist() == [0, 1, 2, 0, 2, 3, 0]  # (the empty contig has no region)


def test_the_seam_layouts_are_what_their_cases_need():
    from tests import test_gpu_layout_seams as seams
    seams.test_the_layouts_are_what_the_cases_need()  # (plain arithmetic on the kernels' constants: checked without a GPU too)


@pytest.mark.parametrize("name", ["fragmented", "seam-1", "seam+0", "seam+3", "empty-1", "empty+0", "empty+2"])
def test_model_equals_the_loop_on_the_seam_layouts(name):
    """the layouts and the depth arrays of tests/test_gpu_layout_seams.py (the fragmented one with fewer contigs: the loop is
    slow), empty contigs included"""
    from tests import test_gpu_layout_seams as seams
    lens = seams.layout_lens(name, tiles_before=2, cycles_after=20) if name == "fragmented" else seams.layout_lens(name)
    flat = [x for g in sorted(lens) for x in lens[g]]
    g, c, first = _regions.layout(lens)
    n = int(first[-1])
    rows = {x: k for k, x in enumerate(zip(g.tolist(), c.tolist()))}
    rng = np.random.default_rng(6)
    cases = [("all covered", np.full(n, 2, dtype=np.uint32), 2, 1)]
    for p in (0.5, 0.95):
        d = (rng.random(n) < p).astype(np.uint32) * rng.integers(1, 9, n).astype(np.uint32)
        cases += [((p, ml), d, 1, ml) for ml in (1, 2)]
    for what, d in seams.boundary_depths(first, n).items():
        cases += [((what, ml), d, 1, ml) for ml in (1, 2)]
    big, k = seams.large_depths(lens, first, n, rng)
    cases += [(("large", hex(md)), big, md, 1) for md in (1, 0x80000000, 0xFFFFFFFF)]
    for what, d, md, ml in cases:
        a, b = _regions.regions(d, lens, md, ml), _regions.regions_loop(d, lens, md, ml)
        _regions.assert_regions(a, b, (name, what))
        assert int(a["seq_off"][-1]) == int(a["len"].sum()) and (a["len"] >= ml).all()
        row = np.array([rows[x] for x in zip(a["genome"].tolist(), a["contig"].tolist())], dtype=np.int64)
        assert (a["start"] + a["len"] <= np.array(flat, dtype=np.uint64)[row]).all()  # inside its contig: never an empty contig's
    full = _regions.regions(cases[0][1], lens, 2, 1)
    assert full["len"].tolist() == [x for x in flat if x] and int(_regions.regions(big, lens, 0xFFFFFFFF)["depth_sum"][0]) == 0xFFFFFFFF * flat[k] > 1 << 32


def gold_files(host_lib, r, seq, names, fasta_path, tsv_path):
    n = len(r["genome"])
    cols = [np.ascontiguousarray(r[k]) for k, _ in _regions.COLUMNS]
    s = np.frombuffer(seq, dtype=np.uint8) if seq else np.zeros(1, dtype=np.uint8)
    slots = sorted(names)
    gid = (C.c_char_p * len(slots))(*[names[g][0].encode() for g in slots])
    nc = (C.c_uint32 * len(slots))(*[len(names[g][1]) for g in slots])
    flat = [x.encode() for g in slots for x in names[g][1]]
    sid = (C.c_char_p * len(flat))(*flat)
    p = host_lib.simmr_host_gold_files(n, *[c.ctypes.data for c in cols], s.ctypes.data, len(slots), gid, nc, sid,
                                       str(fasta_path).encode() if fasta_path else None, str(tsv_path).encode() if tsv_path else None)
    msg = C.string_at(p).decode()
    host_lib.simmr_host_free(p)
    return msg


def test_writers_equal_the_python_formatters(host_lib, tmp_path):
    rng = np.random.default_rng(3)
    names = {0: ("genome-a", ["chr1 first", "chr2"]), 1: ("b", ["x|3"])}
    lens = {0: [400, 161], 1: [90]}
    contigs = {g: [np.frombuffer(b"ACGTN-", dtype=np.uint8)[rng.integers(0, 6, x)] for x in v] for g, v in lens.items()}
    # regions of 79, 80, 81 and 160 bases (the 80-column wrap), then one of 1 and the whole of two contigs
    d = np.zeros(651, dtype=np.uint32)
    for a, n in ((0, 79), (80, 80), (161, 81), (243, 1)):
        d[a:a + n] = rng.integers(1, 9, n)
    d[400:560] = 4_000_000_000 // 160
    d[561:] = 2
    r = _regions.regions(d, lens)
    assert r["len"].tolist() == [79, 80, 81, 1, 160, 90]
    seq = _regions.bases(r, contigs).tobytes()
    fa, tv = tmp_path / "g.fa", tmp_path / "g.tsv"
    assert gold_files(host_lib, r, seq, names, fa, tv) == "OK"
    text = fa.read_bytes()
    assert text == _regions.fasta(r, seq, names) and tv.read_text() == _regions.tsv(r, names)
    lines = text.split(b"\n")
    # 79: one short line; 80: one full line and no empty one; 81: 80 + 1; 1; 160: two full lines; 90: 80 + 10
    assert [len(x) if not x.startswith(b">") else -1 for x in lines] == [-1, 79, -1, 80, -1, 80, 1, -1, 1, -1, 80, 80, -1, 80, 10, 0]
    assert lines[0] == b">genome-a|chr1 first:1-79 depth_sum=%d" % int(d[:79].sum()) and lines[4].startswith(b">genome-a|chr1 first:162-242 ")
    assert lines[9] == b">genome-a|chr2:1-160 depth_sum=4000000000" and lines[12] == b">b|x|3:1-90 depth_sum=180"
    assert tv.read_text().splitlines()[0] == "genome_id\tsequence_id\tstart\tlength\tdepth_sum\tseq_off" and "b\tx|3\t0\t90\t180\t401" in tv.read_text().splitlines()
    # no regions: an empty FASTA and the TSV's header line
    r0 = _regions.regions(np.zeros(651, dtype=np.uint32), lens)
    assert gold_files(host_lib, r0, b"", names, fa, tv) == "OK" and fa.read_bytes() == b"" and tv.read_text() == _regions.TSV_HEADER
    # a region that names a sequence the run does not have, or leaves the base stream, is refused
    bad = dict(r, contig=r["contig"].copy())
    bad["contig"][5] = 9
    assert gold_files(host_lib, bad, seq, names, fa, None).startswith("ERR\t")
    assert fa.read_bytes() == b""  # (a refused list leaves the file as it was)
    short = dict(r, seq_off=r["seq_off"].copy())
    short["seq_off"][5] = short["seq_off"][6]
    assert gold_files(host_lib, short, seq, names, fa, None).startswith("ERR\t") and fa.read_bytes() == b""


def test_gold_flags_are_in_the_cli_surface(host_lib):
    exe = HOST / "simmr-hip"
    helptext = subprocess.check_output([str(exe), "--help"]).decode()
    for needle in ("--gold-assembly <FILE>", "--gold-regions <FILE>", "--gold-min-depth <D>", "--gold-min-length <M>"):
        assert needle in helptext, needle
    for opt in ("--gold-assembly", "--gold-regions", "--gold-min-depth", "--gold-min-length"):
        r = subprocess.run([str(exe), opt], capture_output=True)
        assert r.returncode == 2 and opt.encode() in r.stderr
    for opt in ("--gold-min-depth", "--gold-min-length"):
        for bad in ("0", "-1", "x"):
            r = subprocess.run([str(exe), opt, bad], capture_output=True)
            assert r.returncode == 2 and opt.encode() in r.stderr


@pytest.mark.parametrize("opt", ["--gold-assembly", "--gold-regions"])
def test_gold_with_devices_is_refused_before_any_device(host_lib, opt):
    r = subprocess.run([str(HOST / "simmr-hip"), "--genome", "x.fa", "--output", "x.fq", opt, "g.out", "--gold-min-depth", "2", "--gold-min-length", "50",
                        "--devices", "0,0"], capture_output=True)
    assert r.returncode != 0 and f"{opt} does not combine with --devices: use --device".encode() in r.stderr


def test_gpu_tests_are_sized_from_the_kernels_constants():
    """tests/test_gpu_regions.py places regions on the edges of a tile and stages a genome with more tiles than one iteration
    of k_regions_scan's loop takes; both come from these constants."""
    tile, tops, run_tile = _regions.constants()
    assert (tile, tops, run_tile) == (4096, 1024, 256)
    host = (ROOT / "simmr_amd" / "csrc" / "regions.hip").read_text()
    assert "const uint64_t n_tiles = (n + 1 + REGIONS_TILE - 1) / REGIONS_TILE;" in host
    src = (ROOT / "simmr_amd" / "csrc" / "regions_kernels.hip").read_text()
    assert "for (uint64_t base = 0; base < n; base += REGIONS_TOPS_WIDTH) {" in src
