"""CPU-only checks of the coverage-depth surface: the two structs as gcc lays them out against _abi, the new symbols in the
library, the depth TSV writers of libsimmr_host.so against the Python formatter (tests/_depth.py), the options on the command
line, the numpy model against a read-by-read loop, and where the GPU tests' sizes come from."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _depth

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"
NAMES = ("simmr_depth_reset", "simmr_depth_add", "simmr_depth_emit", "simmr_depth_contig_first", "simmr_depth_summarize",
         "simmr_last_depth_ms")


@pytest.fixture(scope="module")
def host_lib():
    subprocess.check_call(["make", "-s", "-C", str(HOST)])
    lib = C.CDLL(str(HOST / "libsimmr_host.so"))
    lib.simmr_host_depth_tsv.restype = C.c_void_p
    lib.simmr_host_depth_tsv.argtypes = [C.POINTER(_abi.DepthContig), C.c_uint64, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_char_p), C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p]
    lib.simmr_host_free.argtypes = [C.c_void_p]
    return lib


def test_struct_layouts_match_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "simmr_hip.h"\nint main(void){\n'
    want = []
    for ctype, T in (("simmr_depth_contig", _abi.DepthContig), ("simmr_depth_windows", _abi.DepthWindows)):
        src += f' printf("%zu ", sizeof({ctype}));\n'
        want.append(C.sizeof(T))
        for f, _ in T._fields_:
            src += f' printf("%zu %zu ", offsetof({ctype}, {f}), sizeof((({ctype}*)0)->{f}));\n'
            want += [getattr(T, f).offset, getattr(T, f).size]
    src += ' printf("%u", SIMMR_DEPTH_HIST_BINS); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "t.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/t", f"{d}/t.c"])
        got = list(map(int, subprocess.check_output([f"{d}/t"]).decode().split()))
    assert got == want + [_abi.DEPTH_HIST_BINS] and _abi.DEPTH_HIST_BINS == _depth.HIST_BINS == 256
    assert [f for f, _ in _abi.DepthContig._fields_ if f != "reserved0"] == list(_depth.ROW_KEYS)


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, re.M) and name in _abi.SYMBOLS and hasattr(lib, name), name
    # the accessors between the library's two translation units stay inside it
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)]).decode()
    assert "simmr_depth_emit" in dyn and "eng_ext_slot" not in dyn and "eng_fail" not in dyn


def test_depth_calls_need_an_engine():
    lib = _abi.load()
    n = C.c_uint64()
    assert lib.simmr_depth_reset(None, C.byref(n), None) == _abi.EINVAL
    assert lib.simmr_depth_add(None, None, 0) == _abi.EINVAL and lib.simmr_depth_emit(None, None, 0) == _abi.EINVAL


def random_case(rng, lens, n):
    keys = [(g, c) for g in sorted(lens) for c in range(len(lens[g]))]
    pick = rng.integers(0, len(keys), n)
    g = np.array([keys[i][0] for i in pick], dtype=np.uint32)
    c = np.array([keys[i][1] for i in pick], dtype=np.uint32)
    ln = np.array([lens[int(a)][int(b)] for a, b in zip(g, c)], dtype=np.int64)
    L = np.minimum(rng.integers(0, 60, n), ln)
    lo = (rng.random(n) * (ln - L + 1)).astype(np.int64)
    rev = rng.integers(0, 2, n)
    return {"start": np.where(rev == 1, lo + L, lo).astype(np.uint64), "end": np.where(rev == 1, lo, lo + L).astype(np.uint64), "contig": c, "genome": g}


def test_model_equals_a_read_by_read_loop():
    rng = np.random.default_rng(11)
    lens = {0: [1000, 37], 2: [5, 0, 300], 5: [64]}
    cols = random_case(rng, lens, 800)
    cols["start"][:3], cols["end"][:3], cols["contig"][:3], cols["genome"][:3] = [0, 37, 300], [1000, 0, 300], [0, 1, 2], [0, 0, 2]
    d = _depth.depth(cols, lens)
    assert np.array_equal(d, _depth.depth_loop(cols, lens)) and d.size == 1406 and d.max() > 3
    L = np.abs(cols["end"].astype(np.int64) - cols["start"].astype(np.int64))
    for w in (0, 1, 7, 64, 5000):
        s = _depth.summary(d, lens, w)
        assert int(s["depth_sum"].sum()) == int(L.sum()) == int(d.sum()) and int(s["hist"].sum()) == d.size
        assert np.array_equal(s["first"], [0, 1000, 1037, 1042, 1042, 1342]) and s["covered"][1] == 37
        if w:
            n_win = [-(-x // w) for g in sorted(lens) for x in lens[g]]
            assert np.array_equal(s["first_window"], np.cumsum([0] + n_win)[:-1]) and len(s["win_sum"]) == sum(n_win)
            assert int(s["win_sum"].sum()) == int(d.sum()) and int(s["win_covered"].sum()) == int(s["covered"].sum())
            # windows never span contigs: every contig's windows give its row
            for k in range(6):
                a, b = int(s["first_window"][k]), int(s["first_window"][k]) + n_win[k]
                assert int(s["win_sum"][a:b].sum()) == int(s["depth_sum"][k]) and int(s["win_max"][a:b].max(initial=0)) == int(s["depth_max"][k])


def summary_loop(d, lens, window):
    """_depth.summary window by window and position by position, in plain Python"""
    out = {k: [] for k in ("first", "len", "covered", "depth_sum", "depth_max", "first_window", "win_sum", "win_covered", "win_max")}
    hist, x = [0] * _depth.HIST_BINS, 0
    for g in sorted(lens):
        for n in lens[g]:
            vals = [int(v) for v in d[x:x + n]]
            out["first"].append(x)
            out["len"].append(n)
            out["covered"].append(sum(1 for v in vals if v))
            out["depth_sum"].append(sum(vals))
            out["depth_max"].append(max(vals, default=0))
            out["first_window"].append(len(out["win_sum"]) if window else 0)
            for v in vals:
                hist[min(v, _depth.HIST_BINS - 1)] += 1
            for a in range(0, n, window) if window else ():
                w = vals[a:a + window]
                out["win_sum"].append(sum(w))
                out["win_covered"].append(sum(1 for v in w if v))
                out["win_max"].append(max(w))
            x += n
    out["hist"] = hist
    return out


@pytest.mark.parametrize("name", ["fragmented", "seam-1", "seam+0", "seam+3", "empty-1", "empty+0", "empty+2"])
def test_models_on_the_seam_layouts(name):
    """the layouts of tests/test_gpu_layout_seams.py (the fragmented one with fewer contigs: the loops are slow): depth[] against
    the read-by-read loop and the summary against a plain loop per window, empty contigs included"""
    from tests import test_gpu_layout_seams as seams
    lens = seams.layout_lens(name, tiles_before=2, cycles_after=20) if name == "fragmented" else seams.layout_lens(name)
    flat = [x for g in sorted(lens) for x in lens[g]]
    cols = seams.layout_reads(lens, np.random.default_rng(4), 1500)
    d = _depth.depth(cols, lens)
    assert np.array_equal(d, _depth.depth_loop(cols, lens)) and d.size == sum(flat) and d.min() >= 2
    L = np.abs(cols["end"].astype(np.int64) - cols["start"].astype(np.int64))
    assert (L == 0).sum() == flat.count(0) and int(L.sum()) == int(d.sum())
    for w in (0, 1, 3, 64, seams.TILE, max(flat) + 1):
        s, want = _depth.summary(d, lens, w), summary_loop(d, lens, w)
        for k, v in want.items():
            if w or not k.startswith("win_"):
                assert s[k].tolist() == v, (name, w, k)
        assert int(s["hist"].sum()) == d.size and ("win_sum" in s) == bool(w)
        for k in np.flatnonzero(np.array(flat) == 0):  # an empty contig: a row of zeros and no windows
            assert s["len"][k] == s["covered"][k] == s["depth_sum"][k] == s["depth_max"][k] == 0
            assert k + 1 == len(flat) or s["first_window"][k] == s["first_window"][k + 1]


def test_tsv_writers_equal_the_python_formatter(host_lib, tmp_path):
    rng = np.random.default_rng(7)
    lens = {0: [1000, 37], 1: [5, 0, 300]}
    names = {0: ("genome-a", ["chr1 first", "chr2"]), 1: ("b", ["x", "empty", "z|3"])}
    d = _depth.depth(random_case(rng, lens, 900), lens)
    d[1001] = 4_000_000_000  # (a full-width value in every column)
    for window in (7, 1000):
        s = _depth.summary(d, lens, window)
        rows = (_abi.DepthContig * 5)()
        for k in range(5):
            for f in _depth.ROW_KEYS:
                setattr(rows[k], f, int(s[f][k]))
        gid = (C.c_char_p * 2)(*[names[g][0].encode() for g in (0, 1)])
        nc = (C.c_uint32 * 2)(2, 3)
        sid = (C.c_char_p * 5)(*[x.encode() for g in (0, 1) for x in names[g][1]])
        ws, wc, wm = (np.ascontiguousarray(s[k]) for k in ("win_sum", "win_covered", "win_max"))
        p = host_lib.simmr_host_depth_tsv(rows, 5, 2, gid, nc, sid, str(tmp_path / "d.tsv").encode(), window, ws.ctypes.data, wc.ctypes.data,
                                          wm.ctypes.data, str(tmp_path / "t.tsv").encode())
        msg = C.string_at(p).decode()
        host_lib.simmr_host_free(p)
        assert msg == "OK", msg
        text, track = (tmp_path / "d.tsv").read_text(), (tmp_path / "t.tsv").read_text()
        assert text == _depth.tsv(s, names) and track == _depth.track_tsv(s, names, window)
        assert text.splitlines()[0] == "genome_id\tsequence_id\tlength\tcovered\tdepth_sum\tdepth_max" and len(text.splitlines()) == 6
        assert "b\tempty\t0\t0\t0\t0" in text.splitlines() and "." not in text and "4000000000" in text
        assert len(track.splitlines()) == 1 + len(ws) and track.splitlines()[0] == "genome_id\tsequence_id\tstart\tend\tdepth_sum\tcovered\tdepth_max"
    assert "genome-a\tchr2\t0\t37\t" in track and "b\tz|3\t0\t300\t" in track
    # a row that names a sequence the run does not have is refused
    rows[4].contig = 9
    p = host_lib.simmr_host_depth_tsv(rows, 5, 2, gid, nc, sid, str(tmp_path / "d.tsv").encode(), 0, None, None, None, None)
    msg = C.string_at(p).decode()
    host_lib.simmr_host_free(p)
    assert msg.startswith("ERR\t")


def test_depth_is_in_the_cli_surface(host_lib):
    exe = HOST / "simmr-hip"
    helptext = subprocess.check_output([str(exe), "--help"]).decode()
    for needle in ("--depth <FILE>", "--depth-track <FILE>", "--depth-window <W>"):
        assert needle in helptext, needle
    for opt in ("--depth", "--depth-track", "--depth-window"):
        r = subprocess.run([str(exe), opt], capture_output=True)
        assert r.returncode == 2 and opt.encode() in r.stderr
    r = subprocess.run([str(exe), "--depth-window", "0"], capture_output=True)
    assert r.returncode == 2 and b"--depth-window" in r.stderr


@pytest.mark.parametrize("opt", ["--depth", "--depth-track"])
def test_depth_with_devices_is_refused_before_any_device(host_lib, opt):
    r = subprocess.run([str(HOST / "simmr-hip"), "--genome", "x.fa", "--output", "x.fq", opt, "d.tsv", "--devices", "0,0"], capture_output=True)
    assert r.returncode != 0 and b"--depth does not combine with --devices" in r.stderr


def test_gpu_tests_are_sized_from_the_kernels_constants():
    """tests/test_gpu_depth.py places reads on the edges of a scan tile and stages a genome whose tile sums need more than two
    iterations of k_depth_scan_tiles' loop; both come from these constants (tests/_depth.constants parses them).  If one of
    them changes those tests resize themselves; if the FORM of the loops changes, they have to be read again."""
    src = (ROOT / "simmr_amd" / "csrc" / "depth_kernels.hip").read_text()
    tile, tops = _depth.constants()
    for needle in (f"constexpr uint32_t DEPTH_TILE = {tile};", f"constexpr uint32_t DEPTH_TOPS_WIDTH = {tops};",
                   "for (uint64_t base = 0; base < n_tiles; base += DEPTH_TOPS_WIDTH) {",
                   "const uint64_t base = (uint64_t)blockIdx.x * DEPTH_TILE;"):
        assert needle in src, needle
    host = (ROOT / "simmr_amd" / "csrc" / "depth.hip").read_text()
    assert "s->n_tiles = (s->n_positions + 1 + DEPTH_TILE - 1) / DEPTH_TILE;" in host
    # more than two iterations at fewer than 2^25 positions, as the GPU test asserts of itself
    assert 2 * tops * tile + 3 * tile + 77 < (1 << 25)
    gpu = (ROOT / "tests" / "test_gpu_depth.py").read_text()
    assert "TILE, TOPS = _depth.constants()" in gpu and "n = 2 * TOPS * TILE + 3 * TILE + 77" in gpu
