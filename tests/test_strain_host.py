"""CPU-only checks of the strain-divergence surface: the numpy Philox of tests/_strain.py against the oracle library's, the
struct as gcc lays it out against _abi, the new symbols in the library, the law of the model (site rate and alternates, with
derived bounds), the options on the command line, the TSV writer of libsimmr_host.so against the Python formatter, and where
the GPU tests' sizes come from."""
import ctypes as C
import math
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _strain

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"
NAMES = ("simmr_strain_plan", "simmr_strain_apply", "simmr_last_strain_ms")


@pytest.fixture(scope="module")
def host_lib():
    subprocess.check_call(["make", "-s", "-C", str(HOST)])
    lib = C.CDLL(str(HOST / "libsimmr_host.so"))
    lib.simmr_host_strain_tsv.restype = C.c_void_p
    lib.simmr_host_strain_tsv.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32,
                                          C.POINTER(C.c_char_p), C.c_int, C.c_char_p]
    lib.simmr_host_free.argtypes = [C.c_void_p]
    return lib


def test_numpy_philox_equals_the_oracle_library(oracle):
    """oracle/philox.c is pinned by the Random123 vectors (tests/test_oracle_kat.py); the model's vectorised form must be it"""
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 1 << 32, (1000, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 1 << 32, (1000, 2), dtype=np.uint64).astype(np.uint32)
    ctr[0], key[0] = 0, 0
    ctr[1], key[1] = 0xFFFFFFFF, 0xFFFFFFFF
    got = _strain.philox4x32_10(ctr, key)
    oracle.orc_philox4x32_10.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    oracle.orc_philox4x32_10.restype = None
    o = (C.c_uint32 * 4)()
    for i in range(1000):
        oracle.orc_philox4x32_10((C.c_uint32 * 4)(*map(int, ctr[i])), (C.c_uint32 * 2)(*map(int, key[i])), o)
        assert list(o) == list(map(int, got[i])), i
    assert list(map(int, got[0])) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]  # Random123's first known answer


def test_struct_layout_matches_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "simmr_hip.h"\nint main(void){\n'
    src += ' printf("%zu ", sizeof(simmr_strain_out));\n'
    want = [C.sizeof(_abi.StrainOut)]
    for f, _ in _abi.StrainOut._fields_:
        src += f' printf("%zu %zu ", offsetof(simmr_strain_out, {f}), sizeof(((simmr_strain_out*)0)->{f}));\n'
        want += [getattr(_abi.StrainOut, f).offset, getattr(_abi.StrainOut, f).size]
    src += ' printf("%d", SIMMR_ABI_VERSION); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "t.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/t", f"{d}/t.c"])
        got = list(map(int, subprocess.check_output([f"{d}/t"]).decode().split()))
    assert got == want + [1]  # (the change only adds symbols: the ABI version stays)
    assert [f for f, _ in _abi.StrainOut._fields_] == ["contig", "pos", "ref", "alt", "capacity"]


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, re.M) and name in _abi.SYMBOLS and hasattr(lib, name), name
    # the accessors between the library's translation units stay inside it
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)]).decode()
    assert "simmr_strain_apply" in dyn and "eng_genome_planes" not in dyn and "eng_planes_rewritten" not in dyn
    for needle in ("strain sites, version 1", "(pos >> 2, 5, c, 0x72000003)", "T32 = floor((1 - identity) * 2^32 + 0.5)"):
        assert needle.lower() in header.lower(), needle


def test_strain_calls_need_an_engine():
    lib = _abi.load()
    n, ms = C.c_uint64(), C.c_float()
    assert lib.simmr_strain_plan(None, 0, 0.99, 1, C.byref(n)) == _abi.EINVAL
    assert lib.simmr_strain_apply(None, 0, None) == _abi.EINVAL and lib.simmr_last_strain_ms(None, C.byref(ms)) == _abi.EINVAL


def test_thresholds():
    assert _strain.thresholds(1.0) == (0, 0, 0)
    assert _strain.thresholds(0.25) == (3 << 30, 1 << 30, 1 << 31)
    t, a, b = _strain.thresholds(0.97)
    assert t == math.floor(0.03 * 2**32 + 0.5) or abs(t - 0.03 * 2**32) <= 1  # (1 - 0.97 is not 0.03 to the last bit)
    assert a == -(-t // 3) and b == -(-2 * t // 3) and 3 * a >= t > 3 * (a - 1) and 3 * b >= 2 * t > 3 * (b - 1)


N_LAW = 4_000_000


@pytest.fixture(scope="module")
def law_genome():
    rng = np.random.default_rng(3)
    return _strain.ACGT[rng.integers(0, 4, N_LAW)]


@pytest.mark.parametrize("identity", [0.97, 0.25])
def test_law_of_the_model(law_genome, identity):
    """Every base draws an independent uniform word X: it is a site with probability d = T32 / 2^32, so the count over n bases
    is binomial(n, d) and lies within 5 standard deviations sqrt(n d (1 - d)) of n d (two-sided tail below 6e-7).  Given a
    site, X is uniform below T32 and A, B cut that range in thirds (to within one word): each alternate's count over k sites
    is binomial(k, 1/3), within 5 sqrt(k 2/9) of k / 3.  The seed is fixed; a seed outside the bounds is a finding."""
    seed = 0x1234_5678_9ABC_DEF0
    t32, _, _ = _strain.thresholds(identity)
    d = t32 / 2.0**32
    pos, ref, alt = _strain.sites_of(law_genome, 0, identity, seed)
    k = pos.size
    print(f"identity {identity}: {k} sites of {N_LAW}, expected {N_LAW * d:.1f} +- {5 * math.sqrt(N_LAW * d * (1 - d)):.1f}")
    assert abs(k - N_LAW * d) <= 5 * math.sqrt(N_LAW * d * (1 - d))
    s = (_strain.CODE[alt].astype(np.int64) - _strain.CODE[ref].astype(np.int64)) & 3
    assert s.min() >= 1  # an alternate is never the base itself
    for v in (1, 2, 3):
        n_v = int((s == v).sum())
        print(f"  s = {v}: {n_v}, expected {k / 3:.1f} +- {5 * math.sqrt(k * 2 / 9):.1f}")
        assert abs(n_v - k / 3) <= 5 * math.sqrt(k * 2 / 9)
    assert np.all(np.diff(pos.astype(np.int64)) > 0) and np.array_equal(ref, law_genome[pos.astype(np.int64)])


def test_identity_one_and_the_exception_plane():
    rng = np.random.default_rng(9)
    seq = _strain.ACGT[rng.integers(0, 4, 5000)].copy()
    seq[100:180] = ord("N")
    seq[1000:1033] = ord("-")
    seq[rng.integers(0, 5000, 300)] = ord("N")
    out, cols = _strain.diverge([seq], 1.0, 77)
    assert cols["pos"].size == 0 and np.array_equal(out[0], seq)
    out, cols = _strain.diverge([seq], 0.25, 77)
    exc = (seq == ord("N")) | (seq == ord("-"))
    assert not exc[cols["pos"].astype(np.int64)].any() and np.array_equal(out[0][exc], seq[exc])
    assert 0.70 < cols["pos"].size / (~exc).sum() < 0.80 and np.array_equal(np.flatnonzero(out[0] != seq), cols["pos"].astype(np.int64))
    # the contig index and both seed words are in the draw
    a = _strain.sites_of(seq, 0, 0.9, 77)[0]
    for other in (_strain.sites_of(seq, 1, 0.9, 77)[0], _strain.sites_of(seq, 0, 0.9, 77 + (1 << 32))[0], _strain.sites_of(seq, 0, 0.9, 78)[0]):
        assert not np.array_equal(a, other)


def test_seed_rule():
    assert _strain.genome_seed(7, 0) == 7 + 0x9E3779B97F4A7C15 and _strain.genome_seed(2**64 - 1, 1) == (2 * 0x9E3779B97F4A7C15 - 1) % 2**64
    from simmr_amd import simulate
    assert all(simulate.strain_seed(s, i) == _strain.genome_seed(s, i) for s in (0, 7, 2**64 - 1) for i in (0, 1, 5))


# argv -> (exit status, first line of stderr).  None of them gets as far as a device.
USAGE_ROWS = [
    (["--genome", "a.fna", "--output", "x.fq", "--strain-sites", "s.tsv"], 2, "error: --strain-sites needs --with-ani"),
    (["--strain-sites", "s.tsv"], 2, "error: --strain-sites needs --with-ani"),
    (["--with-ani", "24.9"], 2, "error: invalid value for --with-ani"),
    (["--with-ani", "100.1"], 2, "error: invalid value for --with-ani"),
    (["--with-ani", "abc"], 2, "error: invalid value for --with-ani"),
    (["--with-ani"], 2, "error: invalid value for --with-ani"),
    (["--with-ani", "-99"], 2, "error: invalid value for --with-ani"),
    (["--with-ani", "nan"], 2, "error: invalid value for --with-ani"),
    (["--with-ani", "9e1"], 2, "error: invalid value for --with-ani"),
    (["--strain-sites"], 2, "error: a value is required for '--strain-sites'"),
    (["--strain-sites="], 2, "error: a file name is required for '--strain-sites'"),
    # accepted values get as far as the next usage error
    (["--with-ani", "99.5"], 2, "error: one of --genome / --genome-file is required"),
    (["--with-ani", "25", "--with-ani=100", "--strain-sites", "s.tsv"], 2, "error: one of --genome / --genome-file is required"),
]


@pytest.mark.parametrize("argv,status,line", USAGE_ROWS, ids=[" ".join(r[0]) for r in USAGE_ROWS])
def test_cli_usage_rows(host_lib, argv, status, line):
    r = subprocess.run([str(HOST / "simmr-hip")] + argv, capture_output=True, text=True)
    assert (r.returncode, r.stderr.splitlines()[0]) == (status, line)


def test_help_describes_the_flags(host_lib):
    helptext = subprocess.check_output([str(HOST / "simmr-hip"), "--help"]).decode()
    assert "--strain-sites <FILE>" in helptext and "not implemented" not in helptext
    assert re.search(r"--with-ani <N>\s+Generate reads with an average identity of N", helptext)


def test_tsv_writer_equals_the_python_formatter(host_lib, tmp_path):
    rng = np.random.default_rng(2)
    contigs = [_strain.ACGT[rng.integers(0, 4, n)] for n in (700, 1, 90)]
    _, cols = _strain.diverge(contigs, 0.9, 11)
    cols["pos"][-1] = 2**34 - 1  # (a full-width position)
    sids = ["chr1 first", "lone", "z|3"]
    path = tmp_path / "s.tsv"
    want = _strain.TSV_HEADER
    for with_header, gid in ((1, "genome-a"), (0, "b")):  # the second genome appends
        p = host_lib.simmr_host_strain_tsv(cols["pos"].size, cols["contig"].ctypes.data, cols["pos"].ctypes.data, cols["ref"].ctypes.data,
                                           cols["alt"].ctypes.data, gid.encode(), 3, (C.c_char_p * 3)(*[s.encode() for s in sids]),
                                           with_header, str(path).encode())
        msg = C.string_at(p).decode()
        host_lib.simmr_host_free(p)
        assert msg == "OK", msg
        want += _strain.tsv_rows(cols, gid, sids)
    text = path.read_text()
    assert text == want and text.splitlines()[0] == "genome_id\tsequence_id\tposition\tref\talt"
    assert len(text.splitlines()) == 1 + 2 * cols["pos"].size and f"b\tz|3\t{2**34 - 1}\t" in text and cols["pos"].size > 40
    # a site that names a sequence the genome does not have is refused
    cols["contig"][0] = 3
    p = host_lib.simmr_host_strain_tsv(cols["pos"].size, cols["contig"].ctypes.data, cols["pos"].ctypes.data, cols["ref"].ctypes.data,
                                       cols["alt"].ctypes.data, b"g", 3, (C.c_char_p * 3)(*[s.encode() for s in sids]), 1, str(path).encode())
    msg = C.string_at(p).decode()
    host_lib.simmr_host_free(p)
    assert msg.startswith("ERR\t")


def test_gpu_tests_are_sized_from_the_kernels_constants():
    """tests/test_gpu_strain.py places contigs on the edges of a tile and stages a genome whose tile counts need two iterations
    of k_strain_scan_tiles' loop; both come from these constants.  If one of them changes those tests resize themselves; if
    the FORM of the loops changes, they have to be read again."""
    src = (ROOT / "simmr_amd" / "csrc" / "strain_kernels.hip").read_text()
    tile, tops = _strain.constants()
    for needle in (f"constexpr uint32_t STRAIN_TILE = {tile};", f"constexpr uint32_t STRAIN_TOPS_WIDTH = {tops};",
                   "for (; base < n_tiles; base += STRAIN_TOPS_WIDTH) {", "const uint64_t w = (uint64_t)blockIdx.x * STRAIN_WG + tid;",
                   "static_assert(STRAIN_TILE == STRAIN_WG * STRAIN_WORD_BASES"):
        assert needle in src, needle
    assert "s->n_tiles = (p.plane_words + STRAIN_WG - 1) / STRAIN_WG;" in (ROOT / "simmr_amd" / "csrc" / "strain.hip").read_text()
    gpu = (ROOT / "tests" / "test_gpu_strain.py").read_text()
    assert "TILE, TOPS = _strain.constants()" in gpu and "TOPS * TILE + 5 * TILE + 77" in gpu
    assert tops * tile + 5 * tile + 77 < (1 << 23)  # (seconds in the numpy model)
