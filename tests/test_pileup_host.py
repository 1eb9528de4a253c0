"""CPU-only checks of the allele-count surface: the numpy restatement (tests/_pileup.py) on a case counted by hand, its sum
invariant against the depth model (tests/_depth.py), the struct as gcc lays it out against _abi, the new symbols in the
library, the option on the command line, and the VCF writer of libsimmr_host.so against the Python formatter."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from tests import _depth, _pileup

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"
NAMES = ("simmr_pileup_reset", "simmr_pileup_add", "simmr_pileup_read", "simmr_last_pileup_ms")


def columns(reads):
    """[(genome, contig, lo, L, reverse, bytes as written)] -> compact host columns"""
    g, c, lo, L, rev = (np.array([r[k] for r in reads], dtype=np.int64) for k in range(5))
    assert all(len(r[5]) == r[3] for r in reads)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum(L, out=off[1:])
    return {"start": np.where(rev == 1, lo + L, lo).astype(np.uint64), "end": np.where(rev == 1, lo, lo + L).astype(np.uint64),
            "contig": c.astype(np.uint32), "genome": g.astype(np.uint32), "flags": rev.astype(np.uint8), "seq_off": off,
            "seq": np.frombuffer(b"".join(r[5] for r in reads), dtype=np.uint8)}


def test_hand_computed_case():
    """nine reads, six sites; slots 0 and 2, the second with two contigs: firsts 0, 20 and 30"""
    lens = {0: [20], 2: [10, 8]}
    sites = (np.array([0, 0, 0, 2, 2, 2], np.uint32), np.array([0, 0, 0, 0, 0, 1], np.uint32), np.array([3, 10, 19, 0, 9, 0], np.uint64))
    reads = [
        (0, 0, 3, 5, 0, b"ACGTN"),         # site 0 at its first base: A forward
        (0, 0, 0, 11, 1, b"TACGTACGAAA"),  # reverse over 0..10: site 0 is byte 7 (G, observed C), site 1 its byte 0 (T, observed A)
        (0, 0, 10, 10, 0, b"GCCCCCCCCn"),  # site 1 at its first base (G), site 2 at its last (n: class 4)
        (0, 0, 19, 1, 1, b"N"),            # one base, reverse, on the contig's last position: class 4 stays 4
        (0, 0, 5, 0, 0, b""),              # L = 0 covers nothing
        (2, 0, 0, 10, 0, b"CAAAAAAAAT"),   # a whole contig: ends at its last base, does not reach site 5 on the next contig
        (2, 0, 1, 8, 1, b"AAAAAAAA"),      # site 3 is its lo - 1, site 4 its lo + L: neither counts
        (2, 1, 0, 8, 1, b"CCCCCCC-"),      # reverse: site 5 (pos 0) is its last byte, '-': class 4
        (2, 0, 0, 10, 1, b"ACCCCCCCCG"),   # the first contig again, reverse: site 3 is byte 9 (G, observed C), site 4 byte 0 (A, observed T)
    ]
    want = np.array([
        [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0]],
        [[0, 0, 1, 0, 0], [1, 0, 0, 0, 0]],
        [[0, 0, 0, 0, 1], [0, 0, 0, 0, 1]],
        [[0, 1, 0, 0, 0], [0, 1, 0, 0, 0]],
        [[0, 0, 0, 1, 0], [0, 0, 0, 1, 0]],
        [[0, 0, 0, 0, 0], [0, 0, 0, 0, 1]],
    ], dtype=np.uint32)
    got = _pileup.pileup(columns(reads), sites, lens)
    assert got.dtype == np.uint32 and np.array_equal(got, want), got.tolist()
    assert _pileup.site_keys(sites, lens).tolist() == [3, 10, 19, 20, 29, 30]
    # reads in any order, and in two parts, add up to the same table
    assert np.array_equal(_pileup.pileup(columns(reads[::-1]), sites, lens), want)
    assert np.array_equal(_pileup.pileup(columns(reads[:4]), sites, lens) + _pileup.pileup(columns(reads[4:]), sites, lens), want)
    for bad in ((sites[0], sites[1], np.array([3, 10, 10, 0, 9, 0], np.uint64)), (sites[0], sites[1], np.array([3, 10, 20, 0, 9, 0], np.uint64)),
                (sites[0][::-1], sites[1][::-1], sites[2][::-1])):
        with pytest.raises(AssertionError):
            _pileup.site_keys(bad, lens)


def test_the_ten_counts_sum_to_depth():
    """the invariant of the header: mates count separately, as in read depth"""
    rng = np.random.default_rng(4)
    lens = {0: [5000, 1], 1: [300], 4: [2000, 700, 64]}
    where = [(g, c) for g in lens for c in range(len(lens[g]))]
    reads = []
    for _ in range(3000):
        g, c = where[rng.integers(0, len(where))]
        n = lens[g][c]
        lo = int(rng.integers(0, n + 1))
        L = int(rng.integers(0, min(n - lo, 400) + 1))
        reads.append((g, c, lo, L, int(rng.integers(0, 2)), bytes(np.frombuffer(b"ACGTNa-", dtype=np.uint8)[rng.integers(0, 7, L)])))
    cols = columns(reads)
    layout, n_positions = _depth.layout(lens)
    keys = np.flatnonzero(rng.random(n_positions) < 0.3)
    contig_of = np.searchsorted(layout["first"].astype(np.int64), keys, side="right") - 1
    sites = (layout["genome"][contig_of], layout["contig"][contig_of], (keys - layout["first"].astype(np.int64)[contig_of]).astype(np.uint64))
    assert np.array_equal(_pileup.site_keys(sites, lens), keys)
    counts = _pileup.pileup(cols, sites, lens)
    d = _depth.depth(cols, lens)
    assert np.array_equal(counts.sum(axis=(1, 2)), d[keys]) and d[keys].max() > 50 and counts[:, :, 4].sum() > 0
    assert counts[:, 0].sum() > 0 and counts[:, 1].sum() > 0


def test_struct_layout_matches_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "simmr_hip.h"\nint main(void){\n'
    src += ' printf("%zu ", sizeof(simmr_pileup_sites));\n'
    want = [C.sizeof(_abi.PileupSites)]
    for f, _ in _abi.PileupSites._fields_:
        src += f' printf("%zu %zu ", offsetof(simmr_pileup_sites, {f}), sizeof(((simmr_pileup_sites*)0)->{f}));\n'
        want += [getattr(_abi.PileupSites, f).offset, getattr(_abi.PileupSites, f).size]
    src += ' printf("%d", SIMMR_ABI_VERSION); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "t.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/t", f"{d}/t.c"])
        got = list(map(int, subprocess.check_output([f"{d}/t"]).decode().split()))
    assert got == want + [1]  # (the change only adds symbols: the ABI version stays)
    assert [f for f, _ in _abi.PileupSites._fields_] == ["genome", "contig", "pos", "n"]


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, re.M) and name in _abi.SYMBOLS and hasattr(lib, name), name
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)]).decode()
    assert "simmr_pileup_add" in dyn and "eng_ext_slot" not in dyn
    for needle in ("uint32_t counts[n][2][5]", "strictly ascending by (slot, contig, pos)", "0 <-> 3", "INVARIANT: the ten counts of site s sum to"):
        assert needle in header, needle


def test_pileup_calls_need_an_engine():
    lib = _abi.load()
    ms, sites = C.c_float(), _abi.PileupSites(None, None, None, 0)
    assert lib.simmr_pileup_reset(None, C.byref(sites)) == _abi.EINVAL and lib.simmr_pileup_add(None, None, 0) == _abi.EINVAL
    assert lib.simmr_pileup_read(None, None, 0) == _abi.EINVAL and lib.simmr_last_pileup_ms(None, C.byref(ms)) == _abi.EINVAL


@pytest.fixture(scope="module")
def host_lib():
    subprocess.check_call(["make", "-s", "-C", str(HOST)])
    lib = C.CDLL(str(HOST / "libsimmr_host.so"))
    lib.simmr_host_strain_vcf.restype = C.c_void_p
    lib.simmr_host_strain_vcf.argtypes = [C.c_uint64] + [C.c_void_p] * 6 + [C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p, C.POINTER(C.c_char_p),
                                                                             C.c_void_p, C.c_char_p]
    lib.simmr_host_free.argtypes = [C.c_void_p]
    return lib


USAGE_ROWS = [
    (["--genome", "a.fna", "--output", "x.fq", "--strain-vcf", "v.vcf"], 2, "error: --strain-vcf needs --with-ani"),
    (["--strain-vcf"], 2, "error: a value is required for '--strain-vcf'"),
    (["--strain-vcf="], 2, "error: a file name is required for '--strain-vcf'"),
    (["--with-ani", "97", "--strain-vcf", "v.vcf", "--strain-sites", "s.tsv"], 2, "error: one of --genome / --genome-file is required"),
]


@pytest.mark.parametrize("argv,status,line", USAGE_ROWS, ids=[" ".join(r[0]) for r in USAGE_ROWS])
def test_cli_usage_rows(host_lib, argv, status, line):
    r = subprocess.run([str(HOST / "simmr-hip")] + argv, capture_output=True, text=True)
    assert (r.returncode, r.stderr.splitlines()[0]) == (status, line)


def test_help_describes_the_flag(host_lib):
    helptext = subprocess.check_output([str(HOST / "simmr-hip"), "--help"]).decode()
    assert "--strain-vcf <FILE>" in helptext and "needs --with-ani" in helptext


def write_vcf(lib, sites, ref, alt, counts, names, lens, path):
    slots = sorted(names)
    assert slots == list(range(len(slots)))  # (the writer's genomes are the run's, indexed from 0)
    gids = (C.c_char_p * len(slots))(*[names[g][0].encode() for g in slots])
    n_contigs = np.array([len(names[g][1]) for g in slots], dtype=np.uint32)
    sids = [s.encode() for g in slots for s in names[g][1]]
    flat = np.array([n for g in slots for n in lens[g]], dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    p = lib.simmr_host_strain_vcf(len(sites[2]), sites[0].ctypes.data, sites[1].ctypes.data, sites[2].ctypes.data, ref.ctypes.data, alt.ctypes.data,
                                  counts.ctypes.data, len(slots), gids, n_contigs.ctypes.data, (C.c_char_p * len(sids))(*sids), flat.ctypes.data,
                                  str(path).encode())
    msg = C.string_at(p).decode()
    lib.simmr_host_free(p)
    return msg


def test_vcf_writer_equals_the_python_formatter(host_lib, tmp_path):
    rng = np.random.default_rng(6)
    names = {0: ("genome-a", ["chr1 first", "lone"]), 1: ("b", ["z|3"])}
    lens = {0: [700, 1], 1: [2**34]}
    sites = (np.array([0, 0, 0, 1, 1], np.uint32), np.array([0, 0, 1, 0, 0], np.uint32), np.array([0, 699, 0, 5, 2**34 - 1], np.uint64))
    ref = np.frombuffer(b"ACGTA", dtype=np.uint8).copy()
    alt = np.frombuffer(b"CATGT", dtype=np.uint8).copy()
    counts = rng.integers(0, 50, (5, 2, 5)).astype(np.uint32)
    counts[2] = 0                      # a site nobody covered
    counts[4] = 2**32 - 1              # full-width counts: DP and AD are 64-bit sums
    path = tmp_path / "s.vcf"
    path.write_text("an older file\n")
    assert write_vcf(host_lib, sites, ref, alt, counts, names, lens, path) == "OK"
    text = path.read_text()
    assert text == _pileup.vcf_text(sites, ref, alt, counts, names, lens)
    meta, contigs, records = _pileup.parse_vcf(text)
    assert contigs == [("genome-a|chr1 first", 700), ("genome-a|lone", 1), ("b|z|3", 2**34)] and len(records) == 5
    assert records[2]["info"] == {"DP": 0, "AD": (0, 0), "ADF": (0, 0), "ADR": (0, 0), "OTH": 0}
    k = counts[0].astype(np.int64)
    assert records[0] == {"chrom": "genome-a|chr1 first", "pos": 1, "id": ".", "ref": "A", "alt": "C", "qual": ".", "filter": ".",
                          "info": {"DP": int(k.sum()), "AD": (int(k[:, 0].sum()), int(k[:, 1].sum())), "ADF": (int(k[0, 0]), int(k[0, 1])),
                                   "ADR": (int(k[1, 0]), int(k[1, 1])), "OTH": int(k[:, 2:].sum())}}
    assert records[4]["pos"] == 2**34 and records[4]["info"]["DP"] == 10 * (2**32 - 1) and records[4]["info"]["OTH"] == 6 * (2**32 - 1)
    # no sites: the header alone
    none = tuple(x[:0] for x in sites)
    assert write_vcf(host_lib, none, ref[:0], alt[:0], counts[:0], names, lens, path) == "OK"
    assert path.read_text() == _pileup.vcf_text(none, ref[:0], alt[:0], counts[:0], names, lens) and path.read_text().endswith(_pileup.COLUMNS + "\n")
    # a site that names a sequence the run does not have is refused
    sites[1][3] = 1
    assert write_vcf(host_lib, sites, ref, alt, counts, names, lens, path).startswith("ERR\t")
