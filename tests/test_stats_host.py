"""CPU-only checks of the run-statistics surface: struct simmr_run_stats as gcc lays it out against _abi.RunStats, the
statistics TSV writer of libsimmr_host.so against the Python formatter (tests/_stats.py), --stats on the command line, and
the numpy model against a base-by-base loop, and where the cases of tests/_stats_cases.py land in that model."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import MinimalShortErrorProfile, _abi
from tests import _oracle, _stats, _synth, _truth

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"


@pytest.fixture(scope="module")
def host_lib():
    subprocess.check_call(["make", "-s", "-C", str(HOST)])
    lib = C.CDLL(str(HOST / "libsimmr_host.so"))
    lib.simmr_host_stats_tsv.restype = C.c_void_p
    lib.simmr_host_stats_tsv.argtypes = [C.POINTER(_abi.RunStats), C.c_char_p]
    lib.simmr_host_free.argtypes = [C.c_void_p]
    return lib


def test_run_stats_layout_matches_header():
    import tempfile
    fields = [n for n, _ in _abi.RunStats._fields_]
    assert fields == list(_stats.SHAPES)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "simmr_hip.h"\nint main(void){ printf("%zu", sizeof(simmr_run_stats));\n' + \
          "".join(f' printf(" %zu %zu", offsetof(simmr_run_stats, {f}), sizeof(((simmr_run_stats*)0)->{f}));\n' for f in fields) + \
          ' printf(" %u %u", SIMMR_STATS_CYCLES, SIMMR_STATS_NM_BINS); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "t.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/t", f"{d}/t.c"])
        got = list(map(int, subprocess.check_output([f"{d}/t"]).decode().split()))
    T = _abi.RunStats
    want = [C.sizeof(T)]
    for f in fields:
        want += [getattr(T, f).offset, getattr(T, f).size]
        assert np.ctypeslib.as_array(getattr(T(), f)).shape == _stats.SHAPES[f], f
        assert getattr(T, f).size == 8 * int(np.prod(_stats.SHAPES[f])), f
    assert got == want + [_abi.STATS_CYCLES, _abi.STATS_NM_BINS] and (_abi.STATS_CYCLES, _abi.STATS_NM_BINS) == (_stats.CYCLES, _stats.NM_BINS)
    for name in ("simmr_stats_reset", "simmr_stats_add", "simmr_stats_read", "simmr_last_stats_ms"):
        assert name in _abi.SYMBOLS and hasattr(_abi.load(), name)


def host_tsv(lib, s, path):
    st = _abi.RunStats()
    for k in _stats.SHAPES:
        np.ctypeslib.as_array(getattr(st, k))[...] = s[k]
    p = lib.simmr_host_stats_tsv(C.byref(st), str(path).encode())
    msg = C.string_at(p).decode()
    lib.simmr_host_free(p)
    assert msg == "OK", msg
    return Path(path).read_text()


def test_stats_tsv_writer_equals_the_python_formatter(host_lib, tmp_path):
    rng = np.random.default_rng(7)
    s = {k: (rng.integers(0, 1 << 62, shape, dtype=np.uint64) * (rng.random(shape) < 0.3)).astype(np.uint64) for k, shape in _stats.SHAPES.items()}
    s["reads"][:] = [5, 0]
    s["pair"][4, 4] = np.uint64((1 << 64) - 1)
    assert all((v == 0).any() and (v != 0).any() for v in s.values())
    text = host_tsv(host_lib, s, tmp_path / "s.tsv")
    assert text == _stats.tsv(s)
    lines = text.splitlines()
    assert lines[0] == "table\tset\ti\tj\tcount" and lines[1] == "reads\t0\t-\t-\t5" and "pair\t-\t4\t4\t18446744073709551615" in lines
    assert len(lines) == 1 + sum(int(np.count_nonzero(v)) for v in s.values())
    assert [l.split("\t")[0] for l in lines[1:]] == sorted((l.split("\t")[0] for l in lines[1:]), key=list(_stats.SHAPES).index)
    # the file is replaced, not appended to; all-zero tables are the header alone
    assert host_tsv(host_lib, _stats.zeros(), tmp_path / "s.tsv") == "table\tset\ti\tj\tcount\n"


def test_stats_is_in_the_cli_surface(host_lib):
    exe = HOST / "simmr-hip"
    helptext = subprocess.check_output([str(exe), "--help"]).decode()
    assert "--stats <FILE>" in helptext
    r = subprocess.run([str(exe), "--stats"], capture_output=True)
    assert r.returncode == 2 and b"--stats" in r.stderr


def test_stats_with_devices_is_refused_before_any_device(host_lib):
    r = subprocess.run([str(HOST / "simmr-hip"), "--genome", "x.fa", "--output", "x.fq", "--stats", "s.tsv", "--devices", "0,0"],
                       capture_output=True)
    assert r.returncode != 0 and b"--stats does not combine with --devices" in r.stderr


def test_model_equals_a_base_by_base_loop(oracle):
    """tests/_stats.model is vectorised; the same definitions read off one base at a time give the same tables"""
    g = _oracle.HostGenome(_synth.synthetic_contigs([20_000, 7_001], 3))
    prof = MinimalShortErrorProfile(mean_phred_score=9, rng_mode=_abi.RNG_PHILOX).pod()
    o = _oracle.simulate_pe(oracle, g, prof, 300, 5, qual_offset=33).trimmed()
    o = dict(o, genome=np.full(len(o["start"]), 2, dtype=np.uint32))
    o["seq"] = o["seq"].copy()
    o["seq"][[3, 700, 701]] = [ord("N"), ord("-"), ord("a")]
    comp = _truth.complement_lut(oracle)
    s = _stats.zeros()
    for r in range(len(o["start"])):
        a, b = int(o["start"][r]), int(o["end"][r])
        lo, L, m = min(a, b), abs(b - a), r % 2
        want = g.contigs[int(o["contig"][r])][lo:lo + L]
        if o["flags"][r] & 1:
            want = comp[want[::-1]]
        first = int(o["seq_off"][r])
        nm = gc = 0
        for j in range(L):
            x, q = int(o["seq"][first + j]), (int(o["qual"][first + j]) - 33) & 255
            e, w = (b"ACGT".find(bytes([int(want[j])])) % 5 if bytes([int(want[j])]) in b"ACGT" else 4), (b"ACGT".find(bytes([x])) if bytes([x]) in b"ACGT" else 4)
            edit = x != int(want[j])
            s["qual_n"][q] += 1; s["qual_mismatch"][q] += edit; s["pair"][e, w] += 1
            nm += edit; gc += x in b"GC"
            if j < 512:
                s["cycle_n"][m, j] += 1; s["cycle_qsum"][m, j] += q; s["cycle_mismatch"][m, j] += edit; s["cycle_base"][m, j, w] += 1
        s["reads"][m] += 1; s["bases"][m] += L; s["nm_hist"][min(nm, 63)] += 1
        if L:
            s["gc_hist"][100 * gc // L] += 1
    got = _stats.model(oracle, o, {2: g}, 2, 33)
    _stats.assert_stats(got, s, "model")
    assert got["pair"][:, 4].sum() == 3 and got["qual_mismatch"].sum() == _truth.model(oracle, o, {2: g})["nm"].sum()


# ---- the cases of tests/test_gpu_stats_seams.py land where their builders say ----------------------------------------------------
def test_constants_parse():
    c = _stats.constants()
    assert list(c) == list(_stats.CONSTANTS) and all(isinstance(v, int) and v > 0 for v in c.values())
    assert c["STATS_LANES"] * c["STATS_WG_READS"] == 256 and c["STATS_MAX_L"] == 65535 and c["STATS_FLUSH_BATCHES"] * 4 < 65536
    assert c["STATS_CYC_STRIDE"] == _stats.CYCLES + 16


@pytest.mark.parametrize("n_sets", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 4])
def test_tiled_unit_scales_the_model_of_one_batch(oracle, k, n_sets):
    """what licenses the scaled expectation of the flush case: tests/_stats.model of the unit laid out k times in full is the
    unit's model times k, table for table; and the columns built with torch are the tiled ones"""
    from tests import _stats_cases as cases
    genomes = cases.host_genomes()
    unit = cases.uniform_unit(oracle, genomes)
    host = cases.tiled(unit, k)
    assert len(host["start"]) == cases.WG_READS * k and int(host["seq_off"][-1]) == 40 * k == host["seq"].size
    one = _stats.model(oracle, unit, genomes, n_sets, cases.QUAL_OFFSET)
    _stats.assert_stats(_stats.model(oracle, host, genomes, n_sets, cases.QUAL_OFFSET), cases.scaled(one, k), f"{k} batches")
    assert all(v.dtype == np.uint64 for v in cases.scaled(one, k).values())
    dev = cases.device_tiled(unit, k, "cpu")
    h = dev.to_host()
    assert dev.n_reads == cases.WG_READS * k and dev.seq.numel() == dev.total_bases == 40 * k
    for name, col in host.items():
        assert np.array_equal(h[name], col) and h[name].dtype == col.dtype, name
    part = cases.first_reads(dev, cases.WG_READS).to_host()
    for name, col in unit.items():
        assert np.array_equal(part[name][:col.size], col), name


@pytest.mark.parametrize("cus", [256, 64, 32])
def test_flush_case_sends_workgroups_past_the_flush(cus):
    from tests import _stats_cases as cases
    n_batches = cases.FLUSH_BATCHES * cases.WGS_PER_CU * cus + 3
    assert math.ceil(n_batches / min(n_batches, cases.WGS_PER_CU * cus)) == cases.FLUSH_BATCHES + 1 == 4097
    assert math.ceil(cases.FLUSH_BATCHES / min(cases.FLUSH_BATCHES, cases.WGS_PER_CU * cus)) <= cases.FLUSH_BATCHES  # the run without one
    assert cases.WG_READS * n_batches < 1 << 31                                                       # read_id is 32 bits wide


def test_homopolymer_reads_land(oracle):
    from tests import _stats_cases as cases
    genomes = cases.host_genomes()
    case = cases.homopolymer_reads(oracle, genomes)
    m = _stats.model(oracle, case.host, genomes, 1, cases.QUAL_OFFSET)
    assert [int(m["pair"][c, c]) for c in range(5)] == 4 * [2 * cases.MAX_L] + [0]  # (the reverse read of A is all T: it lands on T)
    off = m["pair"].copy()
    off[np.arange(4), np.arange(4)] = 0
    want_off = case.all_edit.copy()
    want_off[3, 4] = want_off[1, 2] = cases.MAX_L                                   # the N read on T, the G read on C
    assert np.array_equal(off, want_off) and case.all_edit.sum() == cases.MAX_L and case.all_edit[0, 1:4].tolist() == 3 * [21845]
    assert m["nm_hist"][63] == 3 and m["nm_hist"][0] == 8 and m["nm_hist"].sum() == 11   # the all-edit read, and the N and the G read
    assert m["gc_hist"][100] == 1 + 4 and m["gc_hist"][0] == 1 + 4 and m["gc_hist"][66] == 1  # G on C and the C / G reads; N and the A / T reads; C, G of C, G, T
    assert m["reads"].tolist() == [11, 0] and m["bases"][0] == 11 * cases.MAX_L == m["qual_n"].sum() and (m["cycle_n"][0] == 11).all()
    assert m["cycle_base"][0, :, 4].tolist() == 512 * [1] and m["qual_mismatch"].sum() == 3 * cases.MAX_L
    L = np.diff(case.too_long["seq_off"].astype(np.int64))
    assert L.tolist() == [40, cases.MAX_L + 1, 33] and _truth.model(oracle, case.too_long, genomes)["nm"].tolist() == case.nm
    assert np.diff(case.good["seq_off"].astype(np.int64)).tolist() == [40, 33]
    assert _stats.model(oracle, case.good, genomes, 1, cases.QUAL_OFFSET)["nm_hist"][[1, 3]].tolist() == [1, 1]


def test_quality_range_fills_every_bin(oracle):
    from tests import _stats_cases as cases
    genomes = cases.host_genomes()
    host = cases.quality_range(oracle, genomes)
    assert sorted(set(np.diff(host["seq_off"].astype(np.int64)).tolist())) == [16, 17, 256, 512, 513]
    for qual_offset in (33, 0):
        m = _stats.model(oracle, host, genomes, 2, qual_offset)
        assert (m["qual_n"] > 0).all() and m["qual_n"].sum() == host["qual"].size
        low, high = (32 - qual_offset) & 255, (255 - qual_offset) & 255
        assert m["qual_mismatch"][low] >= 4 and m["qual_mismatch"][high] >= 4 and 255 in (low, high)
        for s, byte in ((0, 255), (1, 32)):  # forward reads are set 0 and hold 255 at the edge cycles, reverse ones set 1 and 32
            q = (byte - qual_offset) & 255
            for j in cases.EDGE_CYCLES:
                n = int(m["cycle_n"][s, j])
                assert n == {0: 5, 255: 3, 256: 2, 511: 2}[j] and m["cycle_qsum"][s, j] == n * q, (s, j)
