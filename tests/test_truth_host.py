"""CPU-only checks of the ground-truth surface: the struct simmr_truth_out as gcc lays it out, the truth TSV writer of
libsimmr_host.so against a Python formatter, --truth on the command line, and where the GPU test's loop premise comes from."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import MinimalLongErrorProfile, MinimalShortErrorProfile, _abi
from tests import _oracle, _synth, _truth

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"
HEADER = "read_id\tpair\tgenome_id\tsequence_id\tstart\tend\tstrand\tlength\tNM\tedits\n"


@pytest.fixture(scope="module")
def host_lib():
    subprocess.check_call(["make", "-s", "-C", str(HOST)])
    lib = C.CDLL(str(HOST / "libsimmr_host.so"))
    lib.simmr_host_truth_tsv.restype = C.c_void_p
    lib.simmr_host_truth_tsv.argtypes = [C.c_uint64, C.c_int] + [C.c_void_p] * 12 + [C.c_uint32, C.c_uint32, C.POINTER(C.c_char_p),
                                                                                       C.POINTER(C.c_uint32), C.POINTER(C.c_char_p), C.c_int, C.c_char_p]
    lib.simmr_host_free.argtypes = [C.c_void_p]
    return lib


def test_truth_out_layout_matches_header():
    import tempfile
    fields = ("nm", "edit_off", "edit_pos", "edit_ref", "edit_alt", "edit_qual", "reads_capacity", "edits_capacity")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "simmr_hip.h"\nint main(void){ printf("%zu", sizeof(simmr_truth_out));\n' + \
          "".join(f' printf(" %zu", offsetof(simmr_truth_out, {f}));\n' for f in fields) + " return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "t.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/t", f"{d}/t.c"])
        got = list(map(int, subprocess.check_output([f"{d}/t"]).decode().split()))
    T = _abi.TruthOut
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    assert [n for n, _ in T._fields_] == list(fields)
    for name in ("simmr_truth_plan", "simmr_truth_emit", "simmr_last_truth_ms"):
        assert name in _abi.SYMBOLS and hasattr(_abi.load(), name)


def python_tsv(o, t, paired, names, qual_offset=33):
    lines = []
    for r in range(len(o["start"])):
        gid, sids = names[int(o["genome"][r])]
        a, b = int(o["start"][r]), int(o["end"][r])
        lines.append("\t".join([str(int(o["read_id"][r])), str((r & 1) + 1 if paired else 0), gid, sids[int(o["contig"][r])], str(a), str(b),
                                "-" if o["flags"][r] & _abi.FLAG_REVCOMP else "+", str(abs(b - a)), str(int(t["nm"][r])),
                                _truth.edits_text(t, r, qual_offset)]) + "\n")
    return "".join(lines)


def host_tsv(lib, o, t, paired, names, path, header, qual_offset=33):
    n = len(o["start"])
    cols = [np.ascontiguousarray(o[k], dtype=dt) for k, dt in (("read_id", np.uint32), ("genome", np.uint32), ("contig", np.uint32),
                                                              ("start", np.uint64), ("end", np.uint64), ("flags", np.uint8))]
    cols += [np.ascontiguousarray(t[k], dtype=dt) for k, dt in (("nm", np.uint32), ("edit_off", np.uint64), ("edit_pos", np.uint32),
                                                              ("edit_ref", np.uint8), ("edit_alt", np.uint8), ("edit_qual", np.uint8))]
    cols = [c if c.size else np.zeros(1, dtype=c.dtype) for c in cols]
    ng = max(names) + 1
    gids = (C.c_char_p * ng)(*[names.get(g, ("-", []))[0].encode() for g in range(ng)])
    ncs = (C.c_uint32 * ng)(*[len(names.get(g, ("-", []))[1]) for g in range(ng)])
    flat = [s.encode() for g in range(ng) for s in names.get(g, ("-", []))[1]]
    sids = (C.c_char_p * max(len(flat), 1))(*flat)
    p = lib.simmr_host_truth_tsv(n, 1 if paired else 0, *[c.ctypes.data for c in cols], qual_offset, ng, gids, ncs, sids, 1 if header else 0,
                                 str(path).encode())
    msg = C.string_at(p).decode()
    lib.simmr_host_free(p)
    assert msg == "OK", msg


def test_truth_tsv_writer_equals_the_python_formatter(host_lib, oracle, tmp_path):
    contigs = _synth.synthetic_contigs([40_000, 33_333], 3)
    g = _oracle.HostGenome(contigs)
    names = {2: ("genome two", ["first sequence", "s2 with spaces"])}
    # paired reads with errors: the model's edits of the oracle's reads
    prof = MinimalShortErrorProfile(mean_phred_score=24, rng_mode=_abi.RNG_PHILOX).pod()
    o = _oracle.simulate_pe(oracle, g, prof, 600, 5, read_id_base=1000, qual_offset=33).trimmed()
    o = dict(o, genome=np.full(len(o["start"]), 2, dtype=np.uint32))
    t = _truth.model(oracle, o, {2: g})
    assert (t["nm"] == 0).any() and (t["nm"] > 1).any() and (o["flags"] & 1).any()
    out = tmp_path / "pairs.tsv"
    host_tsv(host_lib, o, t, True, names, out, True)
    assert out.read_text() == HEADER + python_tsv(o, t, True, names)
    host_tsv(host_lib, o, t, True, names, out, False)  # appends, without a second header
    assert out.read_text() == HEADER + 2 * python_tsv(o, t, True, names)
    # long reads: pair 0
    lp = MinimalLongErrorProfile(gamma_mean=3000.0, gamma_std=2500.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    ol = _oracle.simulate_long(oracle, [g], [40], lp, 3, qual_offset=33).trimmed()
    ol = dict(ol, genome=np.full(len(ol["start"]), 2, dtype=np.uint32))
    tl = _truth.model(oracle, ol, {2: g})
    outl = tmp_path / "long.tsv"
    host_tsv(host_lib, ol, tl, False, names, outl, True)
    text = outl.read_text()
    assert text == HEADER + python_tsv(ol, tl, False, names)
    assert all(line.split("\t")[1] == "0" for line in text.splitlines()[1:])
    # a read without an edit is `*`
    z = {k: (np.zeros_like(v) if k in ("nm", "edit_off") else v[:0]) for k, v in t.items()}
    outz = tmp_path / "none.tsv"
    host_tsv(host_lib, o, z, True, names, outz, False)
    assert all(line.endswith("\t0\t*") for line in outz.read_text().splitlines())


def test_truth_is_in_the_cli_surface(host_lib):
    exe = HOST / "simmr-hip"
    helptext = subprocess.check_output([str(exe), "--help"]).decode()
    assert "--truth <FILE>" in helptext
    r = subprocess.run([str(exe), "--truth"], capture_output=True)
    assert r.returncode == 2 and b"--truth" in r.stderr
    # refused together with --devices before any device is touched
    r = subprocess.run([str(exe), "--genome", "x.fa", "--output", "x.fq", "--truth", "t.tsv", "--devices", "0,0"], capture_output=True)
    assert r.returncode == 1 and b"--truth does not combine with --devices" in r.stderr


def test_gpu_truth_test_is_sized_from_the_kernels_constants():
    """tests/test_gpu_truth.py::test_seq_past_4_gib_and_workgroups_loop asserts that workgroups of k_truth loop; the constants
    it computes that from are the kernel file's."""
    import re
    k = (ROOT / "simmr_amd" / "csrc" / "truth_kernels.hip").read_text()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(TRUTH_\w+)\s+(\d+)u?\b", k, re.M)}
    from tests import test_gpu_truth
    assert defines["TRUTH_WG_READS"] == test_gpu_truth.TRUTH_WG_READS
    assert defines["TRUTH_WGS_PER_CU"] == test_gpu_truth.TRUTH_WGS_PER_CU
    assert defines["TRUTH_LANES"] * defines["TRUTH_WG_READS"] == 256  # one workgroup: a row of lanes per read


# ---- the builders of tests/_truth_cases.py, which tests/test_gpu_truth_seams.py runs through the pass -------------------------------
def test_seam_cases_are_sized_from_the_sources():
    """tests/_truth_cases.py reads its constants out of truth_kernels.hip and kernels.hip; the geometry it derives from them is the
    geometry the sources use them for."""
    from tests import _truth_cases as tc
    csrc = ROOT / "simmr_amd" / "csrc"
    kern, scan, eng, host = ((csrc / f).read_text() for f in ("truth_kernels.hip", "kernels.hip", "engine.hip", "truth_host.hpp"))
    K = tc.constants()
    assert tuple(K) == tc.CONSTANTS and (tc.LANES, tc.WG_READS, tc.WGS_PER_CU, tc.SCAN_THREADS, tc.SCAN_ITEMS) == tuple(K.values())
    assert K["TRUTH_LANES"] * K["TRUTH_WG_READS"] == 256 and "__launch_bounds__(256)\nk_truth(" in kern
    # a lane's window is 16 bases, a round TRUTH_LANES of them; workgroups step by the grid, which row_grid caps
    assert "g0 += TRUTH_LANES" in kern and "(L + 15u) >> 4" in kern and tc.GROUP == 16 and tc.ROUND == 16 * K["TRUTH_LANES"] == 256
    assert "batch += gridDim.x" in kern and "batch * TRUTH_WG_READS + row" in kern
    assert "(n_reads + TRUTH_WG_READS - 1) / TRUTH_WG_READS" in host and "(uint64_t)eng_cu_count(e) * wgs_per_cu" in host
    assert "row_grid(e, n_reads, TRUTH_WGS_PER_CU)" in (csrc / "truth.hip").read_text()
    # the scan: SCAN_THREADS * SCAN_ITEMS counts a workgroup, SCAN_THREADS of their sums per trip of k_scan_tops
    assert "per_wg = SCAN_THREADS * SCAN_ITEMS" in eng and "base < n_wg; base += SCAN_THREADS" in scan
    assert tc.SCAN_TILE == K["SCAN_THREADS"] * K["SCAN_ITEMS"]
    for cus in (1, 64, 256, 304):
        n = tc.tiny_n(cus)
        for m, last in ((n, 5), (n - 5, tc.WG_READS)):
            s = tc.tiny_shape(m, cus)
            assert s.trips >= 3 and (s.trips == 3) == (cus >= 256) and s.last == last and s.batches - 1 >= 2 * s.grid and s.scan_tiles > K["SCAN_THREADS"] + 1


def test_dense_reads_are_all_edits(oracle):
    from tests import _truth_cases as tc
    genomes = tc.host_genomes()
    case = tc.dense_reads(oracle)
    m = _truth.model(oracle, case.host, genomes)
    off = m["edit_off"].astype(np.int64)
    seen = []
    for r, kind in enumerate(case.kinds):
        pos = m["edit_pos"][off[r]:off[r + 1]]
        if kind == "dense":
            assert m["nm"][r] == case.L[r] and np.array_equal(pos, np.arange(case.L[r]))
            assert np.array_equal(m["edit_qual"][off[r]:off[r + 1]], tc.qual_of(case.L[r], r))
            if case.L[r] >= 33:
                assert np.unique(m["edit_alt"][off[r]:off[r + 1]]).size >= 5   # three steps, N and lower case
            seen.append((int(case.L[r]), int(case.host["flags"][r])))
        else:
            assert pos.tolist() == ([] if kind == "clean" else [0])
    assert sorted(set(seen)) == sorted((L, rev) for L in tc.DENSE_LENGTHS for rev in (0, 1))
    assert case.kinds[::3] == len(case.kinds) // 3 * ["dense"] and int(m["nm"].max()) == 65535
    assert {int(g) for g, k in zip(case.host["genome"], case.kinds) if k == "dense"} == {tc.BIG, tc.RANDOM, tc.HOMOPOLYMER}
    # stepped_each is tests/_stats_cases.stepped over arrays
    want = np.frombuffer(b"ACGTTGCA", dtype=np.uint8)
    steps = np.array([1, 2, 3, 1, 2, 3, 1, 2])
    assert tc.stepped_each(want, steps).tolist() == [tc.sc.stepped(b, s) for b, s in zip(want, steps)]


def test_overlap_reads_edit_exactly_the_overlapped_bytes(oracle):
    from tests import _truth_cases as tc
    case = tc.overlap_reads(oracle)
    m = _truth.model(oracle, case.host, tc.host_genomes())
    off = m["edit_off"].astype(np.int64)
    L = np.diff(case.host["seq_off"].astype(np.int64))
    assert sorted(set(L.tolist())) == list(tc.OVERLAP_LENGTHS) == [17, 18, 31, 33, 47, 255, 257, 513]
    for r, at in enumerate(case.at):
        assert np.array_equal(m["edit_pos"][off[r]:off[r + 1]], at), r
        owned = 16 * (L[r] // 16)
        pattern = "abc"[r % 3]
        lo, hi = {"a": (L[r] - 16, owned), "b": (owned, L[r]), "c": (L[r] - 16, L[r])}[pattern]
        assert at.tolist() == list(range(lo, hi)) and at.size == {"a": 16 - L[r] % 16, "b": L[r] % 16, "c": 16}[pattern]
    assert set(zip(L.tolist(), case.host["flags"].tolist())) == {(n, rev) for n in tc.OVERLAP_LENGTHS for rev in (0, 1)}


def test_long_reads_pass_65535_with_a_dense_stretch(oracle):
    from tests import _truth_cases as tc
    case = tc.long_reads(oracle)
    m = _truth.model(oracle, case.host, tc.host_genomes())
    off = m["edit_off"].astype(np.int64)
    L = np.diff(case.host["seq_off"].astype(np.int64))
    assert L.tolist() == [65536, 65536, 65537, 65537, 70000, 70000] and case.host["flags"].tolist() == [0, 1, 0, 1, 0, 1]
    assert (case.host["contig"] == tc.LONG_CONTIG).all() and (np.maximum(case.host["start"], case.host["end"]) <= 70000).all()
    for r, at in enumerate(case.at):
        pos = m["edit_pos"][off[r]:off[r + 1]].astype(np.int64)
        assert np.array_equal(pos, at) and 65535 in pos and np.isin(np.arange(0, L[r], 251), pos).all()
        b = min(L[r], 65700)
        run = pos[(pos >= b - 300) & (pos < b)]
        assert np.array_equal(run, np.arange(b - 300, b)) and run[0] < 65535 <= run[-1]  # 300 edits in a row over 65 535
        assert any(run[0] < e <= run[-1] for e in range(256, L[r], 256))       # ... with the start of a round inside
        assert (pos > 65535).any() == (L[r] > 65536)
    assert int(m["edit_pos"].max()) == 69999


def test_the_assembler_of_the_tiny_reads_is_the_model(oracle):
    """tests/_truth_cases.assembled puts the expectation of the grid case together from the models of four 16-read units; here it is
    held to tests/_truth.model run over every read of the tiled host columns, with a partial and with a whole last batch."""
    from tests import _truth_cases as tc
    genomes = tc.host_genomes()
    units = tc.tiny_units(oracle)
    models = [_truth.model(oracle, u, genomes) for u in units]
    assert len({int(m["nm"].sum()) for m in models}) == len(units) == 4 and not models[0]["nm"].any()
    k = 301
    order = tc.unit_order(k, len(units))
    assert set(order.tolist()) == {0, 1, 2, 3}
    for cus in (64, 256, 304):  # a batch, or a trip of the grid, later is another unit more often than not
        long_order = tc.unit_order(3 * cus * tc.WGS_PER_CU, len(units))
        for shift in (1, cus * tc.WGS_PER_CU, 2 * cus * tc.WGS_PER_CU):
            assert (long_order[shift:] != long_order[:-shift]).mean() > 0.5
    for n in (k * 16 - 11, k * 16 - 16 + 1, k * 16):
        host = tc.host_sequenced(units, order, n)
        assert len(host["start"]) == n and host["seq"].size == int(host["seq_off"][n])
        want = _truth.model(oracle, host, genomes)
        _truth.assert_truth(tc.assembled(models, order, n), want, f"{n} tiny reads")
        assert want["nm"].sum() > 0


def test_small_reads_hold_what_they_say(oracle):
    from tests import _truth_cases as tc
    genomes = tc.host_genomes()
    case = tc.small_reads(oracle)
    m = _truth.model(oracle, case.host, genomes)
    assert m["nm"].tolist() == case.planned
    h = case.host
    assert int(h["end"][3]) == int(h["start"][6]) == case.clen and h["flags"][3] == 0 and h["flags"][6] == 1
    assert int(h["start"][4]) == int(h["end"][4]) == case.clen and h["seq_off"][4] == h["seq_off"][5]
    assert tc.UNSTAGED not in genomes and case.clen == genomes[tc.RANDOM].contigs[tc.EDGE_CONTIG].size
