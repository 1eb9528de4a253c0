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
