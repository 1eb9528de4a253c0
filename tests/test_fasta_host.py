"""The host layer's FASTA normalisation and loader (simmr_amd/host: the CLI's --host-normalize path) against the table and the
layout of tests/_fasta.py, which the device's staging is held to in tests/test_gpu_fasta.py — CPU only."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _fasta

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-s", "-C", str(HOST), "libsimmr_host.so"])
    lib = C.CDLL(str(HOST / "libsimmr_host.so"))
    lib.simmr_host_normalize.restype = C.c_void_p
    lib.simmr_host_normalize.argtypes = [C.c_char_p, C.c_uint64]
    lib.simmr_host_load_fasta.restype = C.c_void_p
    lib.simmr_host_load_fasta.argtypes = [C.c_char_p, C.c_int]
    lib.simmr_host_free.argtypes = [C.c_void_p]
    return lib


def host_normalize(lib, raw: bytes, n_expected: int) -> bytes:
    """the result read by its expected length and the byte behind it (a NUL in the result would cut string_at short)"""
    p = lib.simmr_host_normalize(raw, len(raw))
    try:
        got = C.string_at(p, n_expected + 1)
    finally:
        lib.simmr_host_free(p)
    assert got[-1] == 0, "the result is longer than the table says"
    return got[:-1]


def test_host_normalize_every_byte_value(host):
    for v in range(256):
        for raw in (bytes([v]), b"a" + bytes([v]) * 3 + b"T"):
            want = _fasta.normalize(raw).tobytes()
            assert host_normalize(host, raw, len(want)) == want, (v, raw)
    every = bytes(range(256)) * 2
    want = _fasta.normalize(every).tobytes()
    assert len(want) == 2 * 252 and host_normalize(host, every, len(want)) == want


@pytest.mark.parametrize("contiguous", [False, True])
def test_host_load_fasta_equals_layout(host, tmp_path, contiguous):
    rng = np.random.default_rng(31)
    records = [  # (header line with its line end, body up to the next header)
        (b">lead\n", b""),                                           # a leading empty record
        (b">crlf one two\r\n", _fasta.wrap(_fasta.bases(rng, 200), 60, b"\r\n")),
        (b">e1\n", b""), (b">e2\r\n", b""),                          # two adjacent empty records
        (b">mixed\n", _fasta.text(rng, 999) + b"\n"),
        (b">blank\n", b"\n\r\n \t\n\n"),                             # nothing but blank lines
        (b">bytes\n", b"AC>GT;01\x00\xff\x80acgu\n"),                # '>' inside a line belongs to the body
        (b">t\n", b""),                                              # a trailing empty record ...
    ]
    for last in (None, (b">last\n", b"ACGTNN--\nacg")):              # ... and then a last line without a line end
        recs = records + ([last] if last else [])
        path = tmp_path / f"f{len(recs)}.fna"
        path.write_bytes(b"".join(h + b for h, b in recs))
        want = _fasta.layout([b for _, b in recs], contiguous, 0)
        p = host.simmr_host_load_fasta(str(path).encode(), 1 if contiguous else 0)
        try:
            out = C.string_at(p)
        finally:
            host.simmr_host_free(p)
        lines = out.split(b"\n")
        assert lines[-1] == b"" and not out.startswith(b"ERR")
        # the loader applies no size filter (main.rs:117-162 does, later): every record is a sequence
        seqs = want.contigs if contiguous else [_fasta.normalize(b) for _, b in recs]
        sizes = want.sizes if contiguous else want.counts
        ids = [b"whole genome"] if contiguous else [h[1:].rstrip(b"\r\n") for h, _ in recs]
        assert lines[0] == b"%d\t%d" % (len(seqs), sum(want.counts))
        assert len(lines) == len(seqs) + 2
        for line, sid, size, seq in zip(lines[1:], ids, sizes, seqs):
            assert line == b"%s\t%d\t%d\t%s" % (sid, size, seq.size, seq.tobytes()), sid
