"""BGZF framing on the device (simmr_bgzf_frame, include/simmr_hip.h) against tests/_bam.py's walker of blocks, zlib's CRC-32 and
the standard library's gzip reader: sizes on both sides of a lane's 16-byte load, of a lane's segment and of a block, random
bytes, zeros and 0xff, source pointers off their alignment, guard bytes around dst, and the refusals."""
import ctypes as C
import gzip
import re
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from simmr_amd.sam import BGZF_EOF
from tests import _bam

pytestmark = pytest.mark.gpu

_KERNELS = (Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc" / "bam_kernels.hip").read_text()
_DEFINES = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(BGZF_\w+)\s+(\d+)u?\b", _KERNELS, re.M)}
SEG, BLOCK = _DEFINES["BGZF_SEG"], _DEFINES["BGZF_BLOCK"]
SIZES = [0, 1, 3, 4, 5, 15, 16, 17, SEG - 1, SEG, SEG + 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 7]
LARGE = 41 * BLOCK + 12_345  # a few MB: more blocks than one, a short last one
CAN = 64


def fill(kind, n):
    if kind == "random":
        return np.random.default_rng(n + 1).integers(0, 256, n, dtype=np.uint8)
    return np.full(n, 0 if kind == "zeros" else 0xff, dtype=np.uint8)


def frame(engine, data, shift=0, capacity=None):
    """(status, written, the bytes between the guards, guards intact) for the raw call on `data` placed `shift` bytes into its buffer"""
    import torch
    n = len(data)
    src = torch.zeros(shift + n + 1, dtype=torch.uint8, device=engine.device)
    src[shift:shift + n] = torch.from_numpy(np.ascontiguousarray(data)).to(engine.device)
    bound = _bam.bgzf_bound(n)
    buf = torch.full((CAN + bound + CAN,), 0xA5, dtype=torch.uint8, device=engine.device)
    written = C.c_uint64(1 << 60)
    rc = engine.lib.simmr_bgzf_frame(engine._h, C.c_void_p(src.data_ptr() + shift), n, C.c_void_p(buf.data_ptr() + CAN),
                                     bound if capacity is None else capacity, C.byref(written))
    torch.cuda.synchronize()
    h = bytes(buf.cpu().numpy())
    guards = h[:CAN] == b"\xa5" * CAN and h[CAN + bound:] == b"\xa5" * CAN
    return rc, written.value, h[CAN:CAN + bound], guards


def check(engine, data, shift=0):
    rc, written, out, guards = frame(engine, data, shift)
    n = len(data)
    assert rc == 0 and guards and written == engine.lib.simmr_bgzf_bound(n) == _bam.bgzf_bound(n), (n, shift, rc, written)
    blocks = _bam.bgzf_blocks(out)  # every header field, BSIZE, LEN / ~LEN, ISIZE and the CRC against zlib's
    assert len(blocks) == -(-n // BLOCK) and b"".join(blocks) == bytes(data), (n, shift)
    assert out == _bam.bgzf_frame(bytes(data))
    assert gzip.decompress(out + BGZF_EOF) == bytes(data)


@pytest.mark.parametrize("kind", ["random", "zeros", "ff"])
def test_every_size(engine, kind):
    for n in SIZES:
        check(engine, fill(kind, n))


@pytest.mark.parametrize("kind", ["random", "zeros", "ff"])
def test_a_buffer_of_many_blocks(engine, kind):
    check(engine, fill(kind, LARGE))


@pytest.mark.parametrize("shift", [1, 3])
def test_a_source_off_its_alignment(engine, shift):
    for n in SIZES + [5 * BLOCK + 333]:
        check(engine, fill("random", n), shift)


def test_the_python_method_and_the_blocks_of_records(engine):
    import torch
    data = fill("random", 3 * BLOCK + 99)
    out = engine.bgzf(torch.from_numpy(data).to(engine.device))
    assert bytes(out.cpu().numpy()) == _bam.bgzf_frame(bytes(data))
    assert engine.bgzf(torch.zeros(0, dtype=torch.uint8, device=engine.device)).numel() == 0
    with pytest.raises(ValueError):
        engine.bgzf(torch.zeros(4, dtype=torch.int32, device=engine.device))


def test_refusals(engine):
    import torch
    lib = engine.lib
    data = fill("random", BLOCK + 10)
    bound = _bam.bgzf_bound(len(data))
    # ERANGE: one byte short, nothing written
    rc, written, out, guards = frame(engine, data, capacity=bound - 1)
    assert rc == _abi.ERANGE and written == 0 and guards and out == b"\xa5" * bound
    # nothing to frame: nothing written, whatever the pointers
    rc, written, out, guards = frame(engine, data[:0])
    assert (rc, written, guards) == (0, 0, True)
    w = C.c_uint64(7)
    assert lib.simmr_bgzf_frame(engine._h, None, 0, None, 0, C.byref(w)) == 0 and w.value == 0
    # EINVAL: a NULL buffer, no place for `written`, and overlapping buffers (dst inside src, src inside dst's blocks, dst's end on src's start)
    buf = torch.full((4 * bound,), 0xA5, dtype=torch.uint8, device=engine.device)
    p, n = buf.data_ptr(), len(data)
    assert lib.simmr_bgzf_frame(engine._h, None, n, C.c_void_p(p), bound, C.byref(w)) == _abi.EINVAL
    assert lib.simmr_bgzf_frame(engine._h, C.c_void_p(p), n, None, bound, C.byref(w)) == _abi.EINVAL
    assert lib.simmr_bgzf_frame(engine._h, C.c_void_p(p), n, C.c_void_p(p + 2 * bound), bound, None) == _abi.EINVAL
    for src, dst in ((p, p + n - 1), (p + bound - 1, p), (p, p), (p + 5, p)):
        assert lib.simmr_bgzf_frame(engine._h, C.c_void_p(src), n, C.c_void_p(dst), bound, C.byref(w)) == _abi.EINVAL, (src - p, dst - p)
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    # buffers that touch without overlapping are taken
    assert lib.simmr_bgzf_frame(engine._h, C.c_void_p(p), n, C.c_void_p(p + n), bound, C.byref(w)) == 0 and w.value == bound
    assert lib.simmr_bgzf_frame(engine._h, C.c_void_p(p + 2 * bound), n, C.c_void_p(p + bound), bound, C.byref(w)) == 0 and w.value == bound
