"""bench.py --dump-outputs on CPU tensors: the sample of a shard larger than the dump limits, in both layouts of the
columns (compact, and the 16-byte read slots of SIMMR_SLOT16), is what Reads.to_host() hands a caller."""
import numpy as np
import pytest
import torch

import bench
from simmr_amd.engine import Reads


def _shard(n, slot16, seed=3):
    """n reads of random lengths with random bytes in seq / qual, laid out compact or in 16-byte slots; returns the
    Reads (CPU tensors) and what to_host() gives for them"""
    g = np.random.default_rng(seed)
    L = g.integers(0, 40, n)
    if slot16:  # seq at a slot's start + (r % 16), qual at the slot's start
        lead = np.arange(n) % 16
        size = (L + lead + 15) // 16 * 16
        slot = np.concatenate([[0], np.cumsum(size)])
        first = slot[:n] + lead
        tb = int(slot[n])
    else:
        slot = np.concatenate([[0], np.cumsum(L)])
        first = slot[:n]
        tb = int(slot[n])
    r = Reads.allocate(n, tb, "cpu", 33, 16 if slot16 else 0)
    seq, qual = g.integers(0, 256, tb).astype(np.uint8), g.integers(0, 256, tb).astype(np.uint8)
    r.seq[:tb], r.qual[:tb] = torch.from_numpy(seq), torch.from_numpy(qual)
    start = g.integers(0, 10**6, n)
    end = np.where(np.arange(n) % 2 == 1, start - L, start + L)  # mates read backwards: |end - start| = L
    r.seq_off[:n] = torch.from_numpy(first)
    if not slot16:
        r.seq_off[n] = tb
    r.start[:], r.end[:] = torch.from_numpy(start), torch.from_numpy(end)
    for col in ("contig", "genome", "read_id"):
        getattr(r, col)[:] = torch.from_numpy(g.integers(0, 1000, n).astype(np.int32))
    r.flags[:] = torch.from_numpy(g.integers(0, 256, n).astype(np.uint8))
    return r, r.to_host()


@pytest.mark.parametrize("slot16", [False, True], ids=["compact", "slot16"])
def test_dump_is_a_sample_of_what_to_host_gives(tmp_path, monkeypatch, slot16):
    monkeypatch.setattr(bench, "DUMP_READS", 500)
    monkeypatch.setattr(bench, "DUMP_BYTES", 3000)
    reads, h = _shard(4000, slot16)
    bench.dump_outputs(str(tmp_path), "", torch.arange(8, dtype=torch.int64), reads=reads)
    d = {p.stem: np.load(p) for p in tmp_path.iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert np.array_equal(d["counters"], np.arange(8))
    ri, bi = d["read_index"].astype(np.int64), d["base_index"].astype(np.int64)
    assert ri.size == 500 and np.unique(ri).size == 500 and bi.size == 3000 and np.unique(bi).size == 3000
    for col in ("start", "end", "contig", "genome", "flags"):
        assert np.array_equal(d["read_" + col], h[col][ri].astype(np.float64)), col
    assert np.array_equal(d["read_id"], h["read_id"][ri].astype(np.float64))
    assert np.array_equal(d["read_seq_off"], h["seq_off"][ri].astype(np.float64))
    assert np.array_equal(d["read_length"], np.diff(h["seq_off"].astype(np.int64))[ri])
    assert np.array_equal(d["seq"], h["seq"][bi].astype(np.float32))
    assert np.array_equal(d["qual"], h["qual"][bi].astype(np.float32))


def test_dump_sample_depends_on_the_sizes_only():
    a, b = bench._sample(10**9, 1000, 1), bench._sample(10**9, 1000, 1)
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0) and a[-1] < 10**9
    assert np.array_equal(bench._sample(77, 1000, 1), np.arange(77))


def test_dump_of_fastq_text(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 100)
    text = torch.from_numpy(np.frombuffer(b"@r0\nACGT\n+\nIIII\n" * 50, dtype=np.uint8).copy())
    bench.dump_outputs(str(tmp_path), "rank1_", torch.zeros(8, dtype=torch.int64), text=text)
    idx = np.load(tmp_path / "rank1_text_index.npy").astype(np.int64)
    assert np.load(tmp_path / "rank1_text_bytes.npy")[0] == text.numel() and idx.size == 100
    assert np.array_equal(np.load(tmp_path / "rank1_text.npy"), text.numpy()[idx].astype(np.float32))
