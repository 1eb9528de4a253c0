"""Hand-built read columns for the passes that walk reads against the staged genomes (tests/test_gpu_stats.py,
tests/test_gpu_truth.py): the smallest shapes at which that walk can go wrong."""
import numpy as np

from simmr_amd.engine import Reads
from tests import _truth


def hand_built(oracle, genomes, layout, device, rng, spoil=None):
    """Reads whose bytes are copied from the host genomes, with chosen offsets altered: returns the device columns in
    `layout` and the same reads as compact host columns for the model."""
    import torch
    comp = _truth.complement_lut(oracle)
    clen1 = [c.size for c in genomes[1].contigs]
    specs = []  # genome, contig, lo, L, reverse, offsets to alter (or "gc")
    for i, L in enumerate((0, 1, 15, 16, 17, 511, 512, 513)):
        for rev in (0, 1):
            specs.append((3, 0, 11_900 + 37 * i, L, rev, [0, L // 2, L - 1] if L > 2 and i % 2 else []))
            specs.append((1, i % 5, 1000 + 2099 * i + rev, L, rev, [L - 1] if L else []))
    specs.append((1, 3, 5000, 513, 0, list(range(3, 513, 7))))     # 73 edits: the last nm_hist bin
    specs.append((1, 3, 9000, 300, 1, list(range(0, 300, 4))))     # 75 edits, reverse
    specs.append((1, 0, 700, 17, 0, "gc"))                          # every byte 'G' or 'C': bin 100
    specs.append((1, 4, 40, 33, 1, "gc"))
    specs.append((1, 2, clen1[2] - 150, 150, 0, [149]))             # ends exactly at its contig's end
    specs.append((1, 2, clen1[2] - 150, 150, 1, [0]))
    specs.append((3, 0, 30_000 - 16, 16, 0, []))
    specs.append((3, 0, 12_100, 40, 0, [1, 2, 3]))                  # inside the N run: 'N' expected, a base written
    seqs, quals = [], []
    for g, c, lo, L, rev, alter in specs:
        want = genomes[g].contigs[c][lo:lo + L].copy()
        assert want.size == L
        if rev:
            want = comp[want[::-1]]
        if alter == "gc":
            want[:] = np.frombuffer(b"GC", dtype=np.uint8)[rng.integers(0, 2, L)]
        else:
            for j in alter:
                want[j] = ord("ACGT"[("ACGT".find(chr(want[j])) + 1 + j % 3) % 4]) if j % 5 else ord("N")
        seqs.append(want)
        quals.append((33 + rng.integers(0, 61, L)).astype(np.uint8))
    n = len(specs)
    L = np.array([s[3] for s in specs], dtype=np.int64)
    lo = np.array([s[2] for s in specs], dtype=np.int64)
    rev = np.array([s[4] for s in specs], dtype=np.uint8)
    cols = {"start": np.where(rev == 1, lo + L, lo).astype(np.uint64), "end": np.where(rev == 1, lo, lo + L).astype(np.uint64),
            "contig": np.array([s[1] for s in specs], dtype=np.uint32), "genome": np.array([s[0] for s in specs], dtype=np.uint32),
            "flags": rev.copy(), "read_id": np.arange(n, dtype=np.uint32)}
    if spoil:
        spoil(cols, specs)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(L, out=off[1:])
    host = dict(cols, seq=np.concatenate(seqs), qual=np.concatenate(quals), seq_off=off)
    if layout == 16:
        slot = (L + 15) // 16 * 16
        first = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(slot, out=first[1:])
        total = int(first[n])
        seq, qual = np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=np.uint8)
        seq_off = first.copy()
        seq_off[:n] += np.where(rev == 1, slot - L, 0)  # reverse mates right-aligned
        for r in range(n):
            seq[seq_off[r]:seq_off[r] + L[r]] = seqs[r]
            qual[first[r]:first[r] + L[r]] = quals[r]
    else:
        seq, qual, seq_off, total = host["seq"], host["qual"], off.astype(np.int64), int(off[n])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(device)
    dev = Reads(seq=t(seq, np.uint8), qual=t(qual, np.uint8), seq_off=t(seq_off, np.int64), start=t(cols["start"], np.int64),
                end=t(cols["end"], np.int64), contig=t(cols["contig"], np.int32), genome=t(cols["genome"], np.int32),
                read_id=t(cols["read_id"], np.int32), flags=t(cols["flags"], np.uint8), n_reads=n, total_bases=total,
                qual_offset=33, slot_bytes=layout)
    return dev, host
