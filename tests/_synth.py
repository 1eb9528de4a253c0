"""Deterministic synthetic references: word k (32 bases) of the
2-bit plane is SplitMix64 output k of the seed; contigs start on 64-base
boundaries of that plane.  numpy mirror of simmr_stage_synthetic."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def splitmix64_words(seed: int, n: int, first: int = 0) -> np.ndarray:
    """outputs first + 1 .. first + n of the generator"""
    with np.errstate(over="ignore"):
        k = np.arange(first + 1, first + n + 1, dtype=np.uint64)
        z = np.uint64(seed) + k * GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def synthetic_contigs(contig_lens, seed: int):
    """list of uint8 ASCII arrays, one per contig"""
    bases = []
    off = 0
    for n in contig_lens:
        bases.append(off)
        off += (int(n) + 63) // 64 * 64
    words = splitmix64_words(seed, max(off // 32, 1))
    shifts = (np.arange(32, dtype=np.uint64) * np.uint64(2))
    codes = ((words[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.uint8).reshape(-1)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [lut[codes[b:b + int(n)]] for b, n in zip(bases, contig_lens)]


def synthetic_contigs_chunked(contig_lens, seed: int, chunk_words: int = 1 << 20):
    """synthetic_contigs with bounded working memory: the plane is expanded `chunk_words` words (32 bases each) at a
    time, so a 100 Mbp contig costs its own bytes plus a few chunks instead of an 8-byte intermediate per base"""
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    shifts = (np.arange(32, dtype=np.uint64) * np.uint64(2))
    out = []
    off = 0
    for n in contig_lens:
        n = int(n)
        contig = np.empty(n, dtype=np.uint8)
        w0 = off // 32  # contigs start on 64-base boundaries: a whole word
        for a in range(0, (n + 31) // 32, chunk_words):
            nw = min(chunk_words, (n + 31) // 32 - a)
            words = splitmix64_words(seed, nw, w0 + a)
            codes = ((words[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.uint8).reshape(-1)
            lo = 32 * a
            hi = min(n, lo + 32 * nw)
            contig[lo:hi] = lut[codes[: hi - lo]]
        out.append(contig)
        off += (n + 63) // 64 * 64
    return out


def write_fasta(path, contigs, names=None, width=80):
    with open(path, "wb") as f:
        for i, c in enumerate(contigs):
            name = names[i] if names else f"synth_{i}"
            f.write(b">" + name.encode() + b"\n")
            b = c.tobytes()
            for j in range(0, len(b), width):
                f.write(b[j:j + width] + b"\n")
