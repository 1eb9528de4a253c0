"""Numpy restatement of "strain sites, version 1" (include/simmr_hip.h, simmr_strain_plan), written from the specification:
a vectorised Philox4x32-10, the site rule, the in-place edit of ASCII contigs, simmr-hip's seed rule and the TSV of
`--strain-sites`.  Nothing here looks at the kernels except constants(), which parses the sizes the GPU tests place their
genomes by."""
import math
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
DOMAIN, C3 = 5, 0x72000003
SEED_STEP = 0x9E3779B97F4A7C15
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CODE = np.full(256, 255, dtype=np.uint8)  # ASCII -> 2-bit code; 255: under the exception plane ('N', '-')
CODE[ACGT] = np.arange(4, dtype=np.uint8)
TSV_HEADER = "genome_id\tsequence_id\tposition\tref\talt\n"


def constants():
    """(STRAIN_TILE, STRAIN_TOPS_WIDTH) of simmr_amd/csrc/strain_kernels.hip"""
    src = (ROOT / "simmr_amd" / "csrc" / "strain_kernels.hip").read_text()
    return tuple(int(re.search(rf"constexpr uint32_t {name} = (\d+);", src).group(1)) for name in ("STRAIN_TILE", "STRAIN_TOPS_WIDTH"))


def philox4x32_10(ctr, key):
    """ctr: (n, 4), key: (n, 2) of 32-bit words -> (n, 4) uint32.  Random123's Philox4x32-10: ten rounds of
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped by (W0, W1) between
    rounds."""
    c = [np.asarray(ctr)[:, i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[:, i].astype(np.uint64) for i in range(2)]
    mask = np.uint64(0xFFFFFFFF)
    for r in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return np.stack(c, axis=1).astype(np.uint32)


def thresholds(identity):
    """(T32, A, B)"""
    t32 = int(math.floor((1.0 - identity) * 4294967296.0 + 0.5))
    return t32, -(-t32 // 3), -(-2 * t32 // 3)


def words(n, contig, seed):
    """X of positions 0 .. n - 1 of contig `contig`: word pos & 3 of the block with counter (pos >> 2, 5, contig, 0x72000003)"""
    nb = (n + 3) // 4
    ctr = np.empty((nb, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.arange(nb, dtype=np.uint64), DOMAIN, contig, C3
    key = np.empty((nb, 2), dtype=np.uint32)
    key[:, 0], key[:, 1] = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    return philox4x32_10(ctr, key).reshape(-1)[:n]


def sites_of(seq, contig, identity, seed):
    """(pos uint64, ref uint8, alt uint8) of the sites of one ASCII contig"""
    seq = np.asarray(seq, dtype=np.uint8)
    t32, a, b = thresholds(identity)
    x = words(seq.size, contig, seed).astype(np.uint64)
    code = CODE[seq]
    pos = np.flatnonzero((x < t32) & (code != 255))
    s = 1 + (x[pos] >= a).astype(np.uint8) + (x[pos] >= b).astype(np.uint8)
    return pos.astype(np.uint64), seq[pos], ACGT[(code[pos] + s) & 3]


def diverge(contigs, identity, seed):
    """The genome after simmr_strain_apply and the four site columns: ([ASCII contigs], {contig, pos, ref, alt}), the sites
    ordered by contig, then by position."""
    out, cols = [], {"contig": [], "pos": [], "ref": [], "alt": []}
    for c, seq in enumerate(contigs):
        new = np.array(seq, dtype=np.uint8, copy=True)
        pos, ref, alt = sites_of(new, c, identity, seed)
        new[pos.astype(np.int64)] = alt
        out.append(new)
        cols["contig"].append(np.full(pos.size, c, dtype=np.uint32))
        cols["pos"].append(pos)
        cols["ref"].append(ref)
        cols["alt"].append(alt)
    dt = {"contig": np.uint32, "pos": np.uint64, "ref": np.uint8, "alt": np.uint8}
    return out, {k: np.concatenate(v).astype(dt[k]) if v else np.empty(0, dt[k]) for k, v in cols.items()}


def genome_seed(run_seed, i):
    """simmr-hip --with-ani: the seed of genome i (0-based, in the order of the genome list) of a run"""
    return (run_seed + SEED_STEP * (i + 1)) & ((1 << 64) - 1)


def tsv_rows(cols, genome_id, sequence_ids):
    """The lines of `--strain-sites` for one genome (without the header line)"""
    return "".join(f"{genome_id}\t{sequence_ids[int(c)]}\t{int(p)}\t{chr(r)}\t{chr(a)}\n"
                   for c, p, r, a in zip(cols["contig"], cols["pos"], cols["ref"], cols["alt"]))
