"""Read columns for the run statistics (simmr_stats_add; stats_kernels.hip) at the bounds k_read_stats' comment derives — the flush
inside the batch loop, the 16-bit halves of its packed words, the whole range of a quality byte, the longest read — TEST
INFRASTRUCTURE ONLY, no GPU and nothing from the code under test.  Every size comes from tests/_stats.constants()
(stats_kernels.hip).  A builder returns compact host columns (what tests/_stats.model takes) and asserts that its bytes sit where
it says; `device_reads` lays host columns out on the device in either layout, `device_tiled` repeats a batch there without a
host copy.  tests/test_stats_host.py pins where each case lands in the model."""
import functools
from types import SimpleNamespace

import numpy as np

from tests import _fit_cases, _oracle, _stats, _synth, _truth

K = _stats.constants()
LANES, WG_READS, WGS_PER_CU, FLUSH_BATCHES, MAX_L, CYC_STRIDE = (K[n] for n in _stats.CONSTANTS)
QUAL_OFFSET = 33
ACGT = b"ACGT"
SMALL = ("start", "end", "contig", "genome", "flags")   # the columns with one entry per read, read_id apart
RANDOM, HOMOPOLYMER = 0, 1                              # the slots of host_genomes()
EDGE_CYCLES = (0, 255, 256, 511)


def homopolymer_genome():
    """four contigs of MAX_L + 17 bases: all A, all C, all G, all T"""
    return _oracle.HostGenome([np.full(MAX_L + 17, ch, dtype=np.uint8) for ch in ACGT])


@functools.lru_cache(maxsize=None)
def _host_genomes():
    return {RANDOM: _oracle.HostGenome(_synth.synthetic_contigs([4000, 1501], 5)), HOMOPOLYMER: homopolymer_genome()}


def host_genomes():
    """{slot: HostGenome}: slot RANDOM two small synthetic contigs (ACGT only), slot HOMOPOLYMER homopolymer_genome()"""
    return _host_genomes()


def stage(engine, genomes):
    for slot, g in genomes.items():
        engine.stage_genome(slot, g.contigs)


def expected(oracle, genomes, g, c, lo, L, rev):
    """the bytes an unedited read of L bases from `lo` of contig c of genome g carries (a copy)"""
    want = genomes[g].contigs[c][lo:lo + L].copy()
    assert want.size == L, "a read leaves its contig"
    return _truth.complement_lut(oracle)[want[::-1]] if rev else want


def stepped(byte, s):
    """the ACGT letter s places on from `byte`"""
    at = ACGT.find(bytes([int(byte)]))
    assert at >= 0 and s in (1, 2, 3)
    return ACGT[(at + s) % 4]


def columns(reads):
    """compact host columns of `reads`: a list of (genome, contig, lo, rev, written bytes, quality bytes)"""
    n = len(reads)
    L = np.array([len(r[4]) for r in reads], dtype=np.int64)
    assert all(len(r[5]) == len(r[4]) for r in reads)
    lo = np.array([r[2] for r in reads], dtype=np.int64)
    rev = np.array([r[3] for r in reads], dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(L, out=off[1:])
    cat = lambda i: np.concatenate([np.asarray(r[i], dtype=np.uint8) for r in reads])
    return {"start": np.where(rev == 1, lo + L, lo).astype(np.uint64), "end": np.where(rev == 1, lo, lo + L).astype(np.uint64),
            "contig": np.array([r[1] for r in reads], dtype=np.uint32), "genome": np.array([r[0] for r in reads], dtype=np.uint32),
            "flags": rev.copy(), "read_id": np.arange(n, dtype=np.uint32), "seq": cat(4), "qual": cat(5), "seq_off": off}


def device_reads(host, layout, device, qual_offset=QUAL_OFFSET):
    """`host` (compact columns) on the device, compact (layout 0) or in 16-byte slots (16), to be read under `qual_offset`"""
    dev = _fit_cases.device_reads(host, layout, device)
    dev.qual_offset = int(qual_offset)
    return dev


# ---- the flush -----------------------------------------------------------------------------------------------------------------
def uniform_unit(oracle, genomes):
    """One batch of WG_READS reads of 1 .. 4 bases (40 bases in all), each with a base at cycle 0.  Read i sits on row i of its
    workgroup, so in block i & 3 of the packed cycle words; the cycle-0 byte of all four reads of a block is written as 'C'
    (blocks 0, 1) or 'T' (blocks 2, 3) over a reference base that is another letter.  Per batch, then, cycle 0 of a block adds 4
    to both halves of w0 (reads, edits) and 4 to the high half of w1 ('C') or of w2 ('T'): FLUSH_BATCHES batches take those halves
    to the 16 384 the kernel's comment allows.  Block 3's cycle-0 quality byte is QUAL_OFFSET - 1 — below the offset, q = 255 —
    so its w3 reaches the 255 x 16 384 of the same comment.  Both strands in both sets, one written N, a few later edits."""
    rng = np.random.default_rng(16)
    reads = []
    for i in range(WG_READS):
        block, L, rev = i & 3, 1 + ((i + (i >> 2)) & 3), (i >> 1) & 1
        target = ord("C") if block < 2 else ord("T")
        lo = 100 + 37 * i
        while expected(oracle, genomes, RANDOM, 0, lo, L, rev)[0] == target:
            lo += 1
        seq = expected(oracle, genomes, RANDOM, 0, lo, L, rev)
        seq[0] = target
        if i == 1:
            seq[1] = ord("N")
        if i in (3, 6):
            seq[L - 1] = stepped(seq[L - 1], 1 + i % 3)
        qual = rng.integers(QUAL_OFFSET, QUAL_OFFSET + 61, L).astype(np.uint8)
        if block == 3:
            qual[0] = QUAL_OFFSET - 1
        reads.append((RANDOM, 0, lo, rev, seq, qual))
    unit = columns(reads)
    L = np.diff(unit["seq_off"].astype(np.int64))
    assert len(reads) == WG_READS == 16 and sorted(L.tolist()) == sorted(4 * [1, 2, 3, 4]) and int(L.sum()) == 40
    assert all(sorted(L[b::4].tolist()) == [1, 2, 3, 4] for b in range(4))                            # every length in every block
    first = unit["seq"][unit["seq_off"][:-1].astype(np.int64)]
    assert all(set(first[b::4].tolist()) == {ord("C") if b < 2 else ord("T")} for b in range(4))      # one letter per block
    assert all(set(unit["flags"][s::2].tolist()) == {0, 1} for s in (0, 1))                           # both strands in both sets
    for n_sets in (1, 2):
        m = _stats.model(oracle, unit, genomes, n_sets, QUAL_OFFSET)
        assert m["reads"].sum() == m["cycle_n"][:, 0].sum() == m["cycle_mismatch"][:, 0].sum() == 16
        assert m["cycle_base"][:, 0, 1].sum() == m["cycle_base"][:, 0, 3].sum() == 8 and m["bases"].sum() == 40
        if n_sets == 2:  # block b holds set b & 1: every block's four reads are of one set, two blocks a set
            assert m["cycle_base"][:, 0, 1].tolist() == m["cycle_base"][:, 0, 3].tolist() == [4, 4] and m["reads"].tolist() == [8, 8]
        assert m["qual_n"][255] == 4 and m["qual_n"][94:255].sum() == 0 and m["cycle_qsum"][:, 0].sum() >= 4 * 255
        assert m["pair"][:, 4].sum() == 1 and m["qual_mismatch"].sum() == 16 + 3 and m["nm_hist"][2] == 3
    return unit


def tiled(unit, k):
    """the batch `unit` k times as compact host columns: read r is read r mod WG_READS of the unit"""
    n = len(unit["start"])
    per = int(unit["seq_off"][n])
    out = {name: np.tile(unit[name], k) for name in SMALL + ("seq", "qual")}
    out["read_id"] = np.arange(n * k, dtype=np.uint32)
    off = (np.arange(k, dtype=np.uint64)[:, None] * np.uint64(per) + unit["seq_off"][None, :n]).reshape(-1)
    out["seq_off"] = np.concatenate([off, [np.uint64(per * k)]]).astype(np.uint64)
    return out


def scaled(model, k):
    """every table of `model` times k"""
    return {name: (model[name] * np.uint64(k)).astype(np.uint64) for name in _stats.SHAPES}


def device_tiled(unit, k, device):
    """tiled(unit, k) in the compact layout, built on `device` from the unit alone: `repeat` for the columns with one entry a
    read and for the bytes, seq_off from an arange over the batches"""
    import torch
    from simmr_amd.engine import Reads
    n = len(unit["start"])
    per = int(unit["seq_off"][n])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(device)
    seq_off = torch.empty(n * k + 1, dtype=torch.int64, device=device)
    torch.add(torch.arange(k, dtype=torch.int64, device=device)[:, None] * per, t(unit["seq_off"][:n], np.int64)[None, :],
              out=seq_off[:n * k].view(k, n))
    seq_off[n * k] = per * k
    return Reads(seq=t(unit["seq"], np.uint8).repeat(k), qual=t(unit["qual"], np.uint8).repeat(k), seq_off=seq_off,
                 start=t(unit["start"], np.int64).repeat(k), end=t(unit["end"], np.int64).repeat(k),
                 contig=t(unit["contig"], np.int32).repeat(k), genome=t(unit["genome"], np.int32).repeat(k),
                 read_id=torch.arange(n * k, dtype=torch.int32, device=device), flags=t(unit["flags"], np.uint8).repeat(k),
                 n_reads=n * k, total_bases=per * k, qual_offset=QUAL_OFFSET, slot_bytes=0)


def first_reads(dev, n):
    """the first n reads of compact device columns, on the same memory"""
    from simmr_amd.engine import Reads
    assert dev.slot_bytes == 0 and n <= dev.n_reads
    return Reads(seq=dev.seq, qual=dev.qual, seq_off=dev.seq_off[:n + 1], start=dev.start[:n], end=dev.end[:n], contig=dev.contig[:n],
                 genome=dev.genome[:n], read_id=dev.read_id[:n], flags=dev.flags[:n], n_reads=n, total_bases=dev.total_bases,
                 qual_offset=dev.qual_offset, slot_bytes=0)


# ---- the 16-bit halves and the longest read --------------------------------------------------------------------------------------
def by_offset(L):
    return (QUAL_OFFSET + np.arange(L, dtype=np.int64) % 61).astype(np.uint8)


def homopolymer_reads(oracle, genomes):
    """Reads of MAX_L bases on homopolymer_genome().  .host: per contig a forward and a reverse read with no edit (one class of
    the diagonal takes all MAX_L bases of a row: each half of same01 / same23 filled with nothing in the other — the reverse
    read of the A contig is all 'T'); one read on the A contig with every byte an edit to C, G, T in turn (nm = MAX_L, nothing
    on the diagonal); one on the T contig with every byte 'N' (class "other", every one an edit); one on the C contig with every
    byte 'G' (gc = L: bin 100).  .too_long: a good read, one of MAX_L + 1 bases inside its contig with two edits, a good read —
    and .good, the two good ones alone.  .all_edit: where the all-edit read lands off the diagonal of pair."""
    g = HOMOPOLYMER
    plain = lambda c, lo, L, rev: (g, c, lo, rev, expected(oracle, genomes, g, c, lo, L, rev), by_offset(L))
    reads = [plain(c, 3 + 2 * c + rev, MAX_L, rev) for c in range(4) for rev in (0, 1)]
    cgt = np.frombuffer(b"CGT", dtype=np.uint8)[np.arange(MAX_L) % 3]
    reads.append((g, 0, 1, 0, cgt, by_offset(MAX_L)))
    reads.append((g, 3, 17, 0, np.full(MAX_L, ord("N"), dtype=np.uint8), by_offset(MAX_L)))
    reads.append((g, 1, 0, 0, np.full(MAX_L, ord("G"), dtype=np.uint8), by_offset(MAX_L)))
    assert all(len(r[4]) == MAX_L == 65535 for r in reads) and len(reads) == 11 <= WG_READS
    for c in range(4):
        assert set(reads[2 * c][4].tolist()) == {ACGT[c]} and set(reads[2 * c + 1][4].tolist()) == {ACGT[3 - c]}
    all_edit = np.zeros((5, 5), dtype=np.uint64)
    all_edit[0, 1:4] = MAX_L // 3

    def short(lo, L, rev, at):
        seq = expected(oracle, genomes, g, 2, lo, L, rev)
        for j in at:
            seq[j] = stepped(seq[j], 1 + j % 3)
        return (g, 2, lo, rev, seq, by_offset(L))
    long_one = expected(oracle, genomes, g, 0, 7, MAX_L + 1, 0)
    long_one[[0, MAX_L]] = ord("G")
    good = [short(40, 40, 0, [5]), short(900, 33, 1, [0, 16, 32])]
    too_long = [good[0], (g, 0, 7, 0, long_one, by_offset(MAX_L + 1)), good[1]]
    assert len(long_one) == MAX_L + 1 <= genomes[g].contigs[0].size - 7
    return SimpleNamespace(host=columns(reads), too_long=columns(too_long), good=columns(good), all_edit=all_edit, nm=[1, 2, 3])


# ---- every quality byte ----------------------------------------------------------------------------------------------------------
def quality_range(oracle, genomes):
    """Reads of 16, 17, 256, 512 and 513 bases on both strands whose quality bytes run through all 256 values, so every q bin
    is hit under qual_offset 33 (where bytes 0 .. 32 wrap) and under 0.  At each of EDGE_CYCLES a read holds, its byte is 255
    (forward) or 32 (reverse: below 33, and q = 255 under it), and the base there is an edit in the reads of 512 and 513."""
    reads = []
    for k, (L, rev) in enumerate((L, rev) for L in (16, 17, 256, 512, 513) for rev in (0, 1)):
        lo = 50 + 300 * k
        seq = expected(oracle, genomes, RANDOM, 0, lo, L, rev)
        qual = ((7 * np.arange(L) + 11 * k) & 255).astype(np.uint8)
        for j in EDGE_CYCLES:
            if j < L:
                qual[j] = 32 if rev else 255
                if L >= 512 or j == 0 and k & 2:
                    seq[j] = stepped(seq[j], 1 + (j + k) % 3)
        if L == 17:
            seq[16] = ord("N")
        reads.append((RANDOM, 0, lo, rev, seq, qual))
    host = columns(reads)
    assert np.unique(host["qual"]).size == 256
    off = host["seq_off"].astype(np.int64)
    for j in EDGE_CYCLES:
        there = {int(host["qual"][off[r] + j]) for r in range(len(reads)) if off[r + 1] - off[r] > j}
        assert there == {32, 255}, j
    return host
