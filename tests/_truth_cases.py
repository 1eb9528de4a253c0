"""Read columns for the truth pass (simmr_truth_plan / simmr_truth_emit; truth_kernels.hip) at the sizes where k_truth, its grid and
the engine's scan take another path — TEST INFRASTRUCTURE ONLY, no GPU and nothing from the code under test.  Every size comes from
constants() (truth_kernels.hip, kernels.hip).  A read is bytes copied from the host genome (tests/_stats_cases.expected) with chosen
bytes altered; a builder returns compact host columns (tests/_stats_cases.columns: what tests/_truth.model takes) with notes on where
it put its edits, and asserts that its bytes sit where it says.  tests/_stats_cases.device_reads lays host columns out on the device in
either layout; device_sequenced builds the many tiny reads of the grid case there.  tests/test_truth_host.py holds each builder to the
model without a GPU."""
import functools
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from tests import _fit_cases, _truth
from tests import _stats_cases as sc

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"
CONSTANTS = ("TRUTH_LANES", "TRUTH_WG_READS", "TRUTH_WGS_PER_CU", "SCAN_THREADS", "SCAN_ITEMS")


def constants():
    """{name: value} of CONSTANTS as the sources state them: TRUTH_* in truth_kernels.hip, SCAN_* in kernels.hip"""
    define = lambda src, name: int(re.search(rf"^#define\s+{name}\s+(\d+)u?\b", src, re.M).group(1))
    truth, scan = (CSRC / "truth_kernels.hip").read_text(), (CSRC / "kernels.hip").read_text()
    return {n: define(truth if n.startswith("TRUTH_") else scan, n) for n in CONSTANTS}


K = constants()
LANES, WG_READS, WGS_PER_CU, SCAN_THREADS, SCAN_ITEMS = (K[n] for n in CONSTANTS)
GROUP = 16                                   # bases of a lane's window (one 16-byte load)
ROUND = GROUP * LANES                        # bases a row of lanes takes per round
SCAN_TILE = SCAN_THREADS * SCAN_ITEMS        # counts per workgroup of the scan; k_scan_tops takes SCAN_THREADS tiles a trip
QUAL_OFFSET = sc.QUAL_OFFSET
BIG, RANDOM, UNSTAGED, EXCEPTIONS, HOMOPOLYMER = 0, 1, 2, 3, 4   # the slots of host_genomes(); UNSTAGED is never staged
_ACGT = np.frombuffer(sc.ACGT, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _host_genomes():
    g = dict(_fit_cases.host_genomes())
    g[HOMOPOLYMER] = sc.homopolymer_genome()
    assert UNSTAGED not in g and UNSTAGED < max(g)
    return g


def host_genomes():
    """{slot: HostGenome}: the genomes of tests/_fit_cases.py (BIG one contig of 1 000 000, RANDOM five contigs — the fourth of
    70 000 —, EXCEPTIONS with N and '-' runs) and tests/_stats_cases.homopolymer_genome() in slot HOMOPOLYMER"""
    return _host_genomes()


def stage(engine, genomes):
    _fit_cases.stage(engine, genomes)
    engine.stage_genome(HOMOPOLYMER, genomes[HOMOPOLYMER].contigs)


def stepped_each(want, steps):
    """tests/_stats_cases.stepped over arrays: byte i of `want` turned into the ACGT letter steps[i] places on"""
    at = np.full(256, -1, dtype=np.int64)
    at[list(sc.ACGT)] = np.arange(4)
    i, steps = at[np.asarray(want, dtype=np.uint8)], np.asarray(steps, dtype=np.int64)
    assert (i >= 0).all() and ((steps >= 1) & (steps <= 3)).all(), "a step turns an ACGT base into another"
    return _ACGT[(i + steps) % 4]


def qual_of(L, i):
    """L quality bytes that depend on the offset (and on the read, i): a shifted edit_qual shows"""
    return (QUAL_OFFSET + (np.arange(L, dtype=np.int64) + 7 * i) % 61).astype(np.uint8)


def read(oracle, genomes, g, c, lo, L, rev, at, i):
    """a read for tests/_stats_cases.columns: the expected bytes with the offsets `at` stepped by 1, 2 or 3 places (by the offset),
    every fifth of them written as 'N'"""
    seq = sc.expected(oracle, genomes, g, c, lo, L, rev)
    at = np.asarray(at, dtype=np.int64)
    if at.size:
        seq[at] = np.where(at % 5 == 4, ord("N"), stepped_each(seq[at], 1 + at % 3))
    return (g, c, lo, rev, seq, qual_of(L, i))


def edit_offsets(oracle, genomes, host):
    """per read of compact host columns, the offsets whose byte differs from the expected byte (tests/_stats_cases.expected)"""
    off = host["seq_off"].astype(np.int64)
    out = []
    for r in range(len(host["start"])):
        lo, L = int(min(host["start"][r], host["end"][r])), int(off[r + 1] - off[r])
        want = sc.expected(oracle, genomes, int(host["genome"][r]), int(host["contig"][r]), lo, L, int(host["flags"][r]) & 1)
        out.append(np.flatnonzero(host["seq"][off[r]:off[r + 1]] != want))
    return out


# ---- every base an edit --------------------------------------------------------------------------------------------------------
DENSE_LENGTHS = (1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP - 1, 2 * GROUP, 2 * GROUP + 1, ROUND - 1, ROUND, ROUND + 1,
                 GROUP * ROUND - 1, GROUP * ROUND, GROUP * ROUND + 1, 65535)


def dense_bytes(want):
    """every byte of `want` (ACGT only) replaced by another byte: the letter 1, 2, 3 places on in turn, an 'N' at every seventh
    offset and the expected letter itself in lower case at every eleventh (the comparison is bytewise)"""
    j = np.arange(want.size)
    out = stepped_each(want, 1 + j % 3)
    out[j % 7 == 3] = ord("N")
    low = j % 11 == 5
    out[low] = want[low] | 0x20
    assert (out != want).all()
    return out


@functools.lru_cache(maxsize=None)
def _dense_reads(oracle):
    genomes = host_genomes()
    reads, kinds = [], []
    lo = 1000

    def triple(g, c, at, L, rev):
        i = len(reads)
        reads.append((g, c, at, rev, dense_bytes(sc.expected(oracle, genomes, g, c, at, L, rev)), qual_of(L, i)))
        reads.append(read(oracle, genomes, RANDOM, 1, 77 + 41 * i, 40, rev ^ 1, [], i + 1))
        reads.append(read(oracle, genomes, RANDOM, 1, 99 + 41 * i, 24, rev, [0], i + 2))
        kinds.extend(("dense", "clean", "single"))
    for L in DENSE_LENGTHS[:-1]:
        for rev in (0, 1):
            triple(RANDOM, 0, lo, L, rev)
            lo += L + 13
    for rev in (0, 1):  # the longest: on the random genome and on one letter
        triple(BIG, 0, 100_003 + 400_000 * rev, DENSE_LENGTHS[-1], rev)
        triple(HOMOPOLYMER, 2 * rev, 5 + rev, DENSE_LENGTHS[-1], rev)
    host = sc.columns(reads)
    L = np.diff(host["seq_off"].astype(np.int64))
    dense = np.array([k == "dense" for k in kinds])
    assert DENSE_LENGTHS == (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4095, 4096, 4097, 65535)
    assert sorted(L[dense].tolist()) == sorted(2 * list(DENSE_LENGTHS) + 2 * [65535]) and (L[dense] == 65535).sum() == 4
    assert all(set(host["flags"][dense & (L == n)].tolist()) == {0, 1} for n in DENSE_LENGTHS)
    for ch in (ord("N"), ord("a"), ord("c"), ord("g"), ord("t")):
        assert (host["seq"] == ch).any()
    return SimpleNamespace(host=host, kinds=kinds, L=L)


def dense_reads(oracle):
    """Per length of DENSE_LENGTHS and strand a read whose EVERY byte differs from the expected byte (dense_bytes), on the random
    genome — the four of 65 535 bases on the 1 000 000-base contig and on homopolymers — followed by a read of 40 bases with no edit and
    one of 24 with a single edit at offset 0.  Qualities depend on the offset.  .host, .kinds ("dense" / "clean" / "single" per read)
    and .L.  A dense read has nm == L and edit_pos == arange(L)."""
    return _dense_reads(oracle)


# ---- the last, overlapping window ------------------------------------------------------------------------------------------------
OVERLAP_LENGTHS = (17, 18, 31, 33, 47, 255, 257, 513)


def overlap_offsets(L, pattern):
    """The last window of a read of L bases (L >= 16, no multiple of 16) loads bytes L - 16 .. L - 1 and owns 16 floor(L / 16) ..
    L - 1.  Pattern "a": the bytes it loads and does not own, "b": the ones it owns, "c": both."""
    owned = GROUP * (L // GROUP)
    assert L > GROUP and L % GROUP and L - GROUP < owned < L
    return {"a": np.arange(L - GROUP, owned), "b": np.arange(owned, L), "c": np.arange(L - GROUP, L)}[pattern]


def overlap_reads(oracle):
    """Per length of OVERLAP_LENGTHS, strand and pattern of overlap_offsets a read whose edits are exactly those offsets.
    .host and .at (the offsets per read)."""
    genomes = host_genomes()
    reads, at = [], []
    lo = 2000
    for L in OVERLAP_LENGTHS:
        for rev in (0, 1):
            for pattern in "abc":
                at.append(overlap_offsets(L, pattern))
                reads.append(read(oracle, genomes, RANDOM, 1, lo, L, rev, at[-1], len(reads)))
                lo += L + 5
    assert len(reads) == 3 * 2 * len(OVERLAP_LENGTHS) and all(a.size for a in at)
    return SimpleNamespace(host=sc.columns(reads), at=at)


# ---- reads longer than 65 535 bases -------------------------------------------------------------------------------------------
LONG_CONTIG = 3   # of genome RANDOM
LONG_LENGTHS = (65536, 65537, 70000)


def long_offsets(L):
    """an edit every 251 bases and at the last base, and 300 edits in a row that end at min(L, 65 700): the stretch holds offset 65 535 and starts a round
    (a multiple of ROUND) inside"""
    b = min(L, 65700)
    dense = np.arange(b - 300, b)
    edges = [m for m in range(ROUND, L, ROUND) if dense[0] < m <= dense[-1]]
    assert 65535 in dense and edges and dense[0] > 0
    return np.union1d(np.append(np.arange(0, L, 251), L - 1), dense)


@functools.lru_cache(maxsize=None)
def _long_reads(oracle):
    genomes = host_genomes()
    clen = genomes[RANDOM].contigs[LONG_CONTIG].size
    assert clen == max(LONG_LENGTHS) == 70000
    reads, at = [], []
    for L in LONG_LENGTHS:
        for rev in (0, 1):
            at.append(long_offsets(L))
            reads.append(read(oracle, genomes, RANDOM, LONG_CONTIG, 0 if rev else clen - L, L, rev, at[-1], len(reads)))
    return SimpleNamespace(host=sc.columns(reads), at=at)


def long_reads(oracle):
    """Reads of LONG_LENGTHS bases on the 70 000-base contig, both strands, whose edits are long_offsets(L).  .host and .at."""
    return _long_reads(oracle)


# ---- past the grid cap and the scan's first trip: many tiny reads ---------------------------------------------------------------
TINY_L = tuple((3 * i + 1) % 5 for i in range(16))   # the bases of row i of a batch: 0 .. 4


def tiny_units(oracle):
    """Four batches of WG_READS reads of TINY_L bases (the same lengths in every unit, so one seq_off serves them all), each placed
    elsewhere and on other strands: unit 0 has no edit, unit 1 one at offset 0 of every read that has a base, unit 2 every byte, unit
    3 the last byte of the reads of two bases and more.  The edit totals differ."""
    genomes = host_genomes()
    assert len(TINY_L) == WG_READS == 16 and set(TINY_L) == {0, 1, 2, 3, 4}
    units = []
    for u in range(4):
        reads = []
        for i, L in enumerate(TINY_L):
            at = [[], [0][:L], list(range(L)), [L - 1] if L >= 2 else []][u]
            reads.append(read(oracle, genomes, RANDOM, (i + u) % 2, 3000 + 911 * u + 29 * i, L, (i + u) & 1, at, 16 * u + i))
        units.append(sc.columns(reads))
    totals = [sum(a.size for a in edit_offsets(oracle, genomes, u)) for u in units]
    assert totals[0] == 0 and len(set(totals)) == len(units) >= 3
    assert all(np.array_equal(u["seq_off"], units[0]["seq_off"]) for u in units)
    return units


def unit_order(n_batches, n_units):
    """which unit batch b is: a multiplicative hash of b with its high bits folded in (the number of units may be a power of two),
    so the sequence repeats with no grid size"""
    m32 = np.uint64(0xFFFFFFFF)
    h = (np.arange(n_batches, dtype=np.uint64) * np.uint64(2654435761)) & m32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m32
    h ^= h >> np.uint64(12)
    return (h % np.uint64(n_units)).astype(np.int64)


def tiny_n(cus):
    """reads that take k_truth's workgroups into a third trip and k_scan_tops into a second that holds more than one tile, with five
    reads in the last batch"""
    return max(2 * cus * WGS_PER_CU * WG_READS, SCAN_THREADS * SCAN_TILE) + 3 * SCAN_TILE + WG_READS + 5


def tiny_shape(n, cus):
    """.batches, .grid (row_grid of truth_host.hpp), .trips of a workgroup, .last (reads in the last batch), .scan_tiles"""
    batches = -(-n // WG_READS)
    grid = max(1, min(batches, cus * WGS_PER_CU))
    return SimpleNamespace(batches=batches, grid=grid, trips=-(-batches // grid), last=n - (batches - 1) * WG_READS,
                           scan_tiles=-(-n // SCAN_TILE))


def host_sequenced(units, order, n):
    """the first n reads of the batches units[order[0]], units[order[1]], ... as compact host columns"""
    k, per = len(order), int(units[0]["seq_off"][WG_READS])
    assert (k - 1) * WG_READS < n <= k * WG_READS
    off = (np.arange(k, dtype=np.int64)[:, None] * per + units[0]["seq_off"][None, :WG_READS].astype(np.int64)).reshape(-1)
    off = np.concatenate([off, [per * k]])[:n + 1]
    out = {name: np.stack([u[name] for u in units])[order].reshape(-1)[:n] for name in sc.SMALL}
    for name in ("seq", "qual"):
        out[name] = np.stack([u[name] for u in units])[order].reshape(-1)[:off[n]]
    out["read_id"] = np.arange(n, dtype=np.uint32)
    out["seq_off"] = off.astype(np.uint64)
    return out


def assembled(models, order, n):
    """tests/_truth.model of host_sequenced(units, order, n) from the units' own models (models[u] = the model of units[u]), by
    indexing alone: a batch's edits are its unit's, the last batch's those of its first reads"""
    k = len(order)
    assert (k - 1) * WG_READS < n <= k * WG_READS
    nm = np.stack([m["nm"] for m in models])[order].reshape(-1)[:n]
    edit_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(nm, out=edit_off[1:])
    reads_in = np.full(k, WG_READS, dtype=np.int64)
    reads_in[-1] = n - (k - 1) * WG_READS
    count = np.stack([m["edit_off"].astype(np.int64) for m in models])[order, reads_in]   # edits of each batch
    first = np.concatenate([[0], np.cumsum([m["edit_pos"].size for m in models])])[order]  # where its unit's edits start in the table
    starts = np.concatenate([[0], np.cumsum(count)])
    idx = np.repeat(first - starts[:-1], count) + np.arange(int(starts[-1]), dtype=np.int64)
    out = {"nm": nm.astype(np.uint32), "edit_off": edit_off}
    for col in ("edit_pos", "edit_ref", "edit_alt", "edit_qual"):
        out[col] = np.concatenate([m[col] for m in models])[idx]
    assert int(edit_off[n]) == idx.size
    return out


def device_sequenced(units, order, n, device):
    """host_sequenced(units, order, n) in the compact layout, built on `device` from the units alone: tests/_stats_cases.device_tiled
    lays out the offsets (every unit has the same), then each column is the units' table indexed by `order`"""
    import torch
    k = len(order)
    dev = sc.device_tiled(units[0], k, device)
    at = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int64)).to(device)
    for name in sc.SMALL + ("seq", "qual"):
        was = getattr(dev, name)
        table = torch.from_numpy(np.stack([np.ascontiguousarray(u[name]) for u in units]).astype(np.int64)).to(device=device, dtype=was.dtype)
        new = table[at].reshape(-1)
        assert new.shape == was.shape
        setattr(dev, name, new)
    return dev if n == dev.n_reads else sc.first_reads(dev, n)


# ---- a small set for the calls' own rules ---------------------------------------------------------------------------------------
EDGE_CONTIG = 2   # of genome RANDOM: not its last contig, so one base past its end is still a staged base


def small_reads(oracle):
    """Nine reads with 0, 1 and several edits on both strands; read 3 (forward) and read 6 (reverse) end exactly at their contig's
    end, read 4 has no base and sits at lo == the contig's length.  .host, .planned (edits per read), .clen (that contig's length)."""
    genomes = host_genomes()
    clen = int(genomes[RANDOM].contigs[EDGE_CONTIG].size)
    specs = [(0, 500, 40, 0, []), (0, 700, 17, 1, [3]), (0, 900, 64, 0, [0, 15, 16, 31, 47, 63]), (EDGE_CONTIG, clen - 150, 150, 0, [149]),
             (EDGE_CONTIG, clen, 0, 0, []), (0, 1500, 100, 1, [5, 50, 98]), (EDGE_CONTIG, clen - 33, 33, 1, []),
             (0, 2100, 300, 0, list(range(0, 300, 9))), (0, 2600, 50, 1, [1, 48])]
    host = sc.columns([read(oracle, genomes, RANDOM, c, lo, L, rev, at, i) for i, (c, lo, L, rev, at) in enumerate(specs)])
    planned = [len(s[4]) for s in specs]
    assert EDGE_CONTIG + 1 < len(genomes[RANDOM].contigs) and 0 in planned and 1 in planned and max(planned) > 16
    return SimpleNamespace(host=host, planned=planned, clen=clen)
