"""Read columns for the column route of the model fit (simmr_fit_add; fit_kernels.hip) at the sizes where k_fit_add takes
another path — TEST INFRASTRUCTURE ONLY, no GPU and nothing from the code under test.  Every size comes from
tests/_fit.constants() (fit_device.hpp).  A case is a list of specs `(genome, contig, lo, L, rev, {offset: byte}[, qual])`: L bases
of the contig from `lo`, reverse-complemented if `rev`, then altered in the read's own orientation — a byte as a one-letter
string is written as it is, an integer s in 1 .. 3 turns the read's own ACGT base into the one s places on — with the L quality
bytes given or drawn.  `reads_of` turns specs into compact host columns (what tests/_fit.model takes), `device_reads` lays host
columns out on the device in either layout.  Each builder asserts that its bytes sit where it says; tests/test_fit_host.py
pins the same against the plain k-mer rule."""
import functools
from types import SimpleNamespace

import numpy as np

from tests import _fit, _oracle, _stats, _synth, _truth

K = _fit.constants()
LANES, WG_READS, FLUSH_BATCHES, LDS_POS, LDS_LEN, LDS_K, MAX_PROBE, MAX_L = (K[n] for n in _fit.CONSTANTS)
GROUP = 16                                                  # bases a lane takes per round
ROUND = GROUP * LANES                                       # bases a row takes per round
EDGES = (GROUP, ROUND, 2 * ROUND)                           # 16, 256, 512: the lane's group, the row's round and its second
KS = (3, LDS_K, LDS_K + 1, 10)
QUAL_OFFSET = 33


@functools.lru_cache(maxsize=None)
def _host_genomes():
    # (the genomes of tests/test_gpu_truth.py)
    rng = np.random.default_rng(21)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30000)].copy()
    seq[rng.integers(0, 30000, 3000)] = ord("N")
    seq[rng.integers(0, 30000, 500)] = ord("-")
    seq[12_000:12_400] = ord("N")
    return {0: _oracle.HostGenome(_synth.synthetic_contigs([1_000_000], 1)),
            1: _oracle.HostGenome(_synth.synthetic_contigs([300_000, 90_001, 30_017, 70_000, 123_457], 7)),
            3: _oracle.HostGenome([seq])}


def host_genomes():
    """{slot: HostGenome}: slot 0 and 1 synthetic (ACGT only), slot 3 with N and '-' runs"""
    return _host_genomes()


def stage(engine, genomes):
    engine.stage_synthetic(0, [1_000_000], 1)
    engine.stage_genome(1, genomes[1].contigs)
    engine.stage_genome(3, genomes[3].contigs)


def reads_of(oracle, genomes, specs, rng=None):
    """compact host columns of `specs`; qualities not given are drawn from `rng`, 33 + [0, 61), in the specs' order"""
    comp = _truth.complement_lut(oracle)
    seqs, quals = [], []
    for spec in specs:
        g, c, lo, L, rev, alter = spec[:6]
        want = genomes[g].contigs[c][lo:lo + L].copy()
        assert want.size == L
        if rev:
            want = comp[want[::-1]]
        for j, ch in alter.items():
            if isinstance(ch, str):
                want[j] = ord(ch)
            else:
                at = _fit.ACGT.find(bytes([want[j]]))
                assert at >= 0 and ch in (1, 2, 3), "a step turns an ACGT base into another"
                want[j] = _fit.ACGT[(at + ch) % 4]
        seqs.append(want)
        q = np.asarray(spec[6], dtype=np.uint8) if len(spec) > 6 else (QUAL_OFFSET + rng.integers(0, 61, L)).astype(np.uint8)
        assert q.size == L
        quals.append(q)
    n = len(specs)
    L = np.array([s[3] for s in specs], dtype=np.int64)
    lo = np.array([s[2] for s in specs], dtype=np.int64)
    rev = np.array([s[4] for s in specs], dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(L, out=off[1:])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return {"start": np.where(rev == 1, lo + L, lo).astype(np.uint64), "end": np.where(rev == 1, lo, lo + L).astype(np.uint64),
            "contig": np.array([s[1] for s in specs], dtype=np.uint32), "genome": np.array([s[0] for s in specs], dtype=np.uint32),
            "flags": rev.copy(), "read_id": np.arange(n, dtype=np.uint32), "seq": cat(seqs), "qual": cat(quals), "seq_off": off}


def device_reads(host, layout, device):
    """`host` (compact columns) on the device: compact (layout 0), or in 16-byte slots (layout 16: a reverse read's bases
    right-aligned in its slots, its qualities from the slots' first byte)"""
    import torch
    from simmr_amd.engine import Reads
    n = len(host["start"])
    off = host["seq_off"].astype(np.int64)
    L = np.diff(off)
    rev = (host["flags"] & 1).astype(np.int64)
    if layout == 16:
        slot = (L + 15) // 16 * 16
        first = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(slot, out=first[1:])
        total = int(first[n])
        seq, qual = np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=np.uint8)
        seq_off = first.copy()
        seq_off[:n] += np.where(rev == 1, slot - L, 0)
        within = np.arange(int(off[n]), dtype=np.int64) - np.repeat(off[:n], L)
        seq[np.repeat(seq_off[:n], L) + within] = host["seq"]
        qual[np.repeat(first[:n], L) + within] = host["qual"]
    else:
        assert layout == 0
        seq, qual, seq_off, total = host["seq"], host["qual"], off, int(off[n])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(device)
    return Reads(seq=t(seq, np.uint8), qual=t(qual, np.uint8), seq_off=t(seq_off, np.int64), start=t(host["start"], np.int64),
                 end=t(host["end"], np.int64), contig=t(host["contig"], np.int32), genome=t(host["genome"], np.int32),
                 read_id=t(host["read_id"], np.int32), flags=t(host["flags"], np.uint8), n_reads=n, total_bases=total,
                 qual_offset=QUAL_OFFSET, slot_bytes=layout)


def rows(host, a, b):
    """reads a .. b - 1 of compact host columns, as compact host columns"""
    off = host["seq_off"].astype(np.int64)
    out = {name: host[name][a:b] for name in ("start", "end", "contig", "genome", "flags", "read_id")}
    out["seq"], out["qual"] = host["seq"][off[a]:off[b]], host["qual"][off[a]:off[b]]
    out["seq_off"] = (off[a:b + 1] - off[a]).astype(np.uint64)
    return out


def joined(shards):
    """several compact host column sets as one"""
    out = {name: np.concatenate([s[name] for s in shards]) for name in ("start", "end", "contig", "genome", "flags", "seq", "qual")}
    out["read_id"] = np.arange(len(out["start"]), dtype=np.uint32)
    L = np.concatenate([np.diff(s["seq_off"].astype(np.int64)) for s in shards])
    out["seq_off"] = np.concatenate([[0], np.cumsum(L)]).astype(np.uint64)
    return out


def n_windows(L, k):
    """windows of a read of L bases: the starts ndx with ndx + k < L"""
    return max(L - k, 0)


def place(p):
    """(round, lane, byte) of base p of a read under k_fit_add: a row takes ROUND bases a round, a lane GROUP of them"""
    return p // ROUND, p // GROUP % LANES, p % GROUP


# ---- the row's seams ------------------------------------------------------------------------------------------------------
def seam_rows(k):
    """Around each column E of EDGES, on both strands: 2 k reads with ONE changed base each, at E - k .. E + k - 1, long enough
    that every window over the changed base counts; one read with an N written at E - 1 and at E; and unchanged reads of every
    length E - 1 .. E + k + 1 (the last group holds 1 .. k + 1 bases, or ends the round before).  .specs, and .notes: per spec
    the altered offsets (.at), its windows and how many of them are changed."""
    specs, notes = [], []
    lo = 1000
    for E in EDGES:
        L = E + 2 * k + 1
        for rev in (0, 1):
            for p in range(E - k, E + k):
                # the windows over p end at p .. p + k - 1; the one that ends at e counts when e + 1 < L
                assert p + k - 1 + 1 < L and p >= 0
                assert (place(p)[0] < place(E)[0] or place(p)[1] != place(E)[1]) == (p < E)  # on either side of the seam
                specs.append((1, 0, lo, L, rev, {p: 1 + p % 3}))
                notes.append(SimpleNamespace(E=E, at=[p], windows=n_windows(L, k), changed=min(k, p + 1)))  # (they start at 0 at the earliest)
                lo += 7
            specs.append((1, 0, lo, L, rev, {E - 1: "N", E: "N"}))
            notes.append(SimpleNamespace(E=E, at=[E - 1, E], windows=n_windows(L, k), changed=k + 1))
            lo += 7
            for length in range(E - 1, E + k + 2):
                specs.append((1, 0, lo, length, rev, {}))
                notes.append(SimpleNamespace(E=E, at=[], windows=n_windows(length, k), changed=0))
                lo += 7
    for E in EDGES[1:]:  # lane 15 of one round, lane 0 of the next: what carry_w / carry_h cross
        assert place(E - 1)[1:] == (LANES - 1, GROUP - 1) and place(E)[1:] == (0, 0) and place(E)[0] == place(E - 1)[0] + 1
    assert place(EDGES[0] - 1) == (0, 0, GROUP - 1) and place(EDGES[0]) == (0, 1, 0)
    assert lo + max(EDGES) + 2 * k + 1 < 300_000
    return SimpleNamespace(specs=specs, notes=notes, k=k, n_positions=max(EDGES) + 2 * k + 1)


# ---- inserts ------------------------------------------------------------------------------------------------------------------
def insert_pairs():
    """Pairs by span: 1, LDS_LEN - 1, LDS_LEN, LDS_LEN + 1 (LDS against HBM), MAX_INSERT - 1, MAX_INSERT, MAX_INSERT + 1 (kept against
    dropped) and one far above; forward / reverse mates, both forward, both reverse, the second mate to the left, and a mate
    inside its mate.  .specs, .spans (one per pair) and .kept (the inserts the histogram takes: one per mate)."""
    specs, spans = [], []
    lo = 2000

    def pair(span, l1, l2, rev1, rev2, second_left=False):
        nonlocal lo
        a, b = (1, 0, lo, l1, rev1, {}), (1, 0, lo + span - l2, l2, rev2, {})
        assert span >= max(l1, l2)
        specs.extend((b, a) if second_left else (a, b))
        spans.append(span)
        lo += 13
    pair(1, 1, 1, 0, 1)
    for i, span in enumerate((LDS_LEN - 1, LDS_LEN, LDS_LEN + 1, _fit.MAX_INSERT - 1, _fit.MAX_INSERT, _fit.MAX_INSERT + 1, 200_000)):
        pair(span, 30 + i, 41 - i, 0, 1)
        pair(span, 25, 33 + i, i & 1, i & 1)              # both mates on one strand
        pair(span, 36, 28, 1, 0, second_left=True)
    pair(60, 60, 20, 0, 1)                                 # the second mate ends where the first ends, inside it
    pair(LDS_LEN, LDS_LEN, LDS_LEN, 0, 1)                  # two mates of 1024 bases on one interval
    for i, span in enumerate(spans):                       # the span as the header states it, from the columns the kernel reads
        (_, _, l1, n1, _, _), (_, _, l2, n2, _, _) = specs[2 * i], specs[2 * i + 1]
        assert max(l1 + n1, l2 + n2) - min(l1, l2) == span
    kept = sorted(s for s in spans for _ in (0, 1) if s <= _fit.MAX_INSERT)
    for edge in (LDS_LEN - 1, LDS_LEN, _fit.MAX_INSERT):
        assert kept.count(edge) >= 6
    assert spans.count(_fit.MAX_INSERT + 1) == 3 and max(kept) == _fit.MAX_INSERT
    return SimpleNamespace(specs=specs, spans=spans, kept=kept)


# ---- the pair table ---------------------------------------------------------------------------------------------------------
def full_table(D, k=LDS_K):
    """ONE reference window (genome 1, contig 0, 3000 .. 3000 + k) under D different written ACGT k-mers, none the reference's:
    reads of k + 1 bases, one window each, read m writing the base 4 digits of m + 1 as steps.  Every third k-mer is seen
    twice and every seventh three times, so the counts differ.  .specs, .distinct (D) and .times (per written k-mer)."""
    assert 0 < D < 4 ** k
    specs, times = [], []
    for m in range(1, D + 1):
        alter = {f: (m >> (2 * f)) & 3 for f in range(k) if (m >> (2 * f)) & 3}
        assert alter
        t = 3 if m % 7 == 0 else 2 if m % 3 == 0 else 1
        specs.extend([(1, 0, 3000, k + 1, 0, alter)] * t)
        times.append(t)
    assert n_windows(k + 1, k) == 1 and len(times) == D and len(set(times)) == (3 if D >= 7 else 2 if D >= 3 else 1)
    return SimpleNamespace(specs=specs, distinct=D, times=times, k=k)


# ---- the flush -----------------------------------------------------------------------------------------------------------------
UNIFORM_K, UNIFORM_L, UNIFORM_SPAN = 3, 5, 300
UNIFORM_QUAL = np.array([2, 30, 41, 60, 93], dtype=np.uint8) + QUAL_OFFSET  # a function of the offset alone


def uniform_templates():
    """one batch: WG_READS reads of k + 2 bases at k = 3 (two windows each), mates forward and reverse UNIFORM_SPAN apart; a
    third unchanged, the others with one substitution at an offset that moves through the read, one with a written N"""
    assert UNIFORM_L == UNIFORM_K + 2 and len(UNIFORM_QUAL) == UNIFORM_L and UNIFORM_SPAN < LDS_LEN and WG_READS % 2 == 0
    specs = []
    for i in range(WG_READS // 2):
        lo = 4000 + 37 * i
        for mate, (at, rev) in enumerate(((lo, 0), (lo + UNIFORM_SPAN - UNIFORM_L, 1))):
            r = 2 * i + mate
            alter = {} if r % 3 == 0 else {r % UNIFORM_L: 1 + r % 3}
            if r == 7:
                alter = {2: "N"}
            specs.append((1, 0, at, UNIFORM_L, rev, alter, UNIFORM_QUAL))
    assert len(specs) == WG_READS and sum(1 for s in specs if not s[5]) >= WG_READS // 3 and any("N" in s[5].values() for s in specs)
    return specs


def uniform_batches(oracle, genomes, n_batches):
    """The batch of uniform_templates `n_batches` times, read r being template r mod WG_READS (no loop over reads): .host, the
    compact columns, and .model, what the fit of them is — the templates' counts (tests/_fit.kmerize_flat) and histograms times
    n_batches, the probabilities of those (tests/_fit.kmer_probabilities), and point masses for every density: the quality at an
    offset, the length and the span are one value each."""
    t = reads_of(oracle, genomes, uniform_templates())
    n = WG_READS * n_batches
    host = {name: np.tile(t[name], n_batches) for name in ("start", "end", "contig", "genome", "flags", "seq", "qual")}
    host["read_id"] = np.arange(n, dtype=np.uint32)
    host["seq_off"] = np.arange(n + 1, dtype=np.uint64) * np.uint64(UNIFORM_L)
    _, L, rr, j, have, want, qual = _stats.flat_reads(oracle, t, genomes)
    assert (L == UNIFORM_L).all() and set(_fit.insert_sizes(t, 2)) == {UNIFORM_SPAN}
    counts = {key: c * n_batches for key, c in _fit.kmerize_flat(UNIFORM_K, have, want, j, L[rr]).items()}
    probs = _fit.kmer_probabilities(counts, 20)
    q = qual.astype(np.int64) - QUAL_OFFSET
    assert np.array_equal(q, np.tile(UNIFORM_QUAL.astype(np.int64) - QUAL_OFFSET, WG_READS))
    m = {"qual_hist": np.bincount(j * _fit.QUALS + q, minlength=UNIFORM_L * _fit.QUALS).reshape(UNIFORM_L, _fit.QUALS).astype(np.uint64) * np.uint64(n_batches),
         "qual_density": np.array([_fit.quality_density([int(v) - QUAL_OFFSET]) for v in UNIFORM_QUAL]),
         "length_hist": np.bincount(L, minlength=_fit.MAX_L + 1).astype(np.uint64) * np.uint64(n_batches),
         "insert_hist": np.bincount(_fit.insert_sizes(t, 2), minlength=_fit.MAX_INSERT + 1).astype(np.uint64) * np.uint64(n_batches),
         "kmer_ref": np.array([r for r, _ in probs], dtype=np.uint32),
         "kmer_first": np.cumsum([0] + [len(a) for _, a in probs]).astype(np.uint64),
         "pair_alt": np.array([a for _, alts in probs for a, _, _ in alts], dtype=np.uint32),
         "pair_count": np.array([c for _, alts in probs for _, c, _ in alts], dtype=np.uint64),
         "pair_prob": np.array([p for _, alts in probs for _, _, p in alts], dtype=np.float32),
         "read_length_mean": float(UNIFORM_L), "read_length_std": 0.0, "is_long": 0, "length_bin_width": 10,
         "length_lo": np.array([UNIFORM_L], dtype=np.uint32), "length_hi": np.array([UNIFORM_L], dtype=np.uint32), "length_density": np.array([1.0]),
         "insert_size_mean": float(UNIFORM_SPAN), "insert_size_std": 0.0, "insert_bin_width": 10,
         "insert_lo": np.array([UNIFORM_SPAN], dtype=np.uint32), "insert_hi": np.array([UNIFORM_SPAN], dtype=np.uint32), "insert_density": np.array([1.0])}
    return SimpleNamespace(host=host, model=m, n_reads=n, n_batches=n_batches)


# ---- the longest read, the quality's edges -----------------------------------------------------------------------------------
def by_offset(L):
    """L quality bytes that are a function of the offset alone (every position of reads that share them is a point mass)"""
    return (QUAL_OFFSET + np.arange(L, dtype=np.int64) % 61).astype(np.uint8)


def longest_reads():
    """genome 0: MAX_L bases forward, MAX_L reverse, MAX_L - 1; .too_long is one of MAX_L + 1"""
    specs = [(0, 0, 1000, MAX_L, 0, {5: 1, MAX_L - 1: 2}, by_offset(MAX_L)), (0, 0, 200_000, MAX_L, 1, {0: 3, MAX_L - 2: "N"}, by_offset(MAX_L)),
             (0, 0, 400_000, MAX_L - 1, 0, {MAX_L - 2: 1}, by_offset(MAX_L - 1))]
    assert [s[3] for s in specs] == [65535, 65535, 65534] and place(MAX_L - 1) == (255, LANES - 1, GROUP - 2)
    return SimpleNamespace(specs=specs, too_long=[(0, 0, 600_000, MAX_L + 1, 0, {}, by_offset(MAX_L + 1))])


def quality_reads(first=None):
    """four reads of 2 LDS_POS bases whose first, LDS_POS-th and last base have quality 93 (the last offset in LDS is LDS_POS - 1,
    base LDS_POS is the first in HBM); with `first`, the quality byte of the third read's base 3 is that byte instead.
    .specs and .at, the offsets that hold 93."""
    L = 2 * LDS_POS
    at = (0, LDS_POS - 1, LDS_POS, L - 1)
    specs = []
    for r in range(4):
        q = by_offset(L)
        q[list(at)] = QUAL_OFFSET + _fit.QUALS - 1
        if first is not None and r == 2:
            q[3] = first
        specs.append((1, 1, 500 + 400 * r, L, r & 1, {9: 2}, q))
    assert all(int(q.max()) - QUAL_OFFSET == 93 for *_, q in specs) or first is not None
    return SimpleNamespace(specs=specs, at=at, L=L)
