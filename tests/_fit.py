"""The model-fitting rules of include/simmr_hip.h (simmr_fit_*) restated in plain Python / numpy — TEST INFRASTRUCTURE ONLY.

Written from simmrd/src/alignment.rs (encoded_kmerize_alignment), simmrd/src/probability.rs and shared/src/util.rs as read:
the k-mer rule with its gap branches (`kmerize_alignment`, which the device never needs but the CPU test shows whole), the
population mean / deviation folds in observation order, the Gaussian kernel density, the Freedman-Diaconis width and the two
bin builders — and the one documented departure, the point mass where the bandwidth is 0.  `model` applies them to the
oracle's reads and the host genome bytes (tests/_stats.flat_reads: the expected-byte model of tests/_truth.py).  Nothing
here comes from the code under test."""
import math
import re
from pathlib import Path

import numpy as np

from tests import _stats

QUALS, DENSITIES, MAX_L, MAX_INSERT = 94, 71, 65535, 5000
ACGT = b"ACGT"
CONSTANTS = ("FIT_LANES", "FIT_WG_READS", "FIT_FLUSH_BATCHES", "FIT_LDS_POS", "FIT_LDS_LEN", "FIT_LDS_K", "FIT_MAX_PROBE", "FIT_MAX_L")


def constants():
    """{name: value} of CONSTANTS as fit_device.hpp states them: what tests/_fit_cases.py and tests/test_gpu_fit_seams.py size
    their cases from"""
    src = (Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc" / "fit_device.hpp").read_text()
    return {n: int(re.search(rf"#define {n} (\d+)u\b", src).group(1)) for n in CONSTANTS}


def encode3(kmer: bytes):
    """three_bit_encode_kmer: base i at bits 3 i, A C G T N = 0 1 2 3 4; None where the reference's encoder fails"""
    code = 0
    for i, ch in enumerate(kmer):
        at = b"ACGTN".find(bytes([ch]))
        if at < 0:
            return None
        code |= at << (3 * i)
    return code


def kmerize_alignment(k, reference: bytes, query: bytes, counts=None):
    """count[(ref, alt)] of one alignment (two rows of equal length, '-' for a gap in either): every window ndx with
    ndx + k < length; a reference window that starts with a gap, or holds a gap or a byte outside ACGT, is skipped; the query
    window loses its gaps and its N and is padded with N; an empty one is skipped; a window adds (ref, ref) and (ref, query)."""
    counts = {} if counts is None else counts
    n = len(reference)
    assert len(query) == n
    for ndx in range(n):
        if not ndx + k < n:
            break
        if reference[ndx] == ord("-"):
            continue
        ref = bytes(c for c in reference[ndx:ndx + k] if c != ord("-") and c in ACGT)
        qry = bytes(c for c in query[ndx:ndx + k] if c != ord("-") and c != ord("N"))
        if len(ref) != k or not qry:
            continue
        r = encode3(ref)
        if r is None:
            continue
        q = encode3(qry + b"N" * (k - len(qry)))
        if q is None:
            continue
        counts[(r, r)] = counts.get((r, r), 0) + 1
        counts[(r, q)] = counts.get((r, q), 0) + 1
    return counts


def kmerize_flat(k, have, want, j, L_of_base):
    """the same counts for GAPLESS alignments laid end to end (have / want: the written and expected byte of every base, j its
    offset in its read, L_of_base its read's length), vectorised; windows with an N or '-' written go through the plain rule"""
    counts = {}
    n = have.size
    if n < k:
        return counts
    wc = np.full(256, 4, dtype=np.int64)
    wc[list(ACGT)] = [0, 1, 2, 3]
    hc = np.full(256, 5, dtype=np.int64)
    hc[list(ACGT)] = [0, 1, 2, 3]
    hc[[ord("N"), ord("-")]] = 4
    w, h = wc[want], hc[have]
    win = lambda a: np.lib.stride_tricks.sliding_window_view(a, k)
    starts = np.arange(n - k + 1)
    inside = j[starts] + k < L_of_base[starts]
    shifts = 3 * np.arange(k, dtype=np.int64)
    ww, hh = win(w), win(h)
    ok = inside & (ww < 4).all(axis=1) & (hh < 5).all(axis=1)
    gap = ok & (hh == 4).any(axis=1)
    plain = ok & ~gap
    ref = (ww[plain] << shifts).sum(axis=1)
    alt = (hh[plain] << shifts).sum(axis=1)
    for keys in (ref << 32 | ref, ref << 32 | alt):
        u, c = np.unique(keys, return_counts=True)
        for key, cnt in zip(u.tolist(), c.tolist()):
            kk = (key >> 32, key & 0xffffffff)
            counts[kk] = counts.get(kk, 0) + cnt
    for s in np.flatnonzero(gap).tolist():
        # (one more base on either row: the plain rule leaves the LAST window of what it is given out)
        kmerize_alignment(k, bytes(want[s:s + k].tolist()) + b"A", bytes(have[s:s + k].tolist()) + b"A", counts)
    return counts


def kmer_probabilities(counts, max_alt):
    """[(ref, [(alt, count, f32 probability)])], reference k-mers ascending; alternates by count descending, ties by code
    ascending, cut to max_alt without renormalising"""
    by_ref = {}
    for (r, a), c in counts.items():
        by_ref.setdefault(r, []).append((a, c))
    out = []
    for r in sorted(by_ref):
        alts = sorted(by_ref[r], key=lambda t: (-t[1], t[0]))
        total = np.float32(sum(c for _, c in alts))
        out.append((r, [(a, c, np.float32(c) / total) for a, c in alts[:max_alt]]))
    return out


def mean(xs):
    acc = 0.0
    for v in xs:
        acc += v
    return acc / len(xs)


def std_deviation(xs):
    avg = mean(xs)
    acc = 0.0
    for v in xs:
        acc += (v - avg) * (v - avg)
    return math.sqrt(acc / len(xs))


def bandwidth(xs):
    return 1.06 * std_deviation(xs) * float(len(xs)) ** (-1.0 / 5.0)


def gaussians(points, xs, bw):
    """probability.rs `gaussian` at every point, each folding over the observations in their order (numpy's cumulative sum is that
    fold)"""
    f = (np.asarray(points, dtype=np.float64)[:, None] - np.asarray(xs, dtype=np.float64)[None, :]) / bw
    return (np.cumsum(np.exp(-0.5 * f ** 2), axis=1)[:, -1] / (math.sqrt(2.0 * math.pi) * len(xs) * bw)).tolist()


def quality_density(scores):
    """71 densities of one position; bandwidth 0: the point mass, a score above 70 at entry 70"""
    xs = [float(s) for s in scores]
    bw = bandwidth(xs)
    if bw == 0.0:
        return [1.0 if s == min(int(xs[0]), 70) else 0.0 for s in range(DENSITIES)]
    return gaussians(np.arange(DENSITIES), xs, bw)


def quartile_indices(n):
    return int(math.floor(n * 0.25)), int(math.floor(n * 0.75))


def freedman_diaconis(sorted_xs):
    n = len(sorted_xs)
    i1, i3 = quartile_indices(n)
    iqr = sorted_xs[i3] - sorted_xs[i1]
    return int(2.0 * (iqr / float(n) ** (1.0 / 3.0)))


def bins(xs, clamp_ends):
    """(width, [(lo, hi)], [density]) of create_read_length_bins (clamp_ends) / create_insert_size_bins over the observations xs in
    their order; min == max: ONE bin (min, min) of density 1.0"""
    xs = [float(v) for v in xs]
    fd = freedman_diaconis(sorted(xs))
    width = fd if fd > 1 else 10
    lo, hi = min(xs), max(xs)
    if lo == hi:
        return width, [(int(lo), int(lo))], [1.0]
    num = int(math.ceil((hi - lo) / width))
    ranges = []
    for i in range(num):
        start, end = int(lo) + i * width, int(lo) + (i + 1) * width - 1
        ranges.append((start, min(end, int(hi)) if clamp_ends else end))
    bw = bandwidth(xs)
    return width, ranges, gaussians([(s + e) / 2.0 for s, e in ranges], xs, bw)


def insert_sizes(o, n_sets):
    """|TLEN| once per mate (the span of the pair), values above 5000 left out, in read order"""
    if n_sets != 2:
        return []
    st, en = o["start"].astype(np.int64), o["end"].astype(np.int64)
    lo, hi = np.minimum(st, en), np.maximum(st, en)
    span = np.maximum(hi[0::2], hi[1::2]) - np.minimum(lo[0::2], lo[1::2])
    span = np.repeat(span, 2)
    return span[span <= MAX_INSERT].tolist()


def model(lib, shards, genomes, n_sets, qual_offset, k, max_alt):
    """what Engine.fit_model() answers for the reads of `shards` (a list of compact host column dicts)"""
    counts, scores, lengths, inserts = {}, {}, [], []
    for o in shards:
        n, L, rr, j, have, want, qual = _stats.flat_reads(lib, o, genomes)
        for key, c in kmerize_flat(k, have, want, j, L[rr]).items():
            counts[key] = counts.get(key, 0) + c
        q = (qual.astype(np.int64) - qual_offset) & 255
        assert q.size == 0 or q.max() < QUALS
        order = np.argsort(j, kind="stable")
        jj, qq = j[order], q[order]
        cuts = np.flatnonzero(np.diff(jj)) + 1
        for pos, part in zip(jj[np.r_[0, cuts]].tolist() if jj.size else [], np.split(qq, cuts)):
            scores.setdefault(pos, []).extend(part.tolist())
        lengths += L.tolist()
        inserts += insert_sizes(o, n_sets)
    n_pos = max(lengths) if lengths else 0
    m = {"qual_hist": np.zeros((n_pos, QUALS), dtype=np.uint64), "qual_density": np.zeros((n_pos, DENSITIES))}
    for pos in range(n_pos):
        m["qual_hist"][pos] = np.bincount(scores[pos], minlength=QUALS)
        m["qual_density"][pos] = quality_density(scores[pos])
    probs = kmer_probabilities(counts, max_alt)
    m["kmer_ref"] = np.array([r for r, _ in probs], dtype=np.uint32)
    m["kmer_first"] = np.cumsum([0] + [len(a) for _, a in probs]).astype(np.uint64)
    m["pair_alt"] = np.array([a for _, alts in probs for a, _, _ in alts], dtype=np.uint32)
    m["pair_count"] = np.array([c for _, alts in probs for _, c, _ in alts], dtype=np.uint64)
    m["pair_prob"] = np.array([p for _, alts in probs for _, _, p in alts], dtype=np.float32)
    m["length_hist"] = np.bincount(lengths, minlength=MAX_L + 1).astype(np.uint64)
    m["insert_hist"] = np.bincount(inserts, minlength=MAX_INSERT + 1).astype(np.uint64)
    m["read_length_mean"], m["read_length_std"] = mean(lengths), std_deviation(lengths)
    m["is_long"] = int(m["read_length_mean"] > 400.0)
    m["length_bin_width"], ranges, dens = bins(sorted(lengths), True)
    m["length_lo"], m["length_hi"] = (np.array([r[i] for r in ranges], dtype=np.uint32) for i in (0, 1))
    m["length_density"] = np.array(dens)
    m["insert_size_mean"], m["insert_size_std"] = (mean(inserts), std_deviation(inserts)) if inserts else (0.0, 0.0)
    ranges, dens = [], []
    if inserts and not m["is_long"]:
        m["insert_bin_width"], ranges, dens = bins(inserts, False)
    m["insert_lo"], m["insert_hi"] = (np.array([r[i] for r in ranges], dtype=np.uint32) for i in (0, 1))
    m["insert_density"] = np.array(dens, dtype=np.float64)
    return m


EXACT = ("kmer_ref", "kmer_first", "pair_alt", "pair_count", "pair_prob", "qual_hist", "length_hist", "insert_hist", "length_lo",
         "length_hi", "insert_lo", "insert_hi")
CLOSE = ("qual_density", "length_density", "insert_density")
SCALARS_EXACT = ("is_long", "length_bin_width")
SCALARS_CLOSE = ("read_length_mean", "read_length_std", "insert_size_mean", "insert_size_std")


def assert_close(got, want, what):
    """relative 1e-6, or absolute 1e-290 where the value is in the underflow range (the tolerance the issue derives: a reordered
    f64 fold of n terms moves the bandwidth by about n 2^-52, the exponent is at most about 745, so a density moves by at most
    about 1500 n 2^-52 = 3e-8 at n <= 1e5; 1e-6 leaves a factor of 30 for exp itself).  No entry is skipped."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, the model has {want.shape}"
    bad = ~((np.abs(got - want) <= 1e-6 * np.abs(want)) | (np.abs(got - want) <= 1e-290))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}{list(map(int, i))} is {got[i]!r}, the model has {want[i]!r} ({np.count_nonzero(bad)} entries differ)")


def assert_model(got, want, what=""):
    for name in EXACT:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, the model {w.shape}"
        assert g.dtype == w.dtype, f"{what}: {name} is {g.dtype}"
        if not np.array_equal(g, w):
            i = tuple(np.argwhere(g != w)[0])
            raise AssertionError(f"{what}: {name}{list(map(int, i))} is {g[i]}, the model has {w[i]} ({np.count_nonzero(g != w)} entries differ)")
    for name in CLOSE:
        assert_close(got[name], want[name], f"{what}: {name}")
    for name in SCALARS_EXACT:
        assert int(got[name]) == int(want[name]), f"{what}: {name} is {got[name]}, the model has {want[name]}"
    if len(want["insert_lo"]):
        assert int(got["insert_bin_width"]) == int(want["insert_bin_width"]), what
    for name in SCALARS_CLOSE:
        assert_close([got[name]], [want[name]], f"{what}: {name}")
