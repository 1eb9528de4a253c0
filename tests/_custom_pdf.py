"""Short-read custom models whose per-position tables have a chosen shape, and a property of the qualities they can give.

k_emit_custom_pe and the custom branch of k_plan_pe (csrc/kernels.hip) branch on the shape of the user's model: the number
of densities and of bin ranges of every PDF (one register per lane up to 64 entries, two up to 128, a gather above), the
position of a PDF's header (LDS up to CUSTOM_LDS_PDFS, memory behind), a bin's width (one score, a range that rejects
words, the whole u32).  shaped_model() builds such models on model_io.serialize_model; CASES are the directed cases of
tests/test_gpu_custom_short.py, run against the oracle alone by tests/test_custom_short_models_host.py; sweep_case() is
the generator of the random sweep of both files.

allowed_scores() / qualities_allowed() state, from the model alone, which bytes a read position may carry: the scores of
the bins of positive density of PDF min(p, n_quality - 1) (custom_short.rs:328-350; WeightedAliasIndex never returns an
index of weight zero), taken `as u8`.  Both mates' qualities are in read order (simulate.rs:265-266; only the bases of
mate 2 are reversed, :283).  It shares nothing with oracle/custom.c: a gather from another PDF, bin or lane fails it
even where the oracle made the same mistake."""
import ctypes as C

import numpy as np

from simmr_amd.model_io import serialize_model
from tests import _synth

FULL = (0, 0xFFFFFFFF)
PAIRS = 323  # one full workgroup (256), one full wave (64), one wave of three lanes
READS = 2 * PAIRS
THREADS = 8  # OpenMP threads of the oracle's pair loops (its results do not depend on them)


class Model:
    """blob + what it was made from: quality = [(density, ranges)] per position, length / insert = (density, ranges)"""

    def __init__(self, quality, length, insert, len_mean, ins_mean):
        self.quality, self.length, self.insert = quality, length, insert
        self.len_mean, self.ins_mean = float(len_mean), float(ins_mean)
        self.blob = serialize_model(quality, length, insert, read_length_mean=self.len_mean, insert_size_mean=self.ins_mean)
        self.required = int(2.0 * self.len_mean + self.ins_mean)  # custom_short.rs:535-538

    @property
    def n_quality(self):
        return len(self.quality)

    def profile(self):
        from simmr_amd import CustomShortErrorProfile
        return CustomShortErrorProfile(self.blob)  # (keep it: the POD points into its buffer)


def flat_pdf(rng, lo, hi, width=1):
    """bins (lo, lo + width - 1), ... up to hi inclusive, random positive densities"""
    edges = list(range(lo, hi + 1, width))
    d = rng.uniform(0.5, 1.5, len(edges))
    return list(d / d.sum()), [(e, min(e + width - 1, hi)) for e in edges]


def quality_pdf(rng, n_density, n_bins, zeros=3, wider=0, rejecting=False, full_weight=0.0, keep=None):
    """One position's (density, ranges): random positive densities with `zeros` exact zeros, ranges (i, i); `wider` of
    them (i, i + 1..3); rejecting: every range about 2^31 + k scores wide; full_weight > 0: one bin (0, 0xFFFFFFFF) of that
    weight; keep: the only bin indices whose density stays positive.  Densities beyond the ranges are 0.0 (simmrd writes
    one more density than ranges, probability.rs:162-166): no sample can pick them."""
    live = min(n_density, n_bins)
    d = np.zeros(n_density)
    d[:live] = rng.uniform(0.05, 1.0, live)
    if keep is not None:
        mask = np.zeros(n_density, bool)
        mask[[k for k in keep if k < live]] = True
        d[~mask] = 0.0
    elif live > 4:
        d[rng.choice(live, size=min(zeros, live - 2), replace=False)] = 0.0
    ranges = [(i, i) for i in range(n_bins)]
    if rejecting:
        ranges = [(i, 2 ** 31 + i + int(rng.integers(1, 1000))) for i in range(n_bins)]
    elif wider and n_bins > 4:
        for i in rng.choice(n_bins, size=min(wider, n_bins), replace=False):
            ranges[int(i)] = (int(i), int(i) + int(rng.integers(1, 4)))
    if d.sum() == 0.0:
        d[0] = 1.0
    d = d / d.sum()
    if full_weight > 0.0 and live >= 2:
        at = int(rng.integers(0, live))
        d[at] = 0.0
        d = d / d.sum() * (1.0 - full_weight)
        d[at] = full_weight
        ranges[at] = FULL
    return [float(x) for x in d], ranges


def shaped_model(widths, seed, length, insert, len_mean, ins_mean, wider=0, rejecting=False, full_at=(), full_weight=0.3,
                 keep=None):
    """widths: (n_density, n_bins) per read position; length / insert: (density, ranges), insert None for a model
    without insert bins; full_at: positions with a full-range bin; keep(p): see quality_pdf."""
    rng = np.random.default_rng(seed)
    quality = [quality_pdf(rng, n, nb, wider=wider, rejecting=rejecting, full_weight=full_weight if p in full_at else 0.0,
                           keep=None if keep is None else keep(p)) for p, (n, nb) in enumerate(widths)]
    return Model(quality, length, insert, len_mean, ins_mean)


def allowed_scores(model, p):
    """(mask, every): mask[b] is True when read position p may carry raw quality byte b; every is True when a bin of
    positive density spans 256 scores or more (a full-range bin among them), so that the position allows every byte."""
    density, ranges = model.quality[min(p, model.n_quality - 1)]
    n = min(len(density), len(ranges))  # (a density without a range has no score: picking it is an error)
    mask = np.zeros(256, bool)
    if n:
        r = np.asarray(ranges[:n], dtype=np.int64)
        live = np.asarray(density[:n]) > 0.0
        lo, hi = r[live, 0], r[live, 1]
        one = lo == hi
        mask[lo[one] & 0xff] = True
        for a, b in zip(lo[~one].tolist(), hi[~one].tolist()):
            if b - a >= 255:
                mask[:] = True
            else:
                mask[np.arange(a, b + 1) & 0xff] = True
    return mask, bool(mask.all())


def qualities_allowed(model, cols, qual_offset):
    """The property on one run's columns (seq_off, qual): every quality byte minus the offset, mod 256, at read position p
    of either mate is an allowed score of p.  Returns the number of bytes at positions that allow every byte (skipped)."""
    table = np.stack([allowed_scores(model, p)[0] for p in range(model.n_quality)])
    off = cols["seq_off"].astype(np.int64)
    lens = np.diff(off)
    assert off[-1] == cols["qual"].size
    pos = np.arange(cols["qual"].size, dtype=np.int64) - np.repeat(off[:-1], lens)
    raw = (cols["qual"].astype(np.int64) - qual_offset) % 256
    pdf = np.minimum(pos, model.n_quality - 1)
    ok = table[pdf, raw]
    if not ok.all():
        bad = np.flatnonzero(~ok)
        r = np.searchsorted(off, bad[:6], side="right") - 1
        raise AssertionError(f"{bad.size} of {ok.size} quality bytes are not scores of their position's PDF; first: "
                             f"reads {r.tolist()} positions {pos[bad[:6]].tolist()} scores {raw[bad[:6]].tolist()}")
    return int(table.all(axis=1)[pdf].sum())


def case_genome(seed):
    """3 contigs of 6 000 to 20 000 bases, the second with scattered N and '-' (the copy-only base kernel then also reads
    an exception plane)"""
    rng = np.random.default_rng(1000 + seed)
    lens = [int(x) for x in rng.integers(6000, 20001, 3)]
    contigs = _synth.synthetic_contigs(lens, 500 + seed)
    c = contigs[1].copy()
    c[rng.integers(0, c.size, c.size // 25)] = ord("N")
    c[rng.integers(0, c.size, 25)] = ord("-")
    contigs[1] = c
    return contigs


# ---- the directed cases ----------------------------------------------------------------------------------------------
LADDER = [(1, 1), (63, 63), (64, 64), (65, 65), (64, 65), (65, 64), (127, 128), (128, 128), (129, 129), (128, 129), (129, 128),
          (40, 100), (100, 40), (300, 300), (71, 70)]
MIXED = [(70, 70), (200, 200), (3, 3), (129, 64), (64, 129)]


def is_narrow(w):
    return w[0] <= 128 and w[1] <= 128  # (kernels.hip: k_emit_custom_pe, `narrow`)


def ladder_model(n, nb, seed=11, lo=40, hi=90, positions=60):
    """(a): one width at all 60 positions; lengths lo..hi pass n_quality"""
    rng = np.random.default_rng(seed)
    return shaped_model([(n, nb)] * positions, seed + n * 1000 + nb, flat_pdf(rng, lo, hi), flat_pdf(rng, 60, 260, 10), hi, 260, wider=5)


def lds_edge_model(n_quality):
    """(c): 70-wide PDFs, position p with scores {2 (p % 35), 2 (p % 35) + 1} only — neighbouring positions share no
    score — and lengths 500..530 in one-wide bins: the headers behind the LDS image (2 + p >= 512) and the clamp at
    n_quality - 1 are both reached"""
    rng = np.random.default_rng(21)
    return shaped_model([(70, 70)] * n_quality, 22, flat_pdf(rng, 500, 530), flat_pdf(rng, 400, 900, 20), 530, 900,
                        keep=lambda p: (2 * (p % 35), 2 * (p % 35) + 1))


def _std(seed, widths, **kw):
    """60 (or len(widths)) positions, lengths 40..90, inserts 60..260 in 10-wide bins"""
    rng = np.random.default_rng(seed)
    return shaped_model(widths, seed, flat_pdf(rng, 40, 90), flat_pdf(rng, 60, 260, 10), 90, 260, **kw)


def _with_pdfs(seed, length, insert, len_mean, ins_mean, widths=None, **kw):
    rng = np.random.default_rng(seed)
    return shaped_model(widths or [(70, 70)] * 60, seed, length(rng), insert(rng) if insert else None, len_mean, ins_mean, **kw)


def _cases():
    c = {}
    for n, nb in LADDER:
        c[f"a-ladder-{n}-{nb}"] = lambda n=n, nb=nb: ladder_model(n, nb)
    c["b-mixed"] = lambda: _std(12, [MIXED[p % 5] for p in range(60)], wider=5)
    for nq in (515, 511, 512):
        c[f"c-lds-edge-{nq}"] = lambda nq=nq: lds_edge_model(nq)
    c["d-divergent"] = lambda: _with_pdfs(14, lambda r: ([0.5, 0.5], [(1, 16), (480, 520)]), lambda r: flat_pdf(r, 400, 900, 20),
                                          520, 900, widths=[(70, 70)] * 100, wider=5)
    c["e-full-range"] = lambda: _std(15, [(70, 70)] * 60, full_at=(0, 7, 16, 33, 59))
    c["f-rejecting-wide"] = lambda: _std(16, [(200, 200)] * 60, rejecting=True)
    c["g-as-u16"] = lambda: _with_pdfs(17, lambda r: flat_pdf(r, 65536 + 90, 65536 + 140), lambda r: flat_pdf(r, 65536 + 100, 65536 + 300),
                                       140, 300, wider=5)
    c["h-no-insert"] = lambda: _with_pdfs(18, lambda r: flat_pdf(r, 40, 100), None, 100, 0, wider=5)
    c["i-wide-length-insert"] = lambda: _with_pdfs(19, lambda r: flat_pdf(r, 30, 199), lambda r: flat_pdf(r, 50, 249), 199, 249, wider=5)
    return c


CASES = _cases()
QOFF = {"e-full-range": (0, 200)}  # qual_offset per case; 33 elsewhere


def case_inputs(name):
    """(model, contigs, seed) of a directed case: the same on the CPU (oracle alone) and on the device"""
    k = list(CASES).index(name)
    return CASES[name](), case_genome(k), 4000 + 17 * k


def full_range_length_model():
    """a full-range bin in the LENGTH PDF: L is a random u16, far past every contig here — both sides refuse"""
    rng = np.random.default_rng(23)
    return shaped_model([(70, 70)] * 60, 23, ([0.5, 0.5], [(50, 60), FULL]), flat_pdf(rng, 60, 260, 10), 60, 260)


def bad_bin_model(n):
    """(k): density n - 1 has no range and all the weight (test_custom_short_rejects_bad_models' case at width n)"""
    d = [0.0] * (n - 1) + [1.0]
    return Model([(d, [(30 + i % 40, 30 + i % 40) for i in range(n - 1)])] * 50, ([1.0], [(100, 100)]), None, 100, 0)


# ---- the random sweep ------------------------------------------------------------------------------------------------
SWEEP_WIDTHS = [1, 2, 63, 64, 65, 70, 128, 129, 200]


def sweep_case(rng):
    """One iteration's draw: dict(model, contigs, reads, seed, first, count, qoff)"""
    n_quality = int(rng.integers(1, 601))
    n_shapes = int(rng.integers(1, 5))  # a few shapes, cycled: neighbouring positions differ, 600 PDFs stay cheap to build
    shapes = []
    for _ in range(n_shapes):
        n = int(rng.choice(SWEEP_WIDTHS))
        nb = n - 1 if (n > 1 and rng.random() < 0.4) else n
        kind = rng.random()
        shapes.append(((n, nb), dict(wider=4 if kind < 0.5 else 0, rejecting=0.5 <= kind < 0.65,
                                     full_weight=0.25 if kind >= 0.9 else 0.0)))
    quality = []
    for p in range(n_quality):
        (n, nb), kw = shapes[p % n_shapes]
        quality.append(quality_pdf(rng, n, nb, **kw))
    lo = int(rng.integers(1, 540))
    hi = min(560, lo + int(rng.integers(0, 120)))
    length = flat_pdf(rng, lo, hi, int(rng.choice([1, 1, 5])))
    insert, ins_max = None, 0
    if rng.random() < 0.75:
        ilo = int(rng.integers(0, 400))
        ins_max = ilo + int(rng.integers(0, 300))
        insert = flat_pdf(rng, ilo, ins_max, int(rng.choice([1, 10])))
    # (mostly the largest draws, so that `required` covers every pair; sometimes the simmrd-like means, where a pair near
    # a contig's end can run past it: a refusal, which must be mutual)
    tight = rng.random() < 0.12
    model = Model(quality, length, insert, (lo + hi) / 2 if tight else hi, ins_max / 2 if tight else ins_max)
    nc = int(rng.integers(1, 4))
    lens = [int(rng.integers(1500, 30_000)) for _ in range(nc)]
    contigs = _synth.synthetic_contigs(lens, int(rng.integers(1, 1 << 30)))
    if rng.random() < 0.4:
        c = contigs[0].copy()
        c[rng.integers(0, c.size, c.size // 20)] = ord("N")
        c[rng.integers(0, c.size, 30)] = ord("-")
        contigs[0] = c
    reads = int(rng.integers(0, 701))
    return dict(model=model, contigs=contigs, reads=reads, seed=int(rng.integers(0, 1 << 62)),
                first=int(rng.integers(0, reads // 2 + 2)), count=int(rng.integers(0, 400)), qoff=int(rng.choice([0, 33, 100])))


# ---- the oracle's model reader (oracle/oracle.h: orc_bins, orc_model) ---------------------------------------------------
class OrcBins(C.Structure):
    _fields_ = [("num_bins", C.c_uint64), ("bin_width", C.c_uint64), ("n_density", C.c_uint64), ("n_ranges", C.c_uint64),
                ("density", C.POINTER(C.c_double)), ("range_lo", C.POINTER(C.c_uint32)), ("range_hi", C.POINTER(C.c_uint32))]

    def lists(self):
        return ([self.density[i] for i in range(self.n_density)],
                [(self.range_lo[i], self.range_hi[i]) for i in range(self.n_ranges)])


class OrcModel(C.Structure):
    _fields_ = [("bin_size", C.c_uint64), ("n_quality", C.c_uint64), ("quality", C.POINTER(OrcBins)),
                ("bit_encoding", C.c_uint8), ("kmer_size", C.c_uint64), ("n_prob", C.c_uint64),
                ("prob_kmer", C.c_void_p), ("prob_n", C.c_void_p), ("prob_alt", C.c_void_p), ("prob_w", C.c_void_p),
                ("insert_size_mean", C.c_double), ("insert_size_std", C.c_double), ("has_insert_bins", C.c_uint8),
                ("insert_bins", OrcBins), ("read_length_mean", C.c_double), ("read_length_std", C.c_double),
                ("read_length_bins", OrcBins), ("is_long", C.c_uint8)]


def parse_with_oracle(lib, blob):
    m = OrcModel()
    lib.orc_model_parse.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(OrcModel)]
    assert lib.orc_model_parse(blob, len(blob), C.byref(m)) == 0
    return m
