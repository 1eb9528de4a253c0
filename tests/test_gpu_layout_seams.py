"""Depth, regions and strain (depth_kernels.hip, regions_kernels.hip, strain_kernels.hip) on the layouts at which "which contig
is this position in" is hard: thousands of short contigs with whole wave spans of one-base contigs, contig boundaries on load,
wave-span and tile starts with the array's end on a tile seam, and zero-length contigs.  Expected values come from the numpy
models (tests/_depth.py, tests/_regions.py, tests/_strain.py) alone, every comparison is exact, every size comes from the
kernels' constants, and every precondition a case rests on is asserted, so a changed constant fails here instead of hollowing a
case out.

Zero-length contigs are staged, not refused.  What the units do with one (read from the code, pinned here): it has a row with
len 0 and no windows; it shares its first position with the contig behind it, which owns that position, so it never owns a
region or a site; a read of length 0 at its offset 0 adds nothing and a longer one sets the sticky error word."""
import functools

import numpy as np
import pytest

from simmr_amd import SimmrError, _abi
from simmr_amd.engine import Engine
from tests import _depth, _regions, _strain, _synth
from tests.test_gpu_depth import column_reads, make_cols
from tests.test_gpu_regions import check
from tests.test_gpu_strain import assert_diverged

pytestmark = pytest.mark.gpu
TILE = _depth.constants()[0]
R_TILE, R_TOPS, R_RUN_TILE = _regions.constants()
CYCLE = (1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 70)
RESIDUES = (-1, 0, 1, 2, 3)
SEED = 0x0123_4567_89AB_CDEF
LAYOUTS = ["fragmented"] + [f"seam{r:+d}" for r in RESIDUES] + [f"empty{r:+d}" for r in RESIDUES]


# ---- the layouts (plain Python: tests/test_depth_host.py and tests/test_regions_host.py hold the models to their loops on them) ----
def fill(total):
    """lengths of CYCLE, the largest first, that add up to `total`"""
    out = []
    for x in sorted(CYCLE, reverse=True):
        while total >= x:
            out.append(x)
            total -= x
    return out


def fragmented_lens(tile, tiles_before=12, cycles_after=138):
    """{slot: lengths} and (index of the first one-base contig of the run, the run's length): slot 0 cycles through CYCLE up
    to 64 positions in front of depth[]'s tile `tiles_before`, then more than a quarter tile + 64 one-base contigs follow each
    other (a quarter tile is what one wave of regions_marks owns), then CYCLE again; slot 1 stays unstaged; slot 2 is five
    contigs"""
    run, start = tile // 4 + 64 + 64, tiles_before * tile - 64
    front = list(CYCLE) * (start // sum(CYCLE))
    front += fill(start - sum(front))
    return {0: front + [1] * run + list(CYCLE) * cycles_after, 2: [4097, 1, 333, 64, 1500]}, (len(front), run)


def seam_cuts(tile):
    return [255, 256, 257, 1023, 1024, 1025, tile - 1, tile, tile + 1, 2 * tile, 3 * tile - 1]


def seam_lens(tile, r, empty=False):
    """one slot of 4 * tile + r positions whose contig boundaries are seam_cuts(tile); empty: zero-length contigs first in
    the slot, between two contigs, two in a row and last in the slot"""
    cuts = seam_cuts(tile)
    assert cuts == sorted(set(cuts)) and cuts[-1] < 4 * tile + r
    lens = np.diff([0] + cuts + [4 * tile + r]).tolist()
    if empty:
        lens = [0] + lens[:2] + [0] + lens[2:5] + [0, 0] + lens[5:] + [0]
    return {0: lens}


def layout_lens(name, **small):
    if name == "fragmented":
        return fragmented_lens(TILE, **small)[0]
    return seam_lens(TILE, int(name[-2:]), name.startswith("empty"))


def layout_contigs(lens, seed):
    """ASCII contigs: ACGT with 'N' and '-' runs in the contigs of 300 positions or more, and one one-base contig that is 'N'"""
    rng = np.random.default_rng(seed)
    contigs = {}
    for g in sorted(lens):
        contigs[g] = []
        for n in lens[g]:
            seq = _strain.ACGT[rng.integers(0, 4, n)].copy()
            if n >= 300:
                seq[10:23] = ord("N")                      # crosses a plane word
                seq[n // 2:n // 2 + 30] = ord("-")
                seq[rng.integers(0, n, n // 40)] = ord("N")
                seq[-3:] = ord("-")
            contigs[g].append(seq)
    g = max(lens)
    ones = [c for c, n in enumerate(lens[g]) if n == 1]
    contigs[g][ones[-1]][0] = ord("N")
    return contigs


def layout_reads(lens, rng, n_random=3000):
    """every non-empty contig whole on both strands, one base on its first and on its last position, a read that ends exactly
    at its end, `n_random` reads inside the contigs of 16 positions or more — and a read of length 0 at offset 0 of every
    empty contig"""
    reads, big = [], []
    for g in sorted(lens):
        for c, n in enumerate(lens[g]):
            if n == 0:
                reads.append((g, c, 0, 0, c & 1))
                continue
            k = min(n, 7)
            reads += [(g, c, 0, n, 0), (g, c, 0, n, 1), (g, c, 0, 1, 0), (g, c, n - 1, 1, 1), (g, c, n - k, k, c & 1)]
            if n >= 16:
                big.append((g, c, n))
    for i in rng.integers(0, len(big), n_random):
        g, c, n = big[i]
        L = int(rng.integers(1, min(n, 400) + 1))
        reads.append((g, c, int(rng.integers(0, n - L + 1)), L, int(rng.integers(0, 2))))
    return make_cols(reads)


def boundary_depths(first, n):
    """depth[] covered on both positions beside every boundary, on the left one only, on the right one only"""
    inner = np.unique(first[(first > 0) & (first < n)])
    out = {}
    for what, at in (("both sides", np.concatenate([inner - 1, inner])), ("left side", inner - 1), ("right side", inner)):
        d = np.zeros(n, dtype=np.uint32)
        d[at] = 5
        out[what] = d
    return out


def large_depths(lens, first, n, rng):
    """0x80000000 on half of the positions, small values on the others, 0xFFFFFFFF on a whole contig: the 4097-long one if
    the layout has it, else the longest"""
    d = np.where(rng.random(n) < 0.5, 0x80000000, rng.integers(0, 10, n)).astype(np.uint32)
    flat = [x for g in sorted(lens) for x in lens[g]]
    k = flat.index(4097) if 4097 in flat else int(np.argmax(flat))
    d[first[k]:first[k + 1]] = 0xFFFFFFFF
    return d, k


# ---- engines -----------------------------------------------------------------------------------------------------------
def new_engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine(0)


class Layout:
    def __init__(self, name):
        self.name, self.lens = name, layout_lens(name)
        self.contigs = layout_contigs(self.lens, sum(map(ord, name)))
        self.flat = [x for g in sorted(self.lens) for x in self.lens[g]]
        self.first = _regions.layout(self.lens)[2]
        self.n = int(self.first[-1])
        self.cols = layout_reads(self.lens, np.random.default_rng(self.n))
        self.depth = _depth.depth(self.cols, self.lens)  # the model's, computed once and left unchanged
        self.eng = new_engine()
        for g in sorted(self.lens):  # (staged once per module: simmr_stage_genome synchronises per contig)
            self.eng.stage_genome(g, self.contigs[g])
        assert self.eng.depth_reset() == self.n


@pytest.fixture(scope="module", params=LAYOUTS)
def lay(request):
    L = Layout(request.param)
    yield L
    L.eng.close()


@pytest.fixture(scope="module")
def seng():
    """the engine whose planes the strain tests rewrite"""
    e = new_engine()
    yield e
    e.close()


# ---- what the cases rest on ---------------------------------------------------------------------------------------------
def test_the_layouts_are_what_the_cases_need():
    assert TILE == R_TILE == _strain.constants()[0] and TILE % 4 == 0 and TILE > 1026  # one placement of the seams serves the three units
    lens, (k0, run) = fragmented_lens(TILE)
    first = _regions.layout(lens)[2]
    n = int(first[-1])
    assert len(lens[0]) >= 3000 and set(lens[0]) == set(CYCLE) and 1 not in lens and 100_000 < n < 120_000
    assert run > R_TILE // 4 + 64 and lens[0][k0:k0 + run] == [1] * run
    seam = (int(first[k0]) + 64) // TILE * TILE  # the run crosses this tile start, and the wave span behind it is all boundaries
    assert int(first[k0]) == seam - 64 and seam % TILE == 0 and int(first[k0 + run]) >= seam + TILE // 4 + 64
    assert np.isin(np.arange(seam - 64, seam + TILE // 4 + 64), first).all()
    assert sorted(lens[2]).count(4097) == 1 and len(lens[2]) == 5
    for r in RESIDUES:
        for empty in (False, True):
            lens = seam_lens(TILE, r, empty)
            first = _regions.layout(lens)[2]
            assert list(lens) == [0] and int(first[-1]) == 4 * TILE + r and np.isin(seam_cuts(TILE), first).all()
            assert lens[0].count(0) == (5 if empty else 0)
            if empty:
                z = [i for i, x in enumerate(lens[0]) if x == 0]
                assert z[0] == 0 and z[-1] == len(lens[0]) - 1 and z[3] == z[2] + 1 and lens[0][z[1] - 1] and lens[0][z[1] + 1]
    assert sorted((4 * TILE + r) % 4 for r in RESIDUES) == [0, 1, 2, 3, 3] and 4 * TILE + RESIDUES[0] == 4 * TILE - 1


# ---- depth ----------------------------------------------------------------------------------------------------------------
def test_depth_and_summary(lay):
    import torch
    eng = lay.eng
    assert eng.depth_reset() == lay.n
    eng.depth_add(column_reads(eng.device, lay.cols))
    d = eng.depth()
    got, want = d.cpu().numpy(), lay.depth
    assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want), (lay.name, np.flatnonzero(got != want)[:8])
    assert want[-1] >= 3 and want.min() >= 2  # the last entry of the array, whatever n_positions & 3 is
    for w in (0, 1, 3, 64, TILE, max(lay.flat) + 1):
        s, m = eng.depth_summary(w, d), _depth.summary(want, lay.lens, w)
        _depth.assert_summary(s, m, f"{lay.name}, window {w}")
        assert int(s["hist"].sum()) == int(m["hist"].sum()) == lay.n
        if w:
            n_win = [-(-x // w) for x in lay.flat]
            assert len(s["win_sum"]) == len(m["win_sum"]) == sum(n_win) and np.array_equal(s["first_window"], np.cumsum([0] + n_win)[:-1])
            assert np.array_equal(s["first_window"], m["first_window"])
        for k in np.flatnonzero(np.array(lay.flat) == 0):  # an empty contig: a row of zeros, no windows
            assert s["len"][k] == s["covered"][k] == s["depth_sum"][k] == s["depth_max"][k] == 0
    if lay.name == "fragmented":  # window 1: every wave takes several units and leaves several contigs
        waves = 32 * torch.cuda.get_device_properties(0).multi_processor_count
        units = len(eng.depth_summary(1, d)["win_sum"])
        assert units == lay.n > waves and -(-units // waves) >= 4


def test_a_read_on_an_empty_contig(lay):
    eng = lay.eng
    empties = [(g, c) for g in sorted(lay.lens) for c, n in enumerate(lay.lens[g]) if n == 0]
    assert bool(empties) == lay.name.startswith("empty")
    for g, c in empties:
        eng.depth_reset()
        eng.depth_add(column_reads(eng.device, make_cols([(g, c, 0, 0, 0), (g, c, 0, 0, 1)])))  # length 0 at offset 0: nothing
        assert not eng.depth().cpu().numpy().any()
        eng.depth_add(column_reads(eng.device, make_cols([(g, c, 0, 1, 0)])))                   # one base: the error word
        with pytest.raises(SimmrError) as ei:
            eng.depth()
        assert ei.value.code == _abi.EINVAL
    eng.depth_reset()


# ---- regions --------------------------------------------------------------------------------------------------------------
def test_everything_covered_is_one_region_per_contig(lay):
    want = check(lay.eng, np.full(lay.n, 2, dtype=np.uint32), lay.lens, lay.contigs, 2, 1, f"{lay.name}, all covered")
    assert want["len"].tolist() == [x for x in lay.flat if x] and want["start"].max() == 0  # none merged across a boundary
    assert want["depth_sum"].tolist() == [2 * x for x in lay.flat if x]
    rows = [(g, c) for g in sorted(lay.lens) for c, x in enumerate(lay.lens[g]) if x]
    assert list(zip(want["genome"].tolist(), want["contig"].tolist())) == rows  # an empty contig owns no region
    if lay.name == "fragmented":  # sixteen regions on sixteen contigs inside one 16-byte chunk of the base stream
        chunk = want["seq_off"][:-1] // 16
        assert np.bincount(chunk.astype(np.int64)).max() == 16


@pytest.mark.parametrize("min_len", [1, 2])
@pytest.mark.parametrize("p", [0.5, 0.95])
def test_random_coverage(lay, p, min_len):
    rng = np.random.default_rng(int(p * 100) + min_len)
    d = (rng.random(lay.n) < p).astype(np.uint32) * rng.integers(1, 9, lay.n).astype(np.uint32)
    want = check(lay.eng, d, lay.lens, lay.contigs, 1, min_len, (lay.name, p, min_len))
    assert want["len"].size > 100 and (min_len > 1 or int(want["len"].sum()) == int((d > 0).sum()))


def test_covered_beside_every_boundary(lay):
    inner = np.unique(lay.first[(lay.first > 0) & (lay.first < lay.n)])
    for what, d in boundary_depths(lay.first, lay.n).items():
        want = check(lay.eng, d, lay.lens, lay.contigs, 1, 1, (lay.name, what))
        assert int(want["len"].sum()) == int((d > 0).sum()) and want["len"].size >= inner.size
        if what == "right side":
            assert want["start"].max() == 0 and want["len"].max() == 1
    want = check(lay.eng, boundary_depths(lay.first, lay.n)["both sides"], lay.lens, lay.contigs, 1, 2, (lay.name, "both sides, min_len 2"))
    assert set(want["len"].tolist()) <= {2}  # two-base contigs alone: a run is never longer than its contig


def test_large_depth_values(lay):
    d, k = large_depths(lay.lens, lay.first, lay.n, np.random.default_rng(9))
    for md in (0x80000000, 0xFFFFFFFF):
        want = check(lay.eng, d, lay.lens, lay.contigs, md, 1, (lay.name, hex(md)))
        assert int(want["depth_sum"].max()) > 1 << 32 and int(want["len"].max()) == lay.flat[k] >= 4095
    assert want["len"].size == 1 and int(want["depth_sum"][0]) == 0xFFFFFFFF * lay.flat[k]
    assert bool((d >> 31).any()) and check(lay.eng, d, lay.lens, lay.contigs, 1, 1, (lay.name, "large, min_depth 1"))["len"].size > 100


def test_regions_of_the_engines_own_depth(lay):
    eng = lay.eng
    eng.depth_reset()
    eng.depth_add(column_reads(eng.device, lay.cols))
    for md in (1, 3, 4):
        want = _regions.regions(lay.depth, lay.lens, md, 1)
        got = eng.regions(md, 1)
        _regions.assert_regions(got, want, (lay.name, "chained", md))
        assert np.array_equal(got["seq"].cpu().numpy(), _regions.bases(want, lay.contigs))
    assert want["len"].size > 10


def test_the_run_counts_take_a_second_scan_iteration():
    """k_regions_scan scans the counts of k_regions_flag's workgroups (REGIONS_RUN_TILE runs each) REGIONS_TOPS_WIDTH at a
    time: a depth[] that alternates 1, 0 makes more run workgroups than one iteration takes"""
    host = (_strain.ROOT / "simmr_amd" / "csrc" / "regions.hip").read_text()
    assert "hipLaunchKernelGGL(k_regions_scan, dim3(2), dim3(REGIONS_WG), 0, st, s->run_count.as<const uint64_t>()" in host
    assert "run_tiles = (n_runs + REGIONS_RUN_TILE - 1) / REGIONS_RUN_TILE" in host
    seam = R_RUN_TILE * R_TOPS  # the first run of the second iteration
    n = 2 * (seam + 3 * R_RUN_TILE) + 77
    lens = {0: [n]}
    d = np.zeros(n, dtype=np.uint32)
    d[0::2] = 1
    d[1000:1007] = 1                                           # a run of 7 in the first iteration
    x = int(_regions.regions(d, lens)["start"][seam])
    d[x:x + 7] = 1                                             # ... and one that is run `seam`
    eng = new_engine()
    try:
        eng.stage_synthetic(0, [n], 5)
        assert eng.depth_reset() == n
        contigs = {0: _synth.synthetic_contigs_chunked([n], 5)}
        want = check(eng, d, lens, contigs, 1, 1, "alternating, min_len 1")
        assert -(-want["len"].size // R_RUN_TILE) > R_TOPS and int(want["start"][seam]) == x and int(want["len"][seam]) == 7
        want = check(eng, d, lens, contigs, 1, 2, "alternating, min_len 2")
        assert want["start"].tolist() == [1000, x] and want["len"].tolist() == [7, 7]
    finally:
        eng.close()


# ---- strain ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def strain_contigs(name):
    lens = layout_lens(name)
    return lens[0], layout_contigs(lens, sum(map(ord, name)))[0]


@pytest.mark.parametrize("identity", [1.0, 0.97, 0.25])
@pytest.mark.parametrize("name", [x for x in LAYOUTS if not x.startswith("seam")])
def test_strain(seng, name, identity):
    lens, contigs = strain_contigs(name)
    want = assert_diverged(seng, 0, contigs, identity, SEED, f"{name} at {identity}")
    assert (want["pos"].size == 0) == (identity == 1.0)
    ln = np.array(lens, dtype=np.uint64)
    assert (want["pos"] < ln[want["contig"]]).all()  # never in the padding, never on an empty contig
    if identity == 0.25:
        ones = np.flatnonzero(ln == 1)
        assert np.isin(ones, want["contig"]).any()  # a contig whose plane slot is one base and 63 of padding
        if name == "fragmented":
            assert ones.size > 1000 and np.isin(ones, want["contig"]).sum() > ones.size // 2
            assert (want["contig"] > 2048).any() and int(want["contig"].max()) > len(lens) - 20
