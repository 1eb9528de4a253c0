"""The true overlaps of the device (simmr_overlap_*, include/simmr_hip.h) past the second level of their scans, of the radix
sort and of their capped grids, against tests/_overlap.py and its restatements by index and by digit counts (tests/_seams.py,
held to the model by tests/test_seams_host.py).  Every comparison is exact, every expected value is the models'.

Which loop each test is the first to enter (the `chain` is about 2.1 M reads on 256 CUs, each overlapping its next neighbours):
  test_chain_columns_and_plan
      k_samsort_digit_scan (sam_sort_kernels.hip), reached through samsort_sort_pairs: the loop over 256 tiles at a time with
      its carry, second to fifth iteration (more than 256 tiles of SAMSORT_TILE pairs), in each of the five passes of a 34-bit key;
      k_ovl_partners and k_ovl_offsets (overlap_kernels.hip): the loop of a workgroup over read chunks (more chunks of SAM_CHUNK
      than OVL_WGS_PER_CU workgroups per CU);
      sam_scan_chunks (sam_kernels.hip) through the first launch of k_ovl_scan, over the partner counts: past 256 chunks, many times;
      and through its second launch, over the record bytes: past 256 chunks of OVL_CHUNK records;
  test_chain_text_windows
      k_ovl_write for runs that start and end inside the second level: around place 256 x SAM_CHUNK, around the place whose
      records hold record 256 x OVL_CHUNK, and at the end of the places;
  test_chain_window_sizes
      k_ovl_window: the binary search over chunk prefixes with more than 256 prefixes, for a budget that starts before record
      256 x OVL_CHUNK and ends behind it;
  test_pile_730_text_columns_and_pieces, test_pile_730_exact_capacity_between_canaries
      sam_scan_chunks over record bytes just past its seam (260 chunks of OVL_CHUNK: the second iteration sees four), with a
      window that ends exactly at, one byte before and one byte behind the first byte of record 256 x OVL_CHUNK;
  test_smallest_pile_whose_record_chunks_outnumber_the_grid
      k_ovl_size and k_ovl_write: the loop of a workgroup over record chunks (more chunks of OVL_CHUNK than OVL_WGS_PER_CU
      workgroups per CU).  The one slow test of the module: the model formats 2.1 M records on the host."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from simmr_amd.engine import Engine, Reads
from tests import _overlap, _seams

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def _define(name, what):
    return int(re.search(rf"^#define\s+{what}\s+(\d+)u?\b", (CSRC / name).read_text(), re.M).group(1))


T = _define("sam_sort_kernels.hip", "SAMSORT_TILE")
DIGIT = _define("sam_sort_kernels.hip", "SAMSORT_DIGIT_BITS")
SAM_CHUNK = _define("sam_kernels.hip", "SAM_CHUNK")
OVL_CHUNK = _define("overlap_kernels.hip", "OVL_CHUNK")
WGS_PER_CU = _define("overlap_kernels.hip", "OVL_WGS_PER_CU")
SCAN = 256  # entries a pass of sam_scan_chunks and of k_samsort_digit_scan takes: the workgroup's threads
BIG = 20_000_000
SLOTS = {0: [1_000_000], 1: [300_000, 90_001, 30_017, 70_000, 123_457], 2: [BIG], 3: [400 + 3 * i for i in range(300)]}
CONTIGS = [(s, c, SLOTS[s][c]) for s in SLOTS for c in range(len(SLOTS[s]))]  # row -> (slot, contig, bases)
M = 12        # the chain's min_overlap
N_SHORT = 3000
G = 256       # canary entries


def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def device_reads(o, device):
    """Reads that carry the metadata columns alone: seq, qual and seq_off are one-element tensors nobody may read"""
    import torch
    n = len(o["start"])
    pad = lambda a: np.concatenate([a, np.zeros(1, a.dtype)])  # (no tensor without an element)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(pad(a)).astype(dt)).to(device)
    one = lambda dt: torch.zeros(1, dtype=dt, device=device)
    return Reads(seq=one(torch.uint8), qual=one(torch.uint8), seq_off=one(torch.int64), start=t(o["start"].view(np.int64), np.int64),
                 end=t(o["end"].view(np.int64), np.int64), contig=t(o["contig"].view(np.int32), np.int32), genome=t(o["genome"].view(np.int32), np.int32),
                 read_id=t(o["read_id"].view(np.int32), np.int32), flags=t(o["flags"], np.uint8), n_reads=n, total_bases=0)


def host_columns(g, c, lo, L, rev, rid):
    return {"start": np.where(rev == 1, lo + L, lo).astype(np.uint64), "end": np.where(rev == 1, lo, lo + L).astype(np.uint64),
            "contig": c.astype(np.uint32), "genome": g.astype(np.uint32), "read_id": rid.astype(np.uint32), "flags": rev.astype(np.uint8)}


def random_ids(rng, n):
    """ids of one to ten decimal digits, each width as likely as the others"""
    return (rng.integers(0, 10 ** 10, n) % 10 ** rng.integers(1, 11, n)) % 2**32


def same_text(got, want, what):
    if got != want:
        gl, wl = got.split(b"\n"), want.split(b"\n")
        i = next((k for k in range(min(len(gl), len(wl))) if gl[k] != wl[k]), min(len(gl), len(wl)))
        raise AssertionError(f"{what}: {len(got)} bytes against {len(want)}; line {i} differs:\n{gl[i:i + 1]}\n{wl[i:i + 1]}")


def same_columns(cols, want, what):
    for name, w in zip(("a", "b", "ref_start", "ref_end", "row"), want):
        assert np.array_equal(cols[name].cpu().numpy().astype(np.int64), np.asarray(w, dtype=np.int64)), f"{what}: column {name}"


def emit_text(eng, first, n_places, n_bytes):
    """the raw simmr_overlap_emit of a run of places into a buffer of exactly n_bytes"""
    import torch
    out = torch.empty(max(n_bytes, 1), dtype=torch.uint8, device=eng.device)
    eng._check(eng.lib.simmr_overlap_emit(eng._h, first, n_places, None, C.c_void_p(out.data_ptr()), n_bytes))
    return bytes(out[:n_bytes].cpu().numpy())


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
class Chain:
    """n reads in add order (host arrays), and what the models say of them"""

    def __init__(self, n, seed=17):
        rng = np.random.default_rng(seed)
        ne = n - N_SHORT
        n_rows = len(CONTIGS)
        # reads per row: a tenth of the bases on slots 0 and 1, 30 on each of the 300 short contigs, the rest on the 20 M bases
        count = np.array([clen // 10 if s in (0, 1) else 30 if s == 3 else 0 for s, _, clen in CONTIGS], dtype=np.int64)
        big_row = next(r for r, (s, _, _) in enumerate(CONTIGS) if s == 2)
        count[big_row] = ne - int(count.sum())
        assert count[big_row] > 0
        row = np.repeat(np.arange(n_rows), count)
        clen = np.array([x[2] for x in CONTIGS], dtype=np.int64)[row]
        lo = np.zeros(ne, dtype=np.int64)
        at = 0
        for r in range(n_rows):  # steps of 1 to 19 bases inside a row, scaled down where the row is too short for them
            raw = np.cumsum(rng.integers(1, 20, int(count[r])))
            span = CONTIGS[r][2] - (M + 20)
            lo[at:at + count[r]] = raw if raw[-1] <= span else raw * span // raw[-1]
            at += int(count[r])
        L = M + rng.integers(0, 21, ne)  # a read reaches 0 to 20 bases past the threshold: its next one or two neighbours
        # one read in eight on the (row, lo) of the read before it, and runs of four across tile boundaries of the sorted places
        k = np.arange(7, ne, 8)
        k = k[row[k] == row[k - 1]]
        lo[k] = lo[k - 1]
        n_tiles = (n + T - 1) // T
        self.tie_tiles = [t for t in (1, 2, SCAN - 1, SCAN, SCAN + 1, n_tiles - 2) if 2 <= t * T < ne - 2 and row[t * T - 2] == row[t * T + 1]]
        for t in self.tie_tiles:
            lo[t * T - 1:t * T + 2] = lo[t * T - 2]
        assert (np.diff(lo)[row[1:] == row[:-1]] >= 0).all() and (lo + L <= clen).all()
        # the short reads, anywhere: behind every row in the sorted order, in no record
        srow = rng.integers(0, n_rows, N_SHORT)
        slen = np.array([x[2] for x in CONTIGS], dtype=np.int64)[srow]
        row, lo, L = np.concatenate([row, srow]), np.concatenate([lo, (rng.random(N_SHORT) * (slen - M)).astype(np.int64)]), np.concatenate([L, rng.integers(0, M, N_SHORT)])
        # the add order: a random permutation, then the second read of most ties moved to 3 .. 9 ordinals behind the first
        perm = rng.permutation(n)  # chain index -> ordinal
        inv = np.empty(n, dtype=np.int64)
        inv[perm] = np.arange(n)
        busy = np.zeros(n, dtype=bool)
        busy[k] = busy[k - 1] = True
        want = perm[k - 1] + rng.integers(3, 10, k.size)
        ok = want < n
        j = inv[np.where(ok, want, 0)]  # the chain index that holds the wanted ordinal
        ok &= ~busy[j]
        _, first = np.unique(j, return_index=True)
        once = np.zeros(k.size, dtype=bool)
        once[first] = True
        ok &= once
        perm[k[ok]], perm[j[ok]] = perm[j[ok]], perm[k[ok]]
        assert np.array_equal(np.sort(perm), np.arange(n)) and ok.sum() > k.size // 2

        def put(a):  # from chain order to add order
            out = np.empty_like(a)
            out[perm] = a
            return out

        self.n, self.ne = n, ne
        self.row, self.lo, self.L = put(row), put(lo), put(L)
        self.hi = self.lo + self.L
        self.rev, self.rid = rng.integers(0, 2, n).astype(np.uint8), random_ids(rng, n)
        g = np.array([x[0] for x in CONTIGS], dtype=np.int64)[self.row]
        c = np.array([x[1] for x in CONTIGS], dtype=np.int64)[self.row]
        self.o = host_columns(g, c, self.lo, self.L, self.rev, self.rid)
        cut = [n // 2 + 1, n // 2 + 8]  # three adds of unequal size
        self.calls = [{key: v[a:b] for key, v in self.o.items()} for a, b in zip([0] + cut, cut + [n])]
        # what the models say: the pairs by index, the records' bytes from digit counts, the records of every place
        self.pairs = _seams.pair_columns(self.row, self.lo, self.hi, M)
        a, b, s, e, _ = self.pairs
        self.n_pairs = int(a.size)
        self.lengths = _seams.record_lengths(self.lo, self.hi, self.rev, self.rid, a, b, s, e, False)
        self.byte_at = np.zeros(self.n_pairs + 1, dtype=np.int64)  # the bytes before record j
        np.cumsum(self.lengths, out=self.byte_at[1:])
        order = _seams.sorted_order(self.row, self.lo, self.hi, M)
        assert order.size == ne
        place_of = np.full(n, -1, dtype=np.int64)
        place_of[order] = np.arange(ne)
        q = place_of[a]
        assert (np.diff(q) >= 0).all() and q.min() >= 0
        self.rec_off = np.searchsorted(q, np.arange(n + 1), side="left")  # the first record of place p; the short reads' places hold none
        self.order = order

    def __getitem__(self, r):
        """the model's read tuple of ordinal r, for _overlap.record"""
        return (int(self.row[r]), int(self.lo[r]), int(self.hi[r]), int(self.rev[r]), int(self.rid[r]), 0)

    def text_of(self, first, n_places):
        j0, j1 = int(self.rec_off[first]), int(self.rec_off[first + n_places])
        return "".join(_overlap.record(self, tuple(int(col[j]) for col in self.pairs)) for j in range(j0, j1)).encode()

    def place_holding(self, j):
        """the place whose records hold record j"""
        return int(np.searchsorted(self.rec_off, j, side="right")) - 1


@pytest.fixture(scope="module")
def chain():
    return Chain(max(SCAN * T, n_cu() * WGS_PER_CU * SAM_CHUNK) + T + 5)


@pytest.fixture(scope="module")
def chain_eng(chain):
    """an engine of the chain's own: the four slots staged, the chain added in three calls"""
    e = Engine(0)
    for slot, lens in SLOTS.items():
        e.stage_synthetic(slot, lens, 10 + slot)
    e.overlap_reset(False)
    for o in chain.calls:
        e.overlap_add(device_reads(o, e.device))
    yield e
    e.close()


def test_chain_columns_and_plan(chain, chain_eng):
    n, n_tiles, n_chunks = chain.n, (chain.n + T - 1) // T, (chain.n + SAM_CHUNK - 1) // SAM_CHUNK
    r_chunks = (chain.n_pairs + OVL_CHUNK - 1) // OVL_CHUNK
    # the preconditions: which loops this run enters
    assert n_tiles > SCAN, "k_samsort_digit_scan: more than 256 tiles"
    assert n_chunks > n_cu() * WGS_PER_CU, "k_ovl_partners, k_ovl_offsets: more read chunks than workgroups"
    assert n_chunks > 2 * SCAN and r_chunks > SCAN, "sam_scan_chunks: the counts and the record bytes past 256 chunks"
    assert n_cu() != 256 or -(-n_tiles // SCAN) == 5
    n_rows = len(CONTIGS)
    assert BIG.bit_length() + n_rows.bit_length() == 34 and -(-34 // DIGIT) == 5 and 34 % DIGIT != 0  # (a row more than the contigs: the short reads')
    assert int(chain.lo.max()) >= 2**24 and len(set(chain.row[chain.order].tolist())) == n_rows
    assert sorted(len(o["start"]) for o in chain.calls)[0] == 7 and len({len(o["start"]) for o in chain.calls}) == 3
    # what the chain promises: pairs near n, ties whose stable order shows, ties across tile 256, short reads in no record
    a, b, s, e, row = chain.pairs
    assert n // 2 < chain.n_pairs < 3 * n
    tie = (chain.row[a] == chain.row[b]) & (chain.lo[a] == chain.lo[b])
    assert tie.sum() > n // 10 and (a[tie] < b[tie]).all() and SCAN in chain.tie_tiles and SCAN - 1 in chain.tie_tiles and SCAN + 1 in chain.tie_tiles
    assert (chain.L < M).sum() == N_SHORT and (chain.L[a] >= M).all() and (chain.L[b] >= M).all()
    assert chain.n_pairs == int(chain.rec_off[chain.ne]) == int(chain.rec_off[n])
    # the plan, and the five columns in full: together they carry the whole permutation
    assert chain_eng.overlap_plan(M) == (n, chain.n_pairs, int(chain.lengths.sum()))
    same_columns(chain_eng.overlaps(M, text=False, columns=True), chain.pairs, "chain")


def test_chain_text_windows(chain, chain_eng):
    n, seam_rec = chain.n, SCAN * OVL_CHUNK
    assert chain.n_pairs > seam_rec + OVL_CHUNK and n > SCAN * SAM_CHUNK + SAM_CHUNK
    assert chain_eng.overlap_plan(M)[1] == chain.n_pairs
    p = chain.place_holding(seam_rec)
    assert chain.rec_off[p] <= seam_rec < chain.rec_off[p + 1]
    runs = {"around place 256 x SAM_CHUNK": (SCAN * SAM_CHUNK - 500, 1000),
            "around record 256 x OVL_CHUNK": (p - 500, 1000),
            "the last places": (chain.ne - 1000, n - (chain.ne - 1000))}
    for what, (first, n_places) in runs.items():
        want = chain.text_of(first, n_places)
        j0, j1 = int(chain.rec_off[first]), int(chain.rec_off[first + n_places])
        assert len(want) == int(chain.byte_at[j1] - chain.byte_at[j0]) and j1 - j0 > 500, what
        same_text(emit_text(chain_eng, first, n_places, len(want)), want, what)
    assert emit_text(chain_eng, n - 1000, 1000, 0) == b""  # the last 1000 places are short reads'


def test_chain_window_sizes(chain, chain_eng):
    seam_rec = SCAN * OVL_CHUNK
    r_chunks = (chain.n_pairs + OVL_CHUNK - 1) // OVL_CHUNK
    assert r_chunks > SCAN, "k_ovl_window: more than 256 chunk prefixes to search"
    assert chain_eng.overlap_plan(M)[1] == chain.n_pairs
    place_byte = chain.byte_at[chain.rec_off]  # the bytes before the first record of place p, p <= n
    p = chain.place_holding(seam_rec)

    def want(first, budget):
        last = int(np.searchsorted(place_byte, place_byte[first] + budget, side="right")) - 1  # the longest run that fits
        return last - first, int(chain.rec_off[last] - chain.rec_off[first]), int(place_byte[last] - place_byte[first])

    first = p - 300
    for last in (p + 200, p + 1, chain.place_holding(2 * seam_rec), chain.ne):
        for spare in (0, 5, -1):  # ending with a place's last byte, inside the next place's records, a byte short of the last place
            budget = int(place_byte[last] - place_byte[first]) + spare
            got, w = chain_eng.overlap_window(first, budget), want(first, budget)
            assert got == w, (first, last, spare, got, w)
            assert chain.rec_off[first] < seam_rec and (spare < 0 or seam_rec < chain.rec_off[first + w[0]])
    total = int(chain.byte_at[-1])
    assert chain_eng.overlap_window(0, total) == (chain.n, chain.n_pairs, total) == want(0, total)
    assert chain_eng.overlap_window(0, total - 1) == want(0, total - 1) and want(0, total - 1)[0] < chain.ne


# ---- piles -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pile_eng():
    e = Engine(0)
    e.stage_synthetic(0, [1_000_000], 20)
    yield e
    e.close()


def pile(m, seed):
    """m reads that all share bases 10 050 .. 10 500 of one contig: m (m - 1) / 2 records; ids of one to ten digits, both strands"""
    rng = np.random.default_rng(seed)
    zero = np.zeros(m, dtype=np.int64)
    return host_columns(zero, zero, 10_000 + rng.integers(0, 51, m), 500 + rng.integers(0, 101, m), rng.integers(0, 2, m).astype(np.uint8), random_ids(rng, m))


def pile_model(o, paired):
    """(model reads, text, pairs, bytes before every record, bytes before the first record of every place)"""
    reads = _overlap.reads_of(o, {(0, 0): 0}, paired)
    text, ps = _overlap.paf(reads, 1)
    m = len(reads)
    assert len(ps) == m * (m - 1) // 2
    byte_at = np.zeros(len(ps) + 1, dtype=np.int64)
    np.cumsum(np.array([len(l) for l in text.splitlines(keepends=True)], dtype=np.int64), out=byte_at[1:])
    rec_off = np.concatenate([np.cumsum(np.arange(m, 0, -1)) - m, [len(ps)]])  # place p holds m - 1 - p records
    assert all(ps[int(rec_off[p])][0] != ps[int(rec_off[p]) - 1][0] for p in range(1, m - 1))
    return reads, text, ps, byte_at, rec_off


@pytest.fixture(scope="module")
def pile_730():
    o = pile(730, 5)
    return (o,) + pile_model(o, True)


def columns_of(ps):
    return [[p[k] for p in ps] for k in range(5)]


def test_pile_730_text_columns_and_pieces(pile_eng, pile_730):
    o, reads, text, ps, byte_at, rec_off = pile_730
    seam = SCAN * OVL_CHUNK
    r_chunks = (len(ps) + OVL_CHUNK - 1) // OVL_CHUNK
    assert SCAN < r_chunks <= SCAN + 8 and len(ps) > seam + OVL_CHUNK, "sam_scan_chunks over the record bytes: just past 256 chunks"
    sizes = np.diff(byte_at)
    for j in (seam - OVL_CHUNK, seam, seam + OVL_CHUNK):  # records of different sizes on both sides of chunks 255, 256 and 257
        assert len(set(sizes[j - 4:j].tolist())) > 1 and len(set(sizes[j:j + 4].tolist())) > 1 and sizes[j - 1] != sizes[j], j
    assert {len(str(r[4])) for r in reads} == set(range(1, 11)) and {r[3] for r in reads} == {0, 1} and len({r[1] for r in reads}) > 40
    pile_eng.overlap_reset(True)
    pile_eng.overlap_add(device_reads(o, pile_eng.device))
    assert pile_eng.overlap_plan(1) == (730, len(ps), len(text))
    got, cols = pile_eng.overlaps(1, text=True, columns=True)
    same_text(bytes(got.cpu().numpy()), text, "pile of 730")
    same_columns(cols, columns_of(ps), "pile of 730")
    # a piece that ends exactly at the first byte of record 256 x OVL_CHUNK, a byte before it, a byte behind it
    place_byte = byte_at[rec_off]
    X = int(byte_at[seam])
    assert X not in place_byte.tolist()  # (the record lies inside a place's records)
    for mb in (X - 1, X, X + 1):
        last = int(np.searchsorted(place_byte, mb, side="right")) - 1
        assert pile_eng.overlap_window(0, mb) == (last, int(rec_off[last]), int(place_byte[last])), mb
        got, cols = pile_eng.overlaps(1, text=True, columns=True, max_bytes=mb)
        same_text(bytes(got.cpu().numpy()), text, f"pile of 730 in pieces of {mb} bytes")
        same_columns(cols, columns_of(ps), f"pile of 730 in pieces of {mb} bytes")
    # and windows from inside the pile, whose own bytes end there: the count inside chunk 256 and chunk 255 of the records
    first = 300
    for mb in (X - 1, X, X + 1):
        budget = mb - int(place_byte[first])
        last = int(np.searchsorted(place_byte, mb, side="right")) - 1
        assert pile_eng.overlap_window(first, budget) == (last - first, int(rec_off[last] - rec_off[first]), int(place_byte[last] - place_byte[first]))


def test_pile_730_exact_capacity_between_canaries(pile_eng, pile_730):
    import torch
    o, reads, want, ps, byte_at, rec_off = pile_730
    assert (len(ps) + OVL_CHUNK - 1) // OVL_CHUNK > SCAN
    pile_eng.overlap_reset(True)
    pile_eng.overlap_add(device_reads(o, pile_eng.device))
    n, pairs, total = pile_eng.overlap_plan(1)
    assert (n, pairs, total) == (730, len(ps), len(want))
    text = torch.full((total + 2 * G,), 0xA5, dtype=torch.uint8, device=pile_eng.device)
    c32 = {k: torch.full((pairs + 2 * G,), -7, dtype=torch.int32, device=pile_eng.device) for k in ("a", "b", "row")}
    c64 = {k: torch.full((pairs + 2 * G,), -7, dtype=torch.int64, device=pile_eng.device) for k in ("ref_start", "ref_end")}
    ptr = lambda t: t.data_ptr() + G * t.element_size()
    pod = _abi.OverlapCols(ptr(c32["a"]), ptr(c32["b"]), ptr(c64["ref_start"]), ptr(c64["ref_end"]), ptr(c32["row"]), pairs)
    # short capacity: ERANGE, nothing written
    assert pile_eng.lib.simmr_overlap_emit(pile_eng._h, 0, n, C.byref(pod), C.c_void_p(ptr(text)), total - 1) == _abi.ERANGE
    short = _abi.OverlapCols(ptr(c32["a"]), None, None, None, None, pairs - 1)
    assert pile_eng.lib.simmr_overlap_emit(pile_eng._h, 0, n, C.byref(short), None, 0) == _abi.ERANGE
    assert bool((text == 0xA5).all()) and all(bool((v == -7).all()) for v in list(c32.values()) + list(c64.values()))
    pile_eng._check(pile_eng.lib.simmr_overlap_emit(pile_eng._h, 0, n, C.byref(pod), C.c_void_p(ptr(text)), total))
    host = text.cpu().numpy()
    assert (host[:G] == 0xA5).all() and (host[G + total:] == 0xA5).all()
    same_text(bytes(host[G:G + total]), want, "between canaries")
    for k, v in list(c32.items()) + list(c64.items()):
        h = v.cpu().numpy()
        assert (h[:G] == -7).all() and (h[G + pairs:] == -7).all(), k
    same_columns({k: v[G:G + pairs] for k, v in list(c32.items()) + list(c64.items())}, columns_of(ps), "canaries")


def test_smallest_pile_whose_record_chunks_outnumber_the_grid(pile_eng):
    cap = n_cu() * WGS_PER_CU
    m = 2
    while m * (m - 1) // 2 <= cap * OVL_CHUNK + OVL_CHUNK:
        m += 1
    assert n_cu() != 256 or m == 2050
    o = pile(m, 6)
    reads, text, ps, _, _ = pile_model(o, False)
    assert (len(ps) + OVL_CHUNK - 1) // OVL_CHUNK > cap + 1, "k_ovl_size, k_ovl_write: more record chunks than workgroups"
    pile_eng.overlap_reset(False)
    pile_eng.overlap_add(device_reads(o, pile_eng.device))
    assert pile_eng.overlap_plan(1) == (m, len(ps), len(text))
    got, cols = pile_eng.overlaps(1, text=True, columns=True)
    same_text(bytes(got.cpu().numpy()), text, f"pile of {m}")
    same_columns(cols, columns_of(ps), f"pile of {m}")
