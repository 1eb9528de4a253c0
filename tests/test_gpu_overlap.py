"""The true read-to-read overlaps of the device (simmr_overlap_*, include/simmr_hip.h) against the plain-Python model of
tests/_overlap.py: the PAF text byte for byte and the columns entry for entry.  The pass reads metadata columns only, so the
reads here are hand-built columns on small synthetic slots: no bases are made."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import MinimalLongErrorProfile, _abi
from simmr_amd._abi import SimmrError
from simmr_amd.engine import Engine, Reads
from tests import _overlap

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"
T = int(re.search(r"^#define\s+SAMSORT_TILE\s+(\d+)u", (CSRC / "sam_sort_kernels.hip").read_text(), re.M).group(1))
SLOTS = {0: [1_000_000], 1: [5_000, 7_000, 200_000], 3: [40_000, 20_000]}  # (slot 2 is not staged)
ROWS = {(0, 0): 0, (1, 0): 1, (1, 1): 2, (1, 2): 3, (3, 0): 4, (3, 1): 5}
BIG_ID = 4_000_000_000  # read ids of ten digits


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    for slot, lens in SLOTS.items():
        e.stage_synthetic(slot, lens, 20 + slot)
    yield e
    e.close()


def columns(specs):
    """host columns from specs of (genome, contig, lo, L, reverse[, read_id]); the id defaults to BIG_ID + the read's index"""
    n = len(specs)
    g = np.array([s[0] for s in specs], dtype=np.int64).reshape(n)
    c = np.array([s[1] for s in specs], dtype=np.int64).reshape(n)
    lo = np.array([s[2] for s in specs], dtype=np.int64).reshape(n)
    L = np.array([s[3] for s in specs], dtype=np.int64).reshape(n)
    rev = np.array([s[4] for s in specs], dtype=np.uint8).reshape(n)
    rid = np.array([s[5] if len(s) > 5 else BIG_ID + i for i, s in enumerate(specs)], dtype=np.int64).reshape(n)
    return {"start": np.where(rev == 1, lo + L, lo).astype(np.uint64), "end": np.where(rev == 1, lo, lo + L).astype(np.uint64),
            "contig": c.astype(np.uint32), "genome": g.astype(np.uint32), "read_id": rid.astype(np.uint32), "flags": rev}


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


def concat(calls):
    return {k: np.concatenate([o[k] for o in calls]) for k in calls[0]}


def add_all(eng, calls, paired):
    eng.overlap_reset(paired)
    for o in calls:
        eng.overlap_add(device_reads(o, eng.device))


def same_text(got, want, what):
    if got != want:
        gl, wl = got.split(b"\n"), want.split(b"\n")
        i = next((k for k in range(min(len(gl), len(wl))) if gl[k] != wl[k]), min(len(gl), len(wl)))
        raise AssertionError(f"{what}: {len(got)} bytes against {len(want)}; line {i} differs:\n{gl[i:i + 1]}\n{wl[i:i + 1]}")


def same_columns(cols, ps, what):
    for k, name in enumerate(("a", "b", "ref_start", "ref_end", "row")):
        want = np.array([p[k] for p in ps], dtype=np.int64)
        assert np.array_equal(cols[name].cpu().numpy().astype(np.int64), want), f"{what}: column {name}"


def check(eng, calls, paired, m, what, max_bytes=None):
    """adds `calls` (a list of host column sets, one add each), compares text and columns with the model; returns (model reads, text, pairs)"""
    calls = calls if isinstance(calls, list) else [calls]
    add_all(eng, calls, paired)
    reads = _overlap.reads_of(concat(calls), ROWS, paired, [len(o["start"]) for o in calls])
    want, ps = _overlap.paf(reads, m)
    text, cols = eng.overlaps(m, text=True, columns=True, max_bytes=max_bytes)
    same_text(bytes(text.cpu().numpy()), want, what)
    same_columns(cols, ps, what)
    assert eng.overlap_plan(m) == (len(reads), len(ps), len(want)), what
    return reads, want, ps


def random_specs(n, seed, span=1_000_000, lmax=400):
    rng = np.random.default_rng(seed)
    L = rng.integers(0, lmax, n)
    lo = rng.integers(0, span - lmax, n)
    return [(0, 0, int(lo[i]), int(L[i]), int(rng.integers(0, 2))) for i in range(n)]


# ---- sizes around the sort's tile ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, T - 1, T, T + 1])
def test_sizes(eng, n):
    specs = random_specs(n, 100 + n, span=max(1000, 120 * n))  # (about three partners a read)
    if n == 2:
        specs = [(0, 0, 500, 300, 0), (0, 0, 400, 300, 1)]
    reads, want, ps = check(eng, columns(specs), False, 20, f"n = {n}")
    assert len(ps) == {0: 0, 1: 0, 2: 1}.get(n, len(ps)) and (n < T - 1 or len(ps) > 0)
    assert {(p[0], p[1]) for p in ps} == _overlap.brute(reads, 20)  # (the model's break against the definition)


# ---- the threshold, the short-read filter, rows --------------------------------------------------------------------------------
def test_threshold_edges(eng):
    specs = [(0, 0, 1000, 300, 0), (0, 0, 1201, 299, 0), (0, 0, 1200, 200, 1), (0, 0, 1300, 200, 0)]
    _, _, ps = check(eng, columns(specs), False, 100, "min_overlap 100")
    got = {(p[0], p[1]): p[3] - p[2] for p in ps}
    assert (0, 1) not in got and got[(0, 2)] == 100 and (0, 3) not in got  # ov 99, 100 and 0 against read 0
    _, _, ps1 = check(eng, columns(specs), False, 1, "min_overlap 1")
    assert (0, 1) in {(p[0], p[1]) for p in ps1} and (0, 3) not in {(p[0], p[1]) for p in ps1}  # abutting reads share nothing


def test_a_short_read_between_two_partners_is_skipped(eng):
    specs = [(0, 0, 0, 1000, 0), (0, 0, 100, 500, 1), (0, 0, 200, 50, 0), (0, 0, 300, 600, 0), (0, 0, 250, 0, 1), (0, 0, 250, 99, 1)]
    _, _, ps = check(eng, columns(specs), False, 100, "short read")
    assert [(p[0], p[1]) for p in ps] == [(0, 1), (0, 3), (1, 3)]
    _, _, ps = check(eng, columns(specs), False, 1, "short read, min_overlap 1")
    assert all(4 not in (p[0], p[1]) for p in ps) and any(2 in (p[0], p[1]) for p in ps)  # L == 0 is in no record


def test_rows_do_not_mix(eng):
    specs = [(1, 0, 4000, 1000, 0), (1, 1, 0, 1000, 0), (0, 0, 999_000, 1000, 1), (1, 0, 0, 4500, 0), (3, 1, 0, 20_000, 0), (3, 0, 39_000, 1000, 1),
             (3, 1, 19_999, 1, 1), (0, 0, 0, 1_000_000, 0)]
    _, _, ps = check(eng, columns(specs), False, 1, "rows")
    assert sorted((p[0], p[1]) for p in ps) == [(3, 0), (4, 6), (7, 2)]


def test_strands_and_containment(eng):
    specs = [(1, 2, 1000, 1000, 0), (1, 2, 1500, 1000, 1), (1, 2, 1200, 600, 0), (1, 2, 900, 1700, 1), (1, 2, 1100, 800, 1), (1, 2, 2400, 150, 0),
             (1, 2, 900, 1700, 0), (1, 2, 1000, 1000, 1)]
    _, want, ps = check(eng, columns(specs), False, 1, "strands")
    strands = {(specs[p[0]][4], specs[p[1]][4]) for p in ps}
    assert strands == {(0, 0), (0, 1), (1, 0), (1, 1)} and want.count(b"\t-\t") > 0 and want.count(b"\t+\t") > 0


def test_digit_widths(eng):
    specs = [(0, 0, 0, 300_000, 0, 7), (0, 0, 0, 300_000, 1, BIG_ID)]
    for v in (9, 10, 99, 100, 99_999, 100_000):
        specs += [(0, 0, v, v, 0, v), (0, 0, 300_000 - v, v, 1, 999_999_999 + v)]
    _, want, _ = check(eng, columns(specs), False, 1, "digit widths")
    for v in (9, 10, 99, 100, 99_999, 100_000):
        assert f"\t{v}\t{2 * v}\t".encode() in want or f"\t{v}\t0\t{v}\t".encode() in want


# ---- piles -----------------------------------------------------------------------------------------------------------------------
def test_two_piles(eng):
    """300 reads on one interval: 44 850 records, ties by ordinal, one place's records across several writer chunks; a second pile
    directly behind it, so that a chunk holds records of two places"""
    specs = [(0, 0, 10_000, 500, i & 1, i) for i in range(300)] + [(0, 0, 10_500, 700, (i >> 1) & 1, 1000 + i) for i in range(300)]
    _, _, ps = check(eng, columns(specs), False, 1, "piles")
    assert len(ps) == 2 * 44_850 and ps[0][:2] == (0, 1) and ps[298][:2] == (0, 299) and ps[299][:2] == (1, 2)


# ---- names, adds, windows ---------------------------------------------------------------------------------------------------------
def test_paired_names(eng):
    specs = []
    for i in range(40):
        specs += [(1, 2, 100 * i, 150, 0, BIG_ID + i), (1, 2, 100 * i + 120, 150, 1, BIG_ID + i)]
    _, want, _ = check(eng, columns(specs), True, 1, "paired")
    assert f"{BIG_ID}/1\t150\t120\t150\t-\t{BIG_ID}/2\t150\t120\t150\t30\t30\t255\n".encode() in want  # mates overlap each other


def test_three_adds_equal_one(eng):
    specs = random_specs(900, 7, span=60_000)
    whole = columns(specs)
    parts = [columns(specs[:300]), columns(specs[300:302]), columns(specs[302:])]
    parts[1]["read_id"], parts[2]["read_id"] = whole["read_id"][300:302], whole["read_id"][302:]  # (ids as in the one add)
    _, a, _ = check(eng, whole, False, 30, "one add")
    _, b, _ = check(eng, parts, False, 30, "three adds")
    assert a == b
    _, c, _ = check(eng, parts, True, 30, "three adds, paired")  # the mate is the parity inside the add
    assert c != a and c.replace(b"/1\t", b"\t").replace(b"/2\t", b"\t") == a


def place_bytes(reads, ps):
    """bytes of the records of every query, in place order (queries without records left out)"""
    out = {}
    for p in ps:
        out[p[0]] = out.get(p[0], 0) + len(_overlap.record(reads, p))
    return list(out.values())


def test_windows(eng):
    specs = [(0, 0, 1000 + 40 * i, 400, i & 1) for i in range(200)]  # every place but the last has records
    reads, want, ps = check(eng, columns(specs), False, 10, "whole")
    pb = place_bytes(reads, ps)
    assert eng.overlap_window(0, pb[0]) == (1, 9, pb[0])          # exactly the first place's bytes
    assert eng.overlap_window(0, pb[0] + pb[1] - 1) == (1, 9, pb[0])
    assert eng.overlap_window(0, pb[0] + pb[1]) == (2, 18, pb[0] + pb[1])
    n, pairs, total = eng.overlap_plan(10)
    assert eng.overlap_window(0, total) == (n, pairs, total) and eng.overlap_window(n, 0) == (0, 0, 0)
    assert eng.overlap_window(199, 0) == (1, 0, 0)                  # a place without records fits anywhere
    np_, pr, by = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    rc = eng.lib.simmr_overlap_window(eng._h, 0, pb[0] - 1, C.byref(np_), C.byref(pr), C.byref(by))  # one byte short
    assert (rc, np_.value, by.value) == (_abi.ERANGE, 0, pb[0])
    rc = eng.lib.simmr_overlap_window(eng._h, 5, 3, C.byref(np_), C.byref(pr), C.byref(by))
    assert (rc, np_.value, by.value) == (_abi.ERANGE, 0, pb[5])
    for mb in (max(pb), max(pb) + 17, 5 * max(pb) + 1, total):       # drained in pieces: the same text and columns
        check(eng, columns(specs), False, 10, f"max_bytes {mb}", max_bytes=mb)
    with pytest.raises(SimmrError) as ei:
        eng.overlaps(10, max_bytes=pb[0] - 1)
    assert ei.value.code == _abi.ERANGE


def test_exact_capacity_between_canaries(eng):
    import torch
    specs = random_specs(900, 11, span=40_000)
    add_all(eng, [columns(specs)], False)
    reads = _overlap.reads_of(columns(specs), ROWS, False)
    want, ps = _overlap.paf(reads, 25)
    n, pairs, total = eng.overlap_plan(25)
    assert (pairs, total) == (len(ps), len(want)) and pairs > 2000
    G = 256
    text = torch.full((total + 2 * G,), 0xA5, dtype=torch.uint8, device=eng.device)
    c32 = {k: torch.full((pairs + 2 * G,), -7, dtype=torch.int32, device=eng.device) for k in ("a", "b", "row")}
    c64 = {k: torch.full((pairs + 2 * G,), -7, dtype=torch.int64, device=eng.device) for k in ("ref_start", "ref_end")}
    ptr = lambda t: t.data_ptr() + G * t.element_size()
    pod = _abi.OverlapCols(ptr(c32["a"]), ptr(c32["b"]), ptr(c64["ref_start"]), ptr(c64["ref_end"]), ptr(c32["row"]), pairs)
    # short capacity: ERANGE, nothing written
    assert eng.lib.simmr_overlap_emit(eng._h, 0, n, C.byref(pod), C.c_void_p(ptr(text)), total - 1) == _abi.ERANGE
    short = _abi.OverlapCols(ptr(c32["a"]), None, None, None, None, pairs - 1)
    assert eng.lib.simmr_overlap_emit(eng._h, 0, n, C.byref(short), None, 0) == _abi.ERANGE
    assert bool((text == 0xA5).all()) and all(bool((v == -7).all()) for v in list(c32.values()) + list(c64.values()))
    eng._check(eng.lib.simmr_overlap_emit(eng._h, 0, n, C.byref(pod), C.c_void_p(ptr(text)), total))
    host = text.cpu().numpy()
    assert bytes(host[G:G + total]) == want and (host[:G] == 0xA5).all() and (host[G + total:] == 0xA5).all()
    for k, v in list(c32.items()) + list(c64.items()):
        h = v.cpu().numpy()
        assert (h[:G] == -7).all() and (h[G + pairs:] == -7).all(), k
    same_columns({k: v[G:G + pairs] for k, v in list(c32.items()) + list(c64.items())}, ps, "canaries")
    # text alone, one column alone: the same records
    only = torch.full((pairs,), -7, dtype=torch.int32, device=eng.device)
    eng._check(eng.lib.simmr_overlap_emit(eng._h, 0, n, C.byref(_abi.OverlapCols(None, only.data_ptr(), None, None, None, pairs)), None, 0))
    assert np.array_equal(only.cpu().numpy(), np.array([p[1] for p in ps]))
    assert bytes(eng.overlaps(25).cpu().numpy()) == want and eng.last_overlap_ms() > 0


# ---- status codes -------------------------------------------------------------------------------------------------------------------
def code(fn, *a):
    with pytest.raises(SimmrError) as ei:
        fn(*a)
    return ei.value.code


def test_status_codes():
    e = Engine(0)
    try:
        e.stage_synthetic(0, [10_000], 1)
        good = columns([(0, 0, 100, 500, 0), (0, 0, 300, 500, 1)])
        assert code(e.overlap_plan, 1) == _abi.ESTATE and code(e.overlap_add, device_reads(good, e.device)) == _abi.ESTATE  # no reset
        assert code(e.overlaps, 1) == _abi.ESTATE
        e.overlap_reset(False)
        assert code(e.overlap_window, 0, 100) == _abi.ESTATE  # no plan
        assert e.lib.simmr_overlap_emit(e._h, 0, 0, None, None, 0) == _abi.ESTATE
        assert code(e.overlap_plan, 0) == _abi.EINVAL
        e.overlap_add(device_reads(good, e.device))
        assert e.overlap_plan(1) == (2, 1, len(b"4000000000\t500\t200\t500\t-\t4000000001\t500\t200\t500\t300\t300\t255\n"))
        # a read ending behind its contig, a contig and a slot that are not staged: EINVAL, and nothing of the call appended
        for bad in ((0, 0, 9_600, 401, 0), (0, 1, 0, 10, 0), (1, 0, 0, 10, 0)):
            assert code(e.overlap_add, device_reads(columns([(0, 0, 0, 10_000, 0), bad]), e.device)) == _abi.EINVAL
            assert code(e.overlap_window, 0, 100) == _abi.ESTATE  # an add, even a refused one, drops the plan
            assert e.overlap_plan(1)[:2] == (2, 1)
        e.overlap_add(device_reads(columns([(0, 0, 9_600, 400, 0)]), e.device))  # ending AT the contig's end is inside
        assert e.overlap_plan(1)[:2] == (3, 1)
        e.overlap_add(device_reads(good, e.device))  # add after plan: the plan is gone
        assert e.lib.simmr_overlap_emit(e._h, 0, 0, None, None, 0) == _abi.ESTATE
        assert e.overlap_plan(1)[:2] == (5, 6)
        missing = device_reads(good, e.device)
        pod = missing.pod()
        pod.read_id = None
        assert e.lib.simmr_overlap_add(e._h, C.byref(pod), 2) == _abi.EINVAL
        assert e.lib.simmr_overlap_emit(e._h, 4, 2, None, None, 0) == _abi.EINVAL  # the run leaves the places
        e.overlap_reset(True)
        assert code(e.overlap_add, device_reads(columns([(0, 0, 0, 10, 0)]), e.device)) == _abi.EINVAL  # odd n under paired
        e.overlap_add(device_reads(good, e.device))
        e.stage_synthetic(1, [500], 2)  # staging since the reset
        assert code(e.overlap_add, device_reads(good, e.device)) == _abi.ESTATE and code(e.overlap_plan, 1) == _abi.ESTATE
        e.overlap_reset(False)
        assert e.overlap_plan(1) == (0, 0, 0) and e.overlaps(1).numel() == 0 and e.overlap_window(0, 0) == (0, 0, 0)
    finally:
        e.close()


# ---- simulated reads ------------------------------------------------------------------------------------------------------------------
def test_simulated_long_reads_in_both_layouts(eng):
    lp = MinimalLongErrorProfile(gamma_mean=1500.0, gamma_std=1000.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    texts = []
    for slots in (0, 16):
        eng.set_read_slots(slots)
        try:
            dev = eng.simulate_long_reads([3], [2000], lp, 9, qual_offset=33)
        finally:
            eng.set_read_slots(0)
        o = dev.to_host()
        eng.overlap_reset(False)
        eng.overlap_add(dev)
        reads = _overlap.reads_of(o, ROWS, False)
        want, ps = _overlap.paf(reads, 500)
        text, cols = eng.overlaps(500, text=True, columns=True, max_bytes=1 << 20)
        same_text(bytes(text.cpu().numpy()), want, f"simulated, slots {slots}")
        same_columns(cols, ps, f"simulated, slots {slots}")
        assert len(ps) > 10_000
        texts.append(want)
    assert texts[0] == texts[1]
