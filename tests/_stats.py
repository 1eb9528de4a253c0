"""The tables of simmr_run_stats (include/simmr_hip.h) restated in numpy — TEST INFRASTRUCTURE ONLY.

Same expected-byte model as tests/_truth.py: the expected byte at offset j of read r is the genome's byte at lo + j, or the
complement of the byte at lo + L - 1 - j for a reverse-complemented read; an edit is an offset whose byte differs.  Every
table is a count over the flat list of (read, offset) pairs.  Nothing here comes from the code under test."""
import re
from pathlib import Path

import numpy as np

from simmr_amd import _abi
from tests import _truth

CYCLES, NM_BINS = 512, 64
CONSTANTS = ("STATS_LANES", "STATS_WG_READS", "STATS_WGS_PER_CU", "STATS_FLUSH_BATCHES", "STATS_MAX_L", "STATS_CYC_STRIDE")
SHAPES = {"reads": (2,), "bases": (2,), "qual_n": (256,), "qual_mismatch": (256,), "pair": (5, 5), "nm_hist": (NM_BINS,),
          "gc_hist": (101,), "cycle_n": (2, CYCLES), "cycle_qsum": (2, CYCLES), "cycle_mismatch": (2, CYCLES),
          "cycle_base": (2, CYCLES, 5)}
CLASS = np.full(256, 4, dtype=np.int64)
CLASS[list(b"ACGT")] = [0, 1, 2, 3]


def constants():
    """{name: value} of CONSTANTS as stats_kernels.hip states them: what tests/_stats_cases.py and tests/test_gpu_stats_seams.py size
    their cases from"""
    src = (Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc" / "stats_kernels.hip").read_text()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(STATS_\w+)\s+(\d+)u?\b", src, re.M)}
    return {n: defines[n] for n in CONSTANTS}


def zeros():
    return {k: np.zeros(s, dtype=np.uint64) for k, s in SHAPES.items()}


def add(a, b):
    return {k: a[k] + b[k] for k in SHAPES}


def flat_reads(lib, o, genomes):
    """o: compact host columns; per base of every read: its read, its offset, the written byte, the expected byte, the quality byte"""
    comp = _truth.complement_lut(lib)
    n = len(o["start"])
    st, en = o["start"].astype(np.int64), o["end"].astype(np.int64)
    lo, L = np.minimum(st, en), np.abs(en - st)
    off = o["seq_off"].astype(np.int64)
    assert np.array_equal(np.diff(off), L)
    rev = (o["flags"] & _abi.FLAG_REVCOMP) != 0
    # every contig of every genome in one array; a read's contig starts at base[r]
    where, parts, at = {}, [], 0
    for slot, g in genomes.items():
        for ci, c in enumerate(g.contigs):
            where[(int(slot), ci)] = (at, c.size)
            parts.append(c)
            at += c.size
    flat = np.concatenate(parts)
    key = o["genome"].astype(np.int64) * (1 << 32) + o["contig"].astype(np.int64)
    base, clen = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for k in np.unique(key):
        base[key == k], clen[key == k] = where[(int(k >> 32), int(k & 0xffffffff))]
    assert (lo + L <= clen).all(), "a read leaves its contig"
    total = int(off[n])
    rr = np.repeat(np.arange(n, dtype=np.int64), L)
    j = np.arange(total, dtype=np.int64) - np.repeat(off[:n], L)
    rv = rev[rr]
    want = flat[base[rr] + np.where(rv, lo[rr] + L[rr] - 1 - j, lo[rr] + j)]
    want = np.where(rv, comp[want], want)
    return n, L, rr, j, o["seq"][:total], want, o["qual"][:total]


def model(lib, o, genomes, n_sets, qual_offset):
    assert n_sets in (1, 2)
    n, L, rr, j, have, want, qual = flat_reads(lib, o, genomes)
    q = (qual.astype(np.int64) - qual_offset) & 255
    d = have != want
    ch, cw = CLASS[have], CLASS[want]
    count = lambda x, size: np.bincount(x, minlength=size).astype(np.uint64)
    wsum = lambda x, w, size: np.rint(np.bincount(x, weights=w, minlength=size)).astype(np.uint64)  # (exact below 2^53)
    sets = np.arange(n, dtype=np.int64) % n_sets
    s = {"reads": count(sets, 2), "bases": wsum(sets, L, 2), "qual_n": count(q, 256), "qual_mismatch": count(q[d], 256),
         "pair": count(cw * 5 + ch, 25).reshape(5, 5)}
    nm = np.bincount(rr[d], minlength=n)
    s["nm_hist"] = count(np.minimum(nm, NM_BINS - 1), NM_BINS)
    gc = np.bincount(rr[(have == ord("G")) | (have == ord("C"))], minlength=n)
    some = L > 0
    s["gc_hist"] = count(100 * gc[some] // L[some], 101)
    c = j < CYCLES
    at = sets[rr[c]] * CYCLES + j[c]
    s["cycle_n"] = count(at, 2 * CYCLES).reshape(2, CYCLES)
    s["cycle_qsum"] = wsum(at, q[c], 2 * CYCLES).reshape(2, CYCLES)
    s["cycle_mismatch"] = count(at[d[c]], 2 * CYCLES).reshape(2, CYCLES)
    s["cycle_base"] = count(at * 5 + ch[c], 2 * CYCLES * 5).reshape(2, CYCLES, 5)
    return s


def assert_stats(got, want, what=""):
    assert list(got) == list(SHAPES), list(got)
    for k, shape in SHAPES.items():
        assert got[k].shape == shape and got[k].dtype == np.uint64, f"{what}: {k} is {got[k].dtype}{got[k].shape}"
        if not np.array_equal(got[k], want[k]):
            i = np.argwhere(got[k] != want[k])[0]
            raise AssertionError(f"{what}: {k}{list(map(int, i))} is {got[k][tuple(i)]}, the model has {want[k][tuple(i)]} "
                                 f"({np.count_nonzero(got[k] != want[k])} entries differ)")


def tsv(s):
    """`simmr-hip --stats`: table, set, i, j, count of every non-zero entry, in the struct's order"""
    out = ["table\tset\ti\tj\tcount\n"]
    for k, shape in SHAPES.items():
        for idx in np.ndindex(*shape):
            v = int(s[k][idx])
            if not v:
                continue
            if k in ("reads", "bases"):
                cols = (idx[0], "-", "-")
            elif k.startswith("cycle_"):
                cols = (idx[0], idx[1], idx[2] if len(idx) == 3 else "-")
            elif k == "pair":
                cols = ("-", idx[0], idx[1])
            else:
                cols = ("-", idx[0], "-")
            out.append("%s\t%s\t%s\t%s\t%d\n" % ((k,) + cols + (v,)))
    return "".join(out)
