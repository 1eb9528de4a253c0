"""The coordinate order of include/simmr_hip.h (simmr_sam_sort_plan) restated in plain Python — TEST INFRASTRUCTURE ONLY.

`rnames` is the list Engine.sam_sorted takes, [(genome slot, [RNAME per contig]), ...]: a contig's row is its place in that
list flattened, the order of the @SQ lines.  The lines themselves are those of tests/_sam.py::record.  Nothing here comes from
the code under test."""
import numpy as np

from tests import _sam


def rows_of(rnames):
    rows, at = {}, 0
    for g, names in rnames:
        for c in range(len(names)):
            rows[(int(g), c)] = at
            at += 1
    return rows


def names_of(rnames):
    return {(int(g), c): name for g, names in rnames for c, name in enumerate(names)}


def keys(o, rnames):
    """key[r] = row << 40 | min(start, end), as Python ints"""
    rows = rows_of(rnames)
    return [(rows[(int(o["genome"][r]), int(o["contig"][r]))] << 40) | min(int(o["start"][r]), int(o["end"][r])) for r in range(len(o["start"]))]


def order(o, rnames):
    key = keys(o, rnames)
    return sorted(range(len(key)), key=lambda r: (key[r], r)), key


def sorted_text(o, t, rnames, paired):
    """(text, key of every line written, line_off): the records of tests/_sam.py in the order of (key, read index)"""
    perm, key = order(o, rnames)
    names = names_of(rnames)
    lines = [_sam.record(o, t, names, r, paired).encode("latin-1") for r in perm]
    line_off = np.zeros(len(perm) + 1, dtype=np.int64)
    np.cumsum(np.array([len(l) for l in lines], dtype=np.int64), out=line_off[1:])
    return b"".join(lines), np.array([key[r] for r in perm], dtype=np.int64), line_off


def stable_sort_of_text(text: bytes, sq_names):
    """an unsorted SAM body stable-sorted by (@SQ index, POS): what `samtools sort` keeps of the order among equal keys aside"""
    idx = {n: i for i, n in enumerate(sq_names)}
    lines = text.split(b"\n")
    assert lines[-1] == b""
    lines = lines[:-1]

    def k(line):
        f = line.split(b"\t", 4)
        return idx[f[2].decode()], int(f[3])
    return b"".join(l + b"\n" for l in sorted(lines, key=k))
