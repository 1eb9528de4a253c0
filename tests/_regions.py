"""The gold-standard assembly (include/simmr_hip.h: simmr_regions_*) restated in numpy, independently of the kernels: the
regions of a depth[] array with np.diff, the same with a plain position-by-position loop, the bases from host copies of the
contigs, and the Python formatters of the FASTA and the TSV that `simmr-hip --gold-assembly / --gold-regions` write.

`lens` is {genome slot: [contig length, ...]} as in tests/_depth.py: depth[] is the contigs of the slots in ascending order,
back to back."""
import re
from pathlib import Path

import numpy as np

COLUMNS = (("genome", np.uint32), ("contig", np.uint32), ("start", np.uint64), ("len", np.uint64), ("depth_sum", np.uint64),
           ("seq_off", np.uint64))
TSV_HEADER = "genome_id\tsequence_id\tstart\tlength\tdepth_sum\tseq_off\n"


def layout(lens):
    """(genome, contig, first) per tracked contig and n_positions"""
    g = np.array([s for s in sorted(lens) for _ in lens[s]], dtype=np.uint32)
    c = np.array([i for s in sorted(lens) for i in range(len(lens[s]))], dtype=np.uint32)
    first = np.cumsum([0] + [int(x) for s in sorted(lens) for x in lens[s]]).astype(np.int64)
    return g, c, first


def _columns(g, c, first, a, b, depth, min_len):
    keep = (b - a) >= min_len
    a, b = a[keep], b[keep]
    k = np.searchsorted(first, a, side="right") - 1  # (an empty contig in front shares its first: the later one owns it)
    csum = np.concatenate([[0], np.cumsum(depth.astype(np.uint64), dtype=np.uint64)])
    off = np.concatenate([[0], np.cumsum(b - a)]).astype(np.uint64)
    return {"genome": g[k], "contig": c[k], "start": (a - first[k]).astype(np.uint64), "len": (b - a).astype(np.uint64),
            "depth_sum": (csum[b] - csum[a]).astype(np.uint64), "seq_off": off}


def regions(depth, lens, min_depth=1, min_len=1):
    """np.diff on depth >= min_depth with the contig boundaries forced"""
    g, c, first = layout(lens)
    depth = np.asarray(depth)
    assert depth.size == first[-1]
    q = np.zeros(depth.size + 2, dtype=np.int8)
    q[1:-1] = depth >= min_depth
    edge = np.diff(q)                       # edge[x]: +1 a run starts at x, -1 a run ended in front of x
    starts, ends = edge == 1, edge == -1
    inner = first[(first > 0) & (first < depth.size)]
    both = inner[(q[inner] == 1) & (q[inner + 1] == 1)]  # covered on both sides of a boundary: one run ends, one starts
    starts[both] = True
    ends[both] = True
    return _columns(g, c, first, np.flatnonzero(starts).astype(np.int64), np.flatnonzero(ends).astype(np.int64), depth, min_len)


def regions_loop(depth, lens, min_depth=1, min_len=1):
    """the definition, position by position"""
    g, c, first = layout(lens)
    a, b = [], []
    for k in range(len(g)):
        run = None
        for x in range(int(first[k]), int(first[k + 1])):
            if depth[x] >= min_depth:
                if run is None:
                    run = x
            elif run is not None:
                a.append(run); b.append(x); run = None
        if run is not None:
            a.append(run); b.append(int(first[k + 1]))
    return _columns(g, c, first, np.array(a, dtype=np.int64), np.array(b, dtype=np.int64), np.asarray(depth), min_len)


def bases(r, contigs):
    """the base stream of regions `r` from host copies of the staged contigs: {genome slot: [uint8 array per contig]}"""
    parts = [contigs[int(g)][int(c)][int(a):int(a) + int(n)] for g, c, a, n in zip(r["genome"], r["contig"], r["start"], r["len"])]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def assert_regions(got, want, what):
    for name, dt in COLUMNS:
        assert got[name].dtype == dt and got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), \
            (what, name, got[name][:8], want[name][:8])


def fasta(r, seq, names):
    """names: {genome slot: (genome id, [sequence id, ...])}; seq: the base stream as bytes"""
    out = []
    for k in range(len(r["genome"])):
        gid, sids = names[int(r["genome"][k])]
        a, n, off = int(r["start"][k]), int(r["len"][k]), int(r["seq_off"][k])
        out.append(f">{gid}|{sids[int(r['contig'][k])]}:{a + 1}-{a + n} depth_sum={int(r['depth_sum'][k])}\n".encode())
        out += [seq[off + i:off + min(i + 80, n)] + b"\n" for i in range(0, n, 80)]
    return b"".join(out)


def tsv(r, names):
    text = TSV_HEADER
    for k in range(len(r["genome"])):
        gid, sids = names[int(r["genome"][k])]
        text += f"{gid}\t{sids[int(r['contig'][k])]}\t{int(r['start'][k])}\t{int(r['len'][k])}\t{int(r['depth_sum'][k])}\t{int(r['seq_off'][k])}\n"
    return text


def constants():
    """(REGIONS_TILE, REGIONS_TOPS_WIDTH, REGIONS_RUN_TILE) as regions_kernels.hip states them"""
    src = (Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc" / "regions_kernels.hip").read_text()
    return tuple(int(re.search(rf"constexpr uint32_t {n} = (\d+);", src).group(1)) for n in ("REGIONS_TILE", "REGIONS_TOPS_WIDTH", "REGIONS_RUN_TILE"))
