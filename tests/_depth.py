"""numpy restatement of the coverage-depth definitions of include/simmr_hip.h (simmr_depth_*): depth[] over the dense layout
of the tracked genomes, the contig rows, the histogram and the windows — and the Python formatter of the two TSV files
`simmr-hip --depth / --depth-track` write.  Nothing here calls the library."""
import numpy as np

HIST_BINS = 256
ROW_KEYS = ("genome", "contig", "first", "len", "covered", "depth_sum", "depth_max", "first_window")


def layout(lens):
    """lens: {genome slot: [contig lengths]} -> (rows genome / contig / first / len in the order of depth[], n_positions)"""
    g = [s for s in sorted(lens) for _ in lens[s]]
    c = [k for s in sorted(lens) for k in range(len(lens[s]))]
    ln = np.array([n for s in sorted(lens) for n in lens[s]], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    return {"genome": np.array(g, dtype=np.uint32), "contig": np.array(c, dtype=np.uint32), "first": first[:-1].astype(np.uint64),
            "len": ln.astype(np.uint64)}, int(first[-1])


def _read_windows(cols, lens):
    lay, n = layout(lens)
    where = {(int(g), int(c)): int(f) for g, c, f in zip(lay["genome"], lay["contig"], lay["first"])}
    a, b = cols["start"].astype(np.int64), cols["end"].astype(np.int64)
    lo, L = np.minimum(a, b), np.abs(b - a)
    first = np.array([where[(int(g), int(c))] for g, c in zip(cols["genome"], cols["contig"])], dtype=np.int64)
    return first + lo, L, n


def depth(cols, lens):
    """depth[] of the reads of `cols` (start, end, contig, genome): a difference array and its running sum"""
    at, L, n = _read_windows(cols, lens)
    diff = np.zeros(n + 1, dtype=np.int64)
    np.add.at(diff, at[L > 0], 1)
    np.add.at(diff, (at + L)[L > 0], -1)
    d = np.cumsum(diff)[:n]
    assert (d >= 0).all()
    return d.astype(np.uint32)


def depth_loop(cols, lens):
    """the same read by read (used only to test depth())"""
    at, L, n = _read_windows(cols, lens)
    d = np.zeros(n, dtype=np.uint32)
    for x, k in zip(at, L):
        d[x:x + k] += 1
    return d


def summary(d, lens, window=0):
    """the dict Engine.depth_summary returns, from a depth[] array"""
    lay, n = layout(lens)
    assert d.size == n
    out = dict(lay)
    d64 = d.astype(np.uint64)
    spans = [(int(f), int(f + l)) for f, l in zip(lay["first"], lay["len"])]
    out["covered"] = np.array([np.count_nonzero(d[a:b]) for a, b in spans], dtype=np.uint64)
    out["depth_sum"] = np.array([d64[a:b].sum() for a, b in spans], dtype=np.uint64)
    out["depth_max"] = np.array([d[a:b].max() if b > a else 0 for a, b in spans], dtype=np.uint32)
    out["hist"] = np.bincount(np.minimum(d, HIST_BINS - 1), minlength=HIST_BINS).astype(np.uint64)
    out["first_window"] = np.zeros(len(spans), dtype=np.uint64)
    if window:  # a contig's windows start at multiples of `window` from ITS first position; the last one is partial
        ws, wc, wm, n_win = [], [], [], 0
        for k, (a, b) in enumerate(spans):
            out["first_window"][k] = n_win
            cuts = np.arange(0, b - a, window)
            if cuts.size:
                ws.append(np.add.reduceat(d64[a:b], cuts))
                wc.append(np.add.reduceat((d[a:b] > 0).astype(np.uint32), cuts))
                wm.append(np.maximum.reduceat(d[a:b], cuts))
            n_win += cuts.size
        out["win_sum"] = np.concatenate(ws + [np.zeros(0, np.uint64)]).astype(np.uint64)
        out["win_covered"] = np.concatenate(wc + [np.zeros(0, np.uint32)]).astype(np.uint32)
        out["win_max"] = np.concatenate(wm + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return out


def assert_summary(got, want, what):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, got[k][:8], want[k][:8])


def tsv(s, names):
    """--depth FILE; names = {genome slot: (genome id, [sequence ids])}"""
    text = "genome_id\tsequence_id\tlength\tcovered\tdepth_sum\tdepth_max\n"
    for k in range(len(s["genome"])):
        gid, sids = names[int(s["genome"][k])]
        text += f"{gid}\t{sids[int(s['contig'][k])]}\t{int(s['len'][k])}\t{int(s['covered'][k])}\t{int(s['depth_sum'][k])}\t{int(s['depth_max'][k])}\n"
    return text


def track_tsv(s, names, window):
    """--depth-track FILE: one line per window, start / end 0-based and half-open inside the sequence"""
    text = "genome_id\tsequence_id\tstart\tend\tdepth_sum\tcovered\tdepth_max\n"
    for k in range(len(s["genome"])):
        gid, sids = names[int(s["genome"][k])]
        ln, w0 = int(s["len"][k]), int(s["first_window"][k])
        for i, x in enumerate(range(0, ln, window)):
            text += (f"{gid}\t{sids[int(s['contig'][k])]}\t{x}\t{min(x + window, ln)}\t{int(s['win_sum'][w0 + i])}\t"
                     f"{int(s['win_covered'][w0 + i])}\t{int(s['win_max'][w0 + i])}\n")
    return text


def constants():
    """DEPTH_TILE and DEPTH_TOPS_WIDTH as simmr_amd/csrc/depth_kernels.hip defines them: the GPU tests size their tile
    edges and the genome of the tile-sum loop from these (tests/test_depth_host.py says where they come from)"""
    import re
    from pathlib import Path
    src = (Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc" / "depth_kernels.hip").read_text()
    c = {m.group(1): int(m.group(2)) for m in re.finditer(r"^constexpr uint32_t (DEPTH_\w+) = (\d+);", src, re.M)}
    return c["DEPTH_TILE"], c["DEPTH_TOPS_WIDTH"]
