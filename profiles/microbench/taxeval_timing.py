"""Timing of the scoring of a read classifier's calls (simmr_taxeval_truth_add + simmr_taxeval_truth_plan + simmr_taxeval_add): a
synthetic tree of 100 000 nodes (a root, 8 ranks of fan-out), 1 000 genomes placed at its species, a truth of 10 M single reads
as --truth writes them and a candidate of as many lines as Kraken 2 writes them, in two forms: SPREAD, every call at a node near
the read's own (species, genus, family, or another species), and HOT, every call on ONE taxon:
    python profiles/microbench/taxeval_timing.py [reads] [repeats]
One warm-up pass, then `repeats` timed passes of each form; prints per pass the HIP-event time of each call
(simmr_last_taxeval_ms) and the text's bytes per second, then the medians and the ratio of the hot run's add to the spread run's.
On a shared machine run it under a time limit:
    timeout -k 10 500 python profiles/microbench/taxeval_timing.py"""
import statistics
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from simmr_amd import Engine  # noqa: E402

N_NODES, N_GENOMES = 100_000, 1_000


def tree():
    """taxid i + 1 for node i; node 0 the root, then 9 domains, 90 phyla, ... each level's nodes spread under the level above; what is
    left of the 100 000 are species and strains"""
    level = [1, 9, 90, 400, 1500, 4000, 14000, 50000]   # root, domain .. species; the rest are strains
    taxid = np.arange(1, N_NODES + 1, dtype=np.uint32)
    parent, rank = np.ones(N_NODES, dtype=np.uint32), np.zeros(N_NODES, dtype=np.uint8)
    first = np.concatenate([[0], np.cumsum(level)])
    for r in range(1, 9):
        a, b = int(first[r]), int(first[r + 1]) if r < 8 else N_NODES
        above_a, above_n = int(first[r - 1]), int(first[r] - first[r - 1])
        parent[a:b] = above_a + (np.arange(b - a) % above_n) + 1
        rank[a:b] = r
    species = np.arange(int(first[7]), int(first[8]))
    return (taxid, parent, rank), species


def texts(n, taxonomy, species):
    taxid, parent, rank = taxonomy
    g_taxid = taxid[species[:: len(species) // N_GENOMES][:N_GENOMES]]
    ids = np.arange(n, dtype=np.int64) * 3 + 7
    perm = np.random.default_rng(3).permutation(n)            # the truth in no order
    g = perm % N_GENOMES
    truth = "".join(f"{i}\t0\tg{k}\tc1\t0\t150\t+\t150\t0\t\n" for i, k in zip(ids[perm].tolist(), g.tolist())).encode()
    own = g_taxid[np.arange(n) % N_GENOMES].astype(np.int64)  # the candidate in id order: read j is of genome j % N_GENOMES
    up1 = parent[own - 1].astype(np.int64)
    up2 = parent[up1 - 1].astype(np.int64)
    kind = np.arange(n) % 8
    called = np.where(kind < 4, own, np.where(kind == 4, up1, np.where(kind == 5, up2, np.where(kind == 6, taxid[species[(np.arange(n) * 7919) % len(species)]], 0))))
    spread = "".join(f"{'C' if t else 'U'}\t{i}\t{t}\t150\t0:116\n" for i, t in zip(ids.tolist(), called.tolist())).encode()
    one = int(g_taxid[0])
    hot = "".join(f"C\t{i}\t{one}\t150\t0:116\n" for i in ids.tolist()).encode()
    return [(f"g{k}", int(t)) for k, t in enumerate(g_taxid)], truth, spread, hot


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    taxonomy, species = tree()
    genomes, truth, spread, hot = texts(n, taxonomy, species)
    eng = Engine(0)
    import torch
    up = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(eng.device)
    d_truth, d_cand = up(truth), {"spread": up(spread), "hot": up(hot)}
    size = {"spread": len(spread), "hot": len(hot)}
    ev = eng.classify_eval_open(taxonomy, genomes)
    med = {}
    for form in ("spread", "hot"):
        rows = []
        for it in range(repeats + 1):
            ev.reset(taxonomy, genomes)
            ev.truth_add(d_truth)
            t_add = ev.last_ms()
            entries = ev.truth_plan()
            t_plan = ev.last_ms() - t_add
            ev.add(d_cand[form])
            t_rec = ev.last_ms() - t_add - t_plan
            c, by_rank, _ = ev.read()
            ok = entries == n and c["records"] == n and c["missing"] == 0 and c["unknown_read"] == 0 and c["scored"] == (n if form == "hot" else n - n // 8)
            if it == 0:
                continue   # warm-up
            rows.append((t_add, t_plan, t_rec))
            total = t_add + t_plan + t_rec
            print(f"{form} pass {it}: {n} truth lines ({len(truth)} bytes), {n} candidate lines ({size[form]} bytes), {N_NODES} nodes: truth_add {t_add:.3f} ms "
                  f"({len(truth) / t_add / 1e6:.2f} GB/s), truth_plan {t_plan:.3f} ms, add {t_rec:.3f} ms ({size[form] / t_rec / 1e6:.2f} GB/s), together "
                  f"{total:.3f} ms = {(len(truth) + size[form]) / total / 1e6:.2f} GB/s of text, {2 * n / total / 1e3:.1f} M lines/s; species correct "
                  f"{int(by_rank[6, 4])}; counts as made: {ok}", flush=True)
        med[form] = [statistics.median(r[i] for r in rows) for i in range(3)]
        m = med[form]
        print(f"{form} median of {repeats}: truth_add {m[0]:.3f} ms, truth_plan {m[1]:.3f} ms, add {m[2]:.3f} ms ({size[form] / m[2] / 1e6:.2f} GB/s), together "
              f"{sum(m):.3f} ms = {(len(truth) + size[form]) / sum(m) / 1e6:.2f} GB/s of text, {2 * n / sum(m) / 1e3:.1f} M lines/s", flush=True)
    print(f"hot / spread: add {med['hot'][2] / med['spread'][2]:.2f} x, together {sum(med['hot']) / sum(med['spread']):.2f} x "
          f"(more than about 2 x would be the contention on one counter that the LDS table of k_txe_record is there to remove)")
    print("for comparison, profiles/microbench/mapeval_timing_mi355x.txt: 2 M lines a side of SAM, 785 MB a side, in 42.96 ms = 36.6 GB/s of text, 93 M lines/s")
    ev.close()
    eng.close()


if __name__ == "__main__":
    main()
