"""A plain-Python model of simmr_bineval_* (include/simmr_hip.h states the rules): dicts keyed by the name bytes, no hashing in it.
evaluate(truth_adds, bins_adds, genomes) gives a Model whose read(), bins(), cells() and contigs() have the shapes and dtypes of the
device object's; Model.malformed names the side of a malformed text (then the device answers SIMMR_EINVAL)."""
import numpy as np

COUNTS = ("truth_records", "truth_bases", "truth_none", "records", "unknown_contig", "repeated", "assigned", "assigned_bases", "bins", "cells",
          "sum_top_bases", "sum_best_bases", "pairs_cells", "pairs_bins", "pairs_genomes", "bins_c90_x5", "bins_c70_x5", "bins_c50_x5",
          "bins_c90_x10", "bins_c70_x10", "bins_c50_x10")
NONE = 0xffffffff


def lines_of(text: bytes):
    """the non-empty lines of one add; a '\\r' directly before a '\\n' is not part of its line"""
    parts = bytes(text).split(b"\n")
    out = [p[:-1] if p.endswith(b"\r") else p for p in parts[:-1]] + [parts[-1]]
    return [p for p in out if p]


def name_ok(n: bytes) -> bool:
    return 1 <= len(n) <= 254 and all(c > 0x20 and c != 0x7f for c in n)


def number(f: bytes):
    return int(f) if 1 <= len(f) <= 18 and all(0x30 <= c <= 0x39 for c in f) else None


def pairs(n: int) -> int:
    return n * (n - 1) // 2


class Model:
    def __init__(self, genomes):
        self.names = sorted(g if isinstance(g, bytes) else str(g).encode() for g in genomes)
        self.row = {n: i for i, n in enumerate(self.names)}
        self.n_genomes = len(self.names)
        self.malformed = None
        self.truth = {}        # name -> index
        self.t_genome, self.t_length = [], []
        self.records = []      # (contig index or None, bin name)

    def truth_add(self, text):
        for line in lines_of(text):
            if line.startswith(b"#"):
                continue
            f = line.split(b"\t")
            nums = [number(x) for x in f[1:7]]
            if len(f) < 8 or not name_ok(f[0]) or None in nums or (f[7] != b"." and f[7] not in self.row) or f[0] in self.truth:
                self.malformed = self.malformed or "truth"
                continue
            self.truth[f[0]] = len(self.t_genome)
            self.t_genome.append(self.n_genomes if f[7] == b"." else self.row[f[7]])
            self.t_length.append(nums[0])

    def add(self, text):
        for line in lines_of(text):
            if line[:1] in (b"#", b"@"):
                continue
            f = line.split(b"\t")
            if len(f) < 2 or not name_ok(f[0]) or not name_ok(f[1]):
                self.malformed = self.malformed or "candidate"
                continue
            self.records.append((self.truth.get(f[0]), f[1]))

    def finish(self):
        G, nt = self.n_genomes, len(self.t_genome)
        first, recs = [None] * nt, [0] * nt
        bin_row, bin_first = {}, []
        unknown = 0
        for o, (c, b) in enumerate(self.records):
            if c is None:
                unknown += 1
                continue
            if b not in bin_row:
                bin_row[b] = len(bin_first)
                bin_first.append(o)
            recs[c] += 1
            if first[c] is None:
                first[c] = o
        nb = len(bin_first)
        t_bin = [NONE if f is None else bin_row[self.records[f][1]] for f in first]
        cells = {}
        for i in range(nt):
            if t_bin[i] != NONE:
                k = (t_bin[i], self.t_genome[i])
                n, s = cells.get(k, (0, 0))
                cells[k] = (n + 1, s + self.t_length[i])
        keys = sorted(cells)
        by = np.zeros((G + 1, 7), dtype=np.uint64)
        by[:G, 5] = NONE
        for i in range(nt):
            by[self.t_genome[i], 0] += np.uint64(1)
            by[self.t_genome[i], 1] += np.uint64(self.t_length[i])
        b_contigs, b_bases, b_none, b_real = [0] * nb, [0] * nb, [0] * nb, [0] * nb
        b_top, b_top_bases = [NONE] * nb, [0] * nb
        for (b, g) in keys:                      # ascending: the first to reach a maximum is the lowest row
            n, s = cells[(b, g)]
            b_contigs[b] += n
            b_bases[b] += s
            by[g, 2] += np.uint64(n)
            by[g, 3] += np.uint64(s)
            if g == G:
                b_none[b] += s
                continue
            b_real[b] += n
            by[g, 4] += np.uint64(1)
            if b_top[b] == NONE or s > b_top_bases[b]:
                b_top[b], b_top_bases[b] = g, s
            if int(by[g, 5]) == NONE or s > int(by[g, 6]):
                by[g, 5], by[g, 6] = np.uint64(b), np.uint64(s)
        assigned = [i for i in range(nt) if t_bin[i] != NONE]
        c = dict.fromkeys(COUNTS, 0)
        c.update(truth_records=nt, truth_bases=sum(self.t_length), truth_none=sum(1 for g in self.t_genome if g == G), records=len(self.records),
                 unknown_contig=unknown, repeated=sum(r - 1 for r in recs if r), assigned=len(assigned),
                 assigned_bases=sum(self.t_length[i] for i in assigned), bins=nb, cells=len(keys), sum_top_bases=sum(b_top_bases),
                 sum_best_bases=int(by[:G, 6].sum()), pairs_cells=sum(pairs(cells[k][0]) for k in keys if k[1] != G),
                 pairs_bins=sum(pairs(n) for n in b_real), pairs_genomes=sum(pairs(int(n)) for n in by[:G, 2]))
        for b in range(nb):
            if b_top[b] == NONE:
                continue
            top, bases, truth = b_top_bases[b], b_bases[b], int(by[b_top[b], 1])
            for x in (5, 10):
                for comp in (90, 70, 50):
                    if 100 * top >= comp * truth and 100 * (bases - top) <= x * bases:
                        c[f"bins_c{comp}_x{x}"] += 1
        u32, u64 = np.uint32, np.uint64
        self._read = (c, by)
        self._bins = (np.array(b_contigs, u32), np.array(b_bases, u64), np.array(b_none, u64), np.array(bin_first, u32), np.array(b_top, u32),
                      np.array(b_top_bases, u64))
        self._cells = (np.array([k[0] for k in keys], u32), np.array([k[1] for k in keys], u32), np.array([cells[k][0] for k in keys], u32),
                       np.array([cells[k][1] for k in keys], u64))
        self._contigs = (np.array(self.t_genome, u32), np.array(self.t_length, u64), np.array(t_bin, u32), np.array(recs, u32))
        self.bin_names = [self.records[o][1] for o in bin_first]
        return self

    def read(self):
        return self._read

    def bins(self):
        return self._bins

    def cells(self):
        return self._cells

    def contigs(self):
        return self._contigs


def evaluate(truth_adds, bins_adds, genomes) -> Model:
    m = Model(genomes)
    for t in truth_adds:
        m.truth_add(t)
    if m.malformed is None:
        for t in bins_adds:
            m.add(t)
    return m.finish()


def truth_text(rows, eol=b"\n") -> bytes:
    """rows of (contig name, length, genome name or b'.') as the eight-field text of --eval-assembly-contigs"""
    return b"".join(b"\t".join([n, str(length).encode(), b"7", b"5", b"1", b"0", b"4", g]) + eol for n, length, g in rows)


def bins_text(rows, eol=b"\n") -> bytes:
    return b"".join(c + b"\t" + b + eol for c, b in rows)


def cut_at_every_line_end(text: bytes):
    """one add a line"""
    parts = bytes(text).split(b"\n")
    return [p + b"\n" for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])
