"""The plain model of simmr_asmmap_* (include/simmr_hip.h states the rules): Python dictionaries over strings and a loop per
contig.  A k-mer is a str of k letters and its key the smaller of it and its reverse complement AS STRINGS, as in tests/_asmeval.py,
whose text rules (records, genome_of, Malformed, fasta) are taken as they are; nothing here packs, rolls, sorts or scans.  The
report, the block rows, the contig rows and NGA50 of the command line are stated here too."""
import numpy as np

from tests._asmeval import Malformed, fasta, fasta_records, genome_of, invalid_bases, key_value, records, revcomp, revcomp_bytes  # noqa: F401

COUNTS = ("truth_records", "truth_bases", "truth_invalid", "truth_kmers", "truth_anchors", "truth_repeats", "records", "bases", "invalid", "kmers",
          "hits", "stray_hits", "repeat_hits", "runs", "runs_dropped", "blocks", "block_bases", "breaks_inter_genome", "breaks_inter_record",
          "breaks_inversion", "breaks_relocation", "breaks_local", "contigs_unplaced", "contigs_clean", "contigs_local_only", "contigs_misassembled",
          "misassembled_bases")
GENOME_COLS = ("truth_bases", "truth_anchors", "blocks", "block_bases", "longest_block")
BLOCK_COLS = ("contig", "truth_record", "strand", "q_start", "q_end", "p_start", "p_end", "hits", "join")
JOINS = ("none", "inter_genome", "inter_record", "inversion", "relocation", "local")
NONE = 0xFFFFFFFF


def placed_kmers(seq: bytes, k: int):
    """(key, position of the first base, 1 where the key is the reverse complement) of the k-mers of one record, in position order"""
    s = seq.decode("latin-1").upper()
    bad = -1
    for i, ch in enumerate(s):
        if ch not in "ACGT":
            bad = i
        elif i - bad >= k:
            kmer = s[i - k + 1:i + 1]
            rc = revcomp(kmer)
            yield (kmer, i - k + 1, 0) if kmer < rc else (rc, i - k + 1, 1)


class Model:
    def __init__(self, genomes, k, band=64, relocation=1000, min_anchors=16):
        names = sorted(g if isinstance(g, bytes) else str(g).encode() for g in genomes)
        self.names, self.rows, self.k = names, {n: i for i, n in enumerate(names)}, k
        self.band, self.relocation, self.min_anchors = band, relocation, min_anchors
        self.counts = dict.fromkeys(COUNTS, 0)
        self.occ = {}           # key -> [(t, p, o)]
        self.truth_genome = []  # per truth record
        self.truth_length = []
        self.plan()

    def truth_add(self, text):
        for header, seq in records(text):
            g = genome_of(header, self.rows)
            t = len(self.truth_genome)
            self.truth_genome.append(g)
            self.truth_length.append(len(seq))
            self.counts["truth_records"] += 1
            self.counts["truth_bases"] += len(seq)
            self.counts["truth_invalid"] += invalid_bases(seq)
            for key, p, o in placed_kmers(seq, self.k):
                self.counts["truth_kmers"] += 1
                self.occ.setdefault(key, []).append((t, p, o))

    def plan(self):
        self.anchor = {key: v[0] for key, v in self.occ.items() if len(v) == 1}
        self.repeat = {key for key, v in self.occ.items() if len(v) > 1}
        self.contig_rows = []   # [length, hits, blocks, first_block, block_bases, worst_join]
        self.block_rows = []    # the nine columns
        for name in COUNTS[6:]:
            self.counts[name] = 0
        self.counts["truth_anchors"], self.counts["truth_repeats"] = len(self.anchor), len(self.repeat)
        return len(self.anchor)

    def _new_run(self, a, b):
        """a, b: hits (q, t, s, d, p) that follow each other"""
        return a[1] != b[1] or a[2] != b[2] or abs(a[3] - b[3]) > self.band

    def add(self, text):
        c = self.counts
        for _, seq in records(text):
            row = len(self.contig_rows)
            c["records"] += 1
            c["bases"] += len(seq)
            c["invalid"] += invalid_bases(seq)
            hits = []
            for key, q, oc in placed_kmers(seq, self.k):
                c["kmers"] += 1
                if key in self.anchor:
                    t, p, o = self.anchor[key]
                    s = oc ^ o
                    hits.append((q, t, s, p + q if s else p - q, p))
                elif key in self.repeat:
                    c["repeat_hits"] += 1
            c["hits"] += len(hits)
            runs = []
            for h in hits:
                if not runs or self._new_run(runs[-1][-1], h):
                    runs.append([])
                runs[-1].append(h)
            c["runs"] += len(runs)
            kept = [r for r in runs if len(r) >= self.min_anchors]
            c["runs_dropped"] += len(runs) - len(kept)
            c["stray_hits"] += sum(len(r) for r in runs if len(r) < self.min_anchors)
            blocks = []
            for r in kept:
                if not blocks or self._new_run(blocks[-1][-1], r[0]):
                    blocks.append([])
                blocks[-1] += r
            first, joins = len(self.block_rows), []
            for i, b in enumerate(blocks):
                join = 0
                if i:
                    a, z = blocks[i - 1][-1], b[0]
                    if self.truth_genome[a[1]] != self.truth_genome[z[1]]:
                        join = 1
                    elif a[1] != z[1]:
                        join = 2
                    elif a[2] != z[2]:
                        join = 3
                    else:
                        join = 4 if abs(a[3] - z[3]) > self.relocation else 5
                joins.append(join)
                self.block_rows.append([row, b[0][1], b[0][2], b[0][0], b[-1][0] + self.k, min(h[4] for h in b), max(h[4] for h in b) + self.k,
                                        len(b), join])
            bases = sum(b[-1][0] + self.k - b[0][0] for b in blocks)
            self.contig_rows.append([len(seq), len(hits), len(blocks), first if blocks else NONE, bases, min([j for j in joins if j], default=0)])

    def read(self):
        c = dict(self.counts)
        by = np.zeros((len(self.names), len(GENOME_COLS)), dtype=np.uint64)
        for g, length in zip(self.truth_genome, self.truth_length):
            by[g, 0] += length
        for t, _, _ in self.anchor.values():
            by[self.truth_genome[t], 1] += 1
        for b in self.block_rows:
            g, length = self.truth_genome[b[1]], b[4] - b[3]
            c["blocks"] += 1
            c["block_bases"] += length
            if b[8]:
                c["breaks_" + JOINS[b[8]]] += 1
            by[g, 2] += 1
            by[g, 3] += length
            by[g, 4] = max(int(by[g, 4]), length)
        for length, _, blocks, _, _, worst in self.contig_rows:
            cls = "contigs_unplaced" if blocks == 0 else "contigs_clean" if blocks == 1 else "contigs_local_only" if worst == 5 else "contigs_misassembled"
            c[cls] += 1
            if cls == "contigs_misassembled":
                c["misassembled_bases"] += length
        return c, by

    def anchors(self):
        order = sorted(self.anchor)
        cols = [[self.anchor[key][i] for key in order] for i in range(3)]
        return (np.array([key_value(key) for key in order], dtype=np.uint64),) + tuple(np.array(x, dtype=np.uint32) for x in cols)

    def blocks(self):
        cols = list(zip(*self.block_rows)) if self.block_rows else [[]] * 9
        return tuple(np.array(x, dtype=np.uint32) for x in cols)

    def contigs(self):
        cols = list(zip(*self.contig_rows)) if self.contig_rows else [[]] * 6
        return tuple(np.array(cols[i], dtype=np.uint64 if i in (0, 4) else np.uint32) for i in range(6))


def evaluate(truth_pieces, contig_pieces, genomes, k=31, band=64, relocation=1000, min_anchors=16):
    m = Model(genomes, k, band, relocation, min_anchors)
    for t in truth_pieces:
        m.truth_add(t)
    m.plan()
    for t in contig_pieces:
        m.add(t)
    return m


def invariants(m):
    """what stays the same under any cut into adds and under the reverse complement of any contig"""
    c, by = m.read()
    b = m.blocks()
    rows = sorted(zip(*[x.tolist() for x in (b[0], b[1], b[7], b[4] - b[3], b[5], b[6])]))
    cc = m.contigs()
    return c, by.tolist(), [cc[i].tolist() for i in (0, 1, 2, 4, 5)], rows


def nga50(block_lengths, target):
    """the length of the block at which the lengths, longest first, reach half of `target`; None where they never do"""
    run = 0
    for x in sorted((int(v) for v in block_lengths), reverse=True):
        run += x
        if 2 * run >= target:
            return x
    return None


def report_text(counts, by_genome, names, k, band, relocation, min_anchors, block_lengths, block_genomes):
    """the file of --eval-placement-report (simmr_amd/host/simmr_host.hpp: asmmap_report); block_genomes[i] is the genome row of
    block i's truth record"""
    show = lambda v: "NA" if v is None else "%d" % v
    out = ["#%s\t%d\n" % (n, counts[n]) for n in COUNTS]
    out += ["#k\t%d\n" % k, "#band\t%d\n" % band, "#relocation\t%d\n" % relocation, "#min_anchors\t%d\n" % min_anchors]
    out.append("#misassemblies\t%d\n" % sum(counts["breaks_" + j] for j in JOINS[1:5]))
    out.append("#NA50\t%s\n" % show(nga50(block_lengths, counts["bases"]) if counts["bases"] else None))
    out.append("#NGA50\t%s\n" % show(nga50(block_lengths, counts["truth_bases"]) if counts["truth_bases"] else None))
    out.append("#G\tgenome\ttruth_bases\ttruth_anchors\tblocks\tblock_bases\tlongest_block\tNGA50\tanchored\n")
    for g, name in enumerate(names):
        r = [int(x) for x in by_genome[g]]
        own = [l for l, bg in zip(block_lengths, block_genomes) if bg == g]
        out.append("G\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (name if isinstance(name, str) else name.decode(), *r,
                                                            show(nga50(own, r[0]) if r[0] else None), "NA" if r[0] == 0 else "%.6f" % (r[3] / r[0])))
    return "".join(out)


def block_rows_text(contig_names, truth_names, cols):
    """the file of --eval-placement-blocks (asmmap_block_rows)"""
    out = []
    for i in range(len(cols[0])):
        c, t = int(cols[0][i]), int(cols[1][i])
        out.append("%s\t%d\t%d\t%s\t%d\t%d\t%s\t%d\t%s\n" % (contig_names[c] if c < len(contig_names) else "?", int(cols[3][i]), int(cols[4][i]),
                                                             truth_names[t] if t < len(truth_names) else "?", int(cols[5][i]), int(cols[6][i]),
                                                             "-" if int(cols[2][i]) else "+", int(cols[7][i]), JOINS[int(cols[8][i])]))
    return "".join(out)


def contig_rows_text(contig_names, cols):
    """the file of --eval-placement-contigs (asmmap_contig_rows): name, length, hits, blocks, first_block, block_bases, worst join by name"""
    out = []
    for i in range(len(cols[0])):
        out.append("%s\t%d\t%d\t%d\t%d\t%d\t%s\n" % (contig_names[i] if i < len(contig_names) else "?", *[int(cols[j][i]) for j in range(5)], JOINS[int(cols[5][i])]))
    return "".join(out)
