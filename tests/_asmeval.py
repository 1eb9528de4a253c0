"""The plain model of simmr_asmeval_* (include/simmr_hip.h states the rules): Python dictionaries over strings.  A k-mer is a
str of k letters, its key the smaller of it and its reverse complement AS STRINGS (A < C < G < T is the order of the 2-bit
values, first base first), so nothing here packs, rolls or sorts as the kernels do.  Only `key_value` turns a key into the
number the device's key column holds."""
import math

import numpy as np

COUNTS = ("truth_records", "truth_bases", "truth_invalid", "truth_kmers", "truth_distinct", "truth_shared_distinct", "records", "bases", "invalid",
          "kmers", "found", "shared", "novel", "contigs_short", "contigs_novel", "contigs_pure", "contigs_mixed", "contigs_shared_only")
GENOME_COLS = ("distinct", "distinct_found", "over", "contigs", "contig_bases")
NONE = 0xFFFFFFFF
_COMP = str.maketrans("ACGT", "TGCA")


class Malformed(Exception):
    pass


def revcomp(s: str) -> str:
    return s.translate(_COMP)[::-1]


def revcomp_bytes(seq: bytes) -> bytes:
    """the reverse complement of a sequence whose other bytes stay where the reversal puts them"""
    return seq.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


def key_value(kmer: str) -> int:
    return int(kmer.translate(str.maketrans("ACGT", "0123")), 4)


def records(text: bytes):
    """[(header line without '>', sequence)] of one add; Malformed for a sequence line with a base in front of the first header"""
    out = []
    lines = bytes(text).split(b"\n")
    for i, line in enumerate(lines):
        if i + 1 < len(lines) and line.endswith(b"\r"):  # (the last piece has no '\n' behind it)
            line = line[:-1]
        if not line:
            continue
        if line.startswith(b">"):
            out.append([line[1:], b""])
        elif not out:
            raise Malformed("a sequence line in front of the first header")
        else:
            out[-1][1] += line
    return [(h, s) for h, s in out]


def canonical_kmers(seq: bytes, k: int):
    """the keys of the k-mers of one record, in position order"""
    s = seq.decode("latin-1").upper()
    bad = -1
    for i, ch in enumerate(s):
        if ch not in "ACGT":
            bad = i
        elif i - bad >= k:
            kmer = s[i - k + 1:i + 1]
            yield min(kmer, revcomp(kmer))


def invalid_bases(seq: bytes) -> int:
    return sum(1 for ch in seq.decode("latin-1").upper() if ch not in "ACGT")


def genome_of(header: bytes, rows: dict) -> int:
    word = header.split(b" ")[0].split(b"\t")[0].split(b"\r")[0]
    if b"|" not in word or word.split(b"|")[0] not in rows:
        raise Malformed(f"header {header!r}")
    return rows[word.split(b"|")[0]]


class Model:
    def __init__(self, genomes, k):
        names = sorted(g if isinstance(g, bytes) else str(g).encode() for g in genomes)
        self.names, self.rows, self.k = names, {n: i for i, n in enumerate(names)}, k
        self.counts = dict.fromkeys(COUNTS, 0)
        self.occ = {}      # key -> [mult, {genome rows}]
        self.truth_lengths = []
        self.plan()

    def truth_add(self, text):
        for header, seq in records(text):
            g = genome_of(header, self.rows)
            self.counts["truth_records"] += 1
            self.counts["truth_bases"] += len(seq)
            self.counts["truth_invalid"] += invalid_bases(seq)
            self.truth_lengths.append(len(seq))
            for key in canonical_kmers(seq, self.k):
                self.counts["truth_kmers"] += 1
                e = self.occ.setdefault(key, [0, set()])
                e[0] += 1
                e[1].add(g)

    def plan(self):
        G = len(self.names)
        self.order = sorted(self.occ)
        self.genome = {key: (next(iter(gs)) if len(gs) == 1 else G) for key, (_, gs) in self.occ.items()}
        self.hits = dict.fromkeys(self.order, 0)
        self.rows_of_contigs = []  # [length, kmers, found, shared, top_genome, top_kmers, genomes voted for]
        for name in COUNTS[6:]:
            self.counts[name] = 0
        return len(self.order)

    def add(self, text):
        G = len(self.names)
        for _, seq in records(text):
            kmers = found = shared = 0
            votes = {}
            for key in canonical_kmers(seq, self.k):
                kmers += 1
                if key not in self.genome:
                    continue
                found += 1
                self.hits[key] += 1
                g = self.genome[key]
                if g == G:
                    shared += 1
                else:
                    votes[g] = votes.get(g, 0) + 1
            top = min(votes, key=lambda g: (-votes[g], g)) if votes else NONE
            self.rows_of_contigs.append([len(seq), kmers, found, shared, top, votes.get(top, 0), len(votes)])
            self.counts["invalid"] += invalid_bases(seq)

    def read(self):
        G = len(self.names)
        c = dict(self.counts)
        by = np.zeros((G + 1, len(GENOME_COLS)), dtype=np.uint64)
        for key in self.order:
            g = self.genome[key]
            by[g, 0] += 1
            by[g, 1] += 1 if self.hits[key] > 0 else 0
            by[g, 2] += 1 if self.hits[key] > self.occ[key][0] else 0
        c["truth_distinct"] = len(self.order)
        c["truth_shared_distinct"] = int(by[G, 0])
        for length, kmers, found, shared, top, _, voted in self.rows_of_contigs:
            c["records"] += 1
            c["bases"] += length
            c["kmers"] += kmers
            c["found"] += found
            c["shared"] += shared
            cls = ("contigs_short" if kmers == 0 else "contigs_novel" if found == 0 else "contigs_shared_only" if voted == 0 else
                   "contigs_pure" if voted == 1 else "contigs_mixed")
            c[cls] += 1
            if top != NONE:
                by[top, 3] += 1
                by[top, 4] += length
        c["novel"] = c["kmers"] - c["found"]
        return c, by

    def entries(self):
        return (np.array([key_value(k) for k in self.order], dtype=np.uint64), np.array([self.genome[k] for k in self.order], dtype=np.uint32),
                np.array([self.occ[k][0] for k in self.order], dtype=np.uint32), np.array([self.hits[k] for k in self.order], dtype=np.uint32))

    def contigs(self):
        cols = list(zip(*self.rows_of_contigs)) if self.rows_of_contigs else [[]] * 7
        return (np.array(cols[0], dtype=np.uint64),) + tuple(np.array(cols[i], dtype=np.uint32) for i in range(1, 6))


def evaluate(truth_pieces, contig_pieces, genomes, k=31):
    m = Model(genomes, k)
    for t in truth_pieces:
        m.truth_add(t)
    m.plan()
    for t in contig_pieces:
        m.add(t)
    return m


def n50(lengths):
    """(records, bases, longest, N50): N50 is the length of the record at which the lengths, longest first, reach half the bases"""
    ls = sorted((int(x) for x in lengths), reverse=True)
    total, run = sum(ls), 0
    for x in ls:
        run += x
        if 2 * run >= total:
            return len(ls), total, ls[0], x
    return 0, 0, 0, 0


def qv(novel, kmers, k):
    """the consensus quality -10 log10(1 - (1 - novel / kmers)^(1/k)) as the report prints it"""
    if kmers == 0:
        return "NA"
    if novel == 0:
        return "inf"
    return "%.4f" % (-10.0 * math.log10(1.0 - (1.0 - novel / kmers) ** (1.0 / k)))


def fasta(recs, width=60, eol=b"\n"):
    """[(name, sequence bytes)] as FASTA text"""
    out = []
    for name, seq in recs:
        out.append(b">" + (name if isinstance(name, bytes) else name.encode()) + eol)
        out += [seq[j:j + width] + eol for j in range(0, len(seq), width)]
    return b"".join(out)


def fasta_records(text: bytes):
    """([first word of every header], [bases of every record]) as the host reads a file"""
    recs = records(text)
    return [h.split(b" ")[0].split(b"\t")[0].split(b"\r")[0].decode() for h, _ in recs], [len(s) for _, s in recs]


def report_text(counts, by_genome, names, k, truth_lengths, contig_lengths):
    """the file of --eval-assembly-report (simmr_amd/host/simmr_host.hpp: asmeval_report)"""
    frac = lambda a, b: "NA" if b == 0 else "%.6f" % (a / b)
    out = ["#%s\t%d\n" % (n, counts[n]) for n in COUNTS]
    out.append("#k\t%d\n" % k)
    d, f = int(by_genome[:, 0].sum()), int(by_genome[:, 1].sum())
    out.append("#completeness\t%d/%d\t%s\n" % (f, d, frac(f, d)))
    out.append("#qv\t%s\n" % qv(counts["novel"], counts["kmers"], k))
    out.append("#truth_contiguity\t%d\t%d\t%d\t%d\n" % n50(truth_lengths))
    out.append("#contigs_contiguity\t%d\t%d\t%d\t%d\n" % n50(contig_lengths))
    out.append("#G\tgenome\tdistinct\tdistinct_found\tover\tcontigs\tcontig_bases\tcompleteness\n")
    for g, name in enumerate(list(names) + ["shared"]):
        r = [int(x) for x in by_genome[g]]
        out.append("G\t%s\t%d\t%d\t%d\t%d\t%d\t%s\n" % (name if isinstance(name, str) else name.decode(), *r, frac(r[1], r[0])))
    return "".join(out)


def contig_rows(names, genomes, cols):
    """the file of --eval-assembly-contigs (asmeval_contig_rows)"""
    out = []
    for i in range(len(cols[0])):
        g = int(cols[4][i])
        gname = genomes[g] if g < len(genomes) else "."
        out.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (names[i] if i < len(names) else "?", *[int(c[i]) for c in cols],
                                                              gname if isinstance(gname, str) else gname.decode()))
    return "".join(out)
