"""The plain restatement of simmr_taxeval_* (include/simmr_hip.h states the rules): a taxonomy, the truth TSV and a classifier's
per-read text to the counts, the two rank tables, the entries and the per-taxon clade sums, in Python and numpy alone — and the
three texts the command line writes from them.  It is the yardstick for the device and for host.cpp's formatters."""
import numpy as np

RANKS, CLASSES, MAX_DEPTH, NONE = 8, 5, 255, -1
MAX_NODES, MAX_GENOMES = 1 << 26, 1 << 24
COUNTS = ("truth_lines", "truth_header", "truth_entries", "truth_paired", "lines", "header", "records", "unknown_read", "unclassified",
          "unknown_taxon", "scored", "missing", "multiple")
RANK_NAMES = ("no_rank", "domain", "phylum", "class", "order", "family", "genus", "species", "strain")
RANK_CODES = dict({n: i for i, n in enumerate(RANK_NAMES) if i}, superkingdom=1)
ABSENT, UNCLASSIFIED, WRONG, ABOVE, CORRECT = range(5)


class Malformed(Exception):
    """a malformed record on either side: SIMMR_EINVAL from the plan (truth) or the read"""


class Refused(Exception):
    """a refusal of the reset or of the plan; .code is the name of the error"""

    def __init__(self, code, what):
        super().__init__(f"{code}: {what}")
        self.code = code


# ---- the texts -----------------------------------------------------------------------------------------------------------------------
def truth_line(read_id, pair, genome_id, rest="\tc1\t0\t100\t+\t100\t0\t") -> bytes:
    """a line of --truth: the three fields that are read, and the others"""
    genome_id = genome_id.decode() if isinstance(genome_id, bytes) else genome_id
    return f"{read_id}\t{pair}\t{genome_id}{rest}\n".encode()


def call(name, taxid, classified=None, names=None, rest="\t150\t0:116") -> bytes:
    """a per-read line of Kraken 2: C or U (U for taxid 0 unless told), the read name, the taxid — as `names (taxid N)` with names"""
    flag = ("C" if taxid else "U") if classified is None else ("C" if classified else "U")
    taxon = f"{names} (taxid {taxid})" if names is not None else f"{taxid}"
    return f"{flag}\t{name}\t{taxon}{rest}\n".encode()


def lines(text: bytes):
    return [ln for ln in bytes(text).split(b"\n") if ln]


def is_header(line: bytes) -> bool:
    return line[:1] == b"#" or line.startswith(b"read_id\t")


def number(field: bytes, most: int):
    """the value of 1 to `most` digits; None: not that"""
    return int(field) if 1 <= len(field) <= most and field.isdigit() and field.isascii() else None


def read_id(name: bytes):
    if len(name) >= 3 and name[-2:] in (b"/1", b"/2"):
        name = name[:-2]
    return number(name, 18)


def taxon(field: bytes):
    if field.endswith(b")"):
        digits = len(field) - 1
        while digits > 0 and len(field) - 1 - digits < 11 and field[digits - 1:digits].isdigit():
            digits -= 1
        if digits < 7 or field[digits - 7:digits] != b"(taxid ":
            return None
        field = field[digits:-1]
    v = number(field, 10)
    return v if v is not None and v < 2 ** 32 else None


# ---- the tree ------------------------------------------------------------------------------------------------------------------------
class Tree:
    def __init__(self, taxonomy, genomes):
        taxid, parent, rank = ([int(v) for v in a] for a in taxonomy)
        if len(taxid) > MAX_NODES:
            raise Refused("ERANGE", "more than 2^26 nodes")
        if len(genomes) > MAX_GENOMES:
            raise Refused("ERANGE", "more than 2^24 genomes")
        ids = [g if isinstance(g, bytes) else str(g).encode() for g, _ in genomes]
        for g in ids:
            if not 1 <= len(g) <= 254 or b"\t" in g or b"\n" in g or b"\0" in g:
                raise Refused("ENOTSUP", "a genome id that is empty, too long or holds a tab or a newline")
        if len(set(ids)) != len(ids):
            raise Refused("EINVAL", "a genome id given twice")
        if 0 in taxid:
            raise Refused("EINVAL", "a taxid of 0")
        if len(set(taxid)) != len(taxid):
            raise Refused("EINVAL", "a taxid given twice")
        if any(r > RANKS for r in rank):
            raise Refused("EINVAL", "a rank code above 8")
        order = sorted(range(len(taxid)), key=taxid.__getitem__)
        self.taxid = [taxid[i] for i in order]
        self.rank = [rank[i] for i in order]
        self.row = {t: i for i, t in enumerate(self.taxid)}
        self.n = len(order)
        self.parent = []
        for i, k in enumerate(order):
            p = parent[k]
            if p == 0 or p == taxid[k]:
                self.parent.append(i)
            elif p in self.row:
                self.parent.append(self.row[p])
            else:
                raise Refused("EINVAL", "a parent that is no node")
        self.depth, self.anc = [0] * self.n, [[NONE] * RANKS for _ in range(self.n)]
        for i in range(self.n):
            cur, d = i, 0
            while True:
                r = self.rank[cur]
                if r:
                    if self.anc[i][r - 1] != NONE:
                        raise Refused("EINVAL", "a lineage that holds one rank twice")
                    self.anc[i][r - 1] = cur
                if self.parent[cur] == cur:
                    break
                if d == MAX_DEPTH:
                    raise Refused("EINVAL", "no root within 255 steps")
                cur, d = self.parent[cur], d + 1
            self.depth[i] = d
        pairs = sorted(zip(ids, (int(t) for _, t in genomes)))
        self.genome_ids = [g for g, _ in pairs]
        self.genome_row = {g: i for i, g in enumerate(self.genome_ids)}
        self.genome_node = []
        for _, t in pairs:
            if t == 0 or t not in self.row:
                raise Refused("EINVAL", "a genome whose taxid is no node")
            self.genome_node.append(self.row[t])

    def lineage(self, taxid):
        """(the taxids of the ancestor-or-self at the 8 ranks, 0: none; the depth)"""
        i = self.row[taxid]
        return [self.taxid[a] if a != NONE else 0 for a in self.anc[i]], self.depth[i]

    def lca(self, a, b):
        da, db = self.depth[a], self.depth[b]
        while da > db:
            a, da = self.parent[a], da - 1
        while db > da:
            b, db = self.parent[b], db - 1
        while a != b and da > 0:
            a, b, da = self.parent[a], self.parent[b], da - 1
        return a if a == b else NONE

    def classes(self, t, kind, c=NONE, lca=NONE):
        """the class of each rank for a record of the kind UNCLASSIFIED, WRONG (a taxid that is no node) or CORRECT (scored)"""
        out = []
        for r in range(RANKS):
            at = self.anc[t][r]
            if at == NONE:
                out.append(ABSENT)
            elif kind != CORRECT:
                out.append(kind)
            else:
                ac = self.anc[c][r]
                out.append((CORRECT if ac == at else WRONG) if ac != NONE else (ABOVE if lca == c else WRONG))
        return out


# ---- the evaluation ------------------------------------------------------------------------------------------------------------------
class Evaluation:
    def __init__(self, truth_pieces, call_pieces, taxonomy, genomes):
        T = self.tree = Tree(taxonomy, genomes)
        self.counts = dict.fromkeys(COUNTS, 0)
        c = self.counts
        # the truth: the lines, then the plan
        seen_lines, malformed = [], False
        for piece in truth_pieces:
            for ln in lines(piece):
                c["truth_lines"] += 1
                if is_header(ln):
                    c["truth_header"] += 1
                    continue
                f = ln.split(b"\t")
                rid = number(f[0], 18) if len(f) >= 3 else None
                if rid is None or f[1] not in (b"0", b"1", b"2") or f[2] not in T.genome_row:
                    malformed = True
                    continue
                seen_lines.append((rid, T.genome_row[f[2]]))
        if malformed:
            raise Malformed("a truth record")
        if len(seen_lines) >= 2 ** 31:
            raise Refused("ERANGE", "2^31 truth lines or more")
        by_id = {}
        for rid, g in seen_lines:
            by_id.setdefault(rid, []).append(g)
        if any(len(g) > 2 for g in by_id.values()):
            raise Refused("EINVAL", "more than two lines with one id")
        if any(len(set(g)) > 1 for g in by_id.values()):
            raise Refused("EINVAL", "one id with two genomes")
        self.id = np.array(sorted(by_id), dtype=np.uint64)
        self.genome = np.array([by_id[int(i)][0] for i in self.id], dtype=np.uint32)
        self.mates = np.array([len(by_id[int(i)]) for i in self.id], dtype=np.uint32)
        entry = {int(i): k for k, i in enumerate(self.id)}
        n = len(self.id)
        c["truth_entries"], c["truth_paired"] = n, int((self.mates == 2).sum())
        # the candidate
        self.seen, self.hits = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self.by_rank = np.zeros((RANKS, CLASSES), dtype=np.uint64)
        self.direct = np.zeros((3, max(T.n, 1)), dtype=np.uint64)   # true, called, both
        self.malformed = False
        for piece in call_pieces:
            for ln in lines(piece):
                c["lines"] += 1
                if is_header(ln):
                    c["header"] += 1
                    continue
                f = ln.split(b"\t")
                tax = taxon(f[2]) if len(f) >= 3 and f[0] in (b"C", b"U") else None
                if tax is None:
                    self.malformed = True
                    continue
                c["records"] += 1
                rid = read_id(f[1])
                if rid is None or rid not in entry:
                    c["unknown_read"] += 1
                    continue
                e = entry[rid]
                t = T.genome_node[self.genome[e]]
                self.direct[0, t] += 1
                if f[0] == b"U" or tax == 0:
                    c["unclassified"] += 1
                    cls = T.classes(t, UNCLASSIFIED)
                elif tax not in T.row:
                    c["unknown_taxon"] += 1
                    cls = T.classes(t, WRONG)
                else:
                    c["scored"] += 1
                    cn = T.row[tax]
                    lca = T.lca(t, cn)
                    cls = T.classes(t, CORRECT, cn, lca)
                    self.direct[1, cn] += 1
                    if lca != NONE:
                        self.direct[2, lca] += 1
                self.hits[e] += 1
                for r, k in enumerate(cls):
                    self.by_rank[r, k] += 1
                    if k:
                        self.seen[e] |= np.uint32(1 << (4 * r + k - 1))
        # the entries by their best class
        self.reads_by_rank = np.zeros((RANKS, CLASSES), dtype=np.uint64)
        for e in range(n):
            for r, k in enumerate(self.best(e)):
                self.reads_by_rank[r, k] += 1
        c["missing"] = int((self.hits == 0).sum())
        c["multiple"] = int((self.hits > self.mates).sum())

    def best(self, e):
        """the best class of entry e at each rank"""
        if self.hits[e] == 0:
            return [UNCLASSIFIED if a != NONE else ABSENT for a in self.tree.anc[self.tree.genome_node[self.genome[e]]]]
        return [int((int(self.seen[e]) >> (4 * r)) & 15).bit_length() for r in range(RANKS)]

    def read(self):
        if self.malformed:
            raise Malformed("a candidate record")
        return dict(self.counts), self.by_rank.copy(), self.reads_by_rank.copy()

    def reads(self):
        return self.id.copy(), self.genome.copy(), self.mates.copy(), self.seen.copy(), self.hits.copy()

    def taxa(self):
        """(taxid, true, called, both): the clade sums in taxid order"""
        T = self.tree
        clade = np.zeros((3, T.n), dtype=np.uint64)
        for i in range(T.n):
            if self.direct[:, i].any():
                cur = i
                while True:
                    clade[:, cur] += self.direct[:, i]
                    if T.parent[cur] == cur:
                        break
                    cur = T.parent[cur]
        return (np.array(T.taxid, dtype=np.uint32),) + tuple(clade[k] for k in range(3))

    def lineage(self, taxid):
        return self.tree.lineage(taxid)


def evaluate(truth_pieces, call_pieces, taxonomy, genomes) -> Evaluation:
    return Evaluation(truth_pieces, call_pieces, taxonomy, genomes)


# ---- a small synthetic tree ------------------------------------------------------------------------------------------------------------
def tree_of(rows):
    """rows of (taxid, parent, rank name or code) -> the taxonomy triple"""
    code = [RANK_CODES.get(r, 0) if isinstance(r, str) else int(r) for _, _, r in rows]
    return (np.array([t for t, _, _ in rows], dtype=np.uint32), np.array([p for _, p, _ in rows], dtype=np.uint32), np.array(code, dtype=np.uint8))


SMALL_ROWS = [   # given out of taxid order on purpose
    (61, 60, "strain"), (62, 60, "strain"), (60, 50, "species"), (70, 50, "species"),
    (55, 50, "clade"), (71, 55, "species"),                      # an unranked clade between a genus and a species
    (50, 40, "genus"), (80, 40, "genus"), (81, 80, "species"), (45, 40, "no rank"),   # 45: an unranked clade off every genome's path
    (40, 30, "family"), (30, 20, "order"), (20, 10, "class"), (10, 2, "phylum"), (2, 1, "superkingdom"),
    (3, 1, "domain"), (90, 3, "species"),                        # a lineage without phylum .. genus
    (1, 1, "no rank"),
]
SMALL_GENOMES = [("gStrain", 61), ("gSpecies", 60), ("gClade", 71), ("gOther", 81), ("gArch", 90)]


def small_tree():
    """(taxonomy, genomes): two domains under one root, every rank, two unranked clades, a lineage that lacks ranks"""
    return tree_of(SMALL_ROWS), list(SMALL_GENOMES)


def chain(depth, first=1):
    """a chain whose deepest node has `depth` steps to the root: taxids first .. first + depth, no ranks but species at the end"""
    rows = [(first, first, 0)] + [(first + d, first + d - 1, 7 if d == depth else 0) for d in range(1, depth + 1)]
    return tree_of(rows)


# ---- the texts of the command line -----------------------------------------------------------------------------------------------------
def ratio(a, b) -> str:
    return "NA" if b == 0 else "%.6f" % (float(a) / float(b))


def prf(k) -> str:
    """precision, sensitivity and F1 of one row of five class counts"""
    scored = int(k[UNCLASSIFIED]) + int(k[WRONG]) + int(k[ABOVE]) + int(k[CORRECT])
    cw = int(k[CORRECT]) + int(k[WRONG])
    if cw == 0 or scored == 0:
        f1 = "NA"
    else:
        p, s = float(int(k[CORRECT])) / float(cw), float(int(k[CORRECT])) / float(scored)
        f1 = "NA" if p + s == 0.0 else "%.6f" % (2.0 * p * s / (p + s))
    return f"{ratio(int(k[CORRECT]), cw)}\t{ratio(int(k[CORRECT]), scored)}\t{f1}"


def report(counts, by_rank, reads_by_rank, rank, true, called) -> bytes:
    """the file of --eval-classified-report; rank, true, called: per node in taxid order"""
    out = "".join(f"#{n}\t{counts[n]}\n" for n in COUNTS)
    out += "#R\trank\tname\t" + "\t".join(f"{w}_{k}" for w in ("records", "reads") for k in ("absent", "unclassified", "wrong", "above", "correct")) + "\n"
    for r in range(RANKS):
        out += f"R\t{r + 1}\t{RANK_NAMES[r + 1]}\t" + "\t".join(str(int(v)) for v in list(by_rank[r]) + list(reads_by_rank[r])) + "\n"
    out += "#P\trank\tname\trecords_precision\trecords_sensitivity\trecords_f1\treads_precision\treads_sensitivity\treads_f1\n"
    for r in range(RANKS):
        out += f"P\t{r + 1}\t{RANK_NAMES[r + 1]}\t{prf(by_rank[r])}\t{prf(reads_by_rank[r])}\n"
    out += "#A\trank\tname\tnodes\tl1_distance\n"
    for r in range(1, RANKS + 1):
        at = [i for i in range(len(rank)) if rank[i] == r]
        st, sc = sum(int(true[i]) for i in at), sum(int(called[i]) for i in at)
        l1 = 0.0
        for i in at:
            if st and sc:
                l1 += abs(float(int(true[i])) / float(st) - float(int(called[i])) / float(sc))
        out += f"A\t{r}\t{RANK_NAMES[r]}\t{len(at)}\t" + ("%.6f" % l1 if st and sc else "NA") + "\n"
    return out.encode()


def read_rows(genome_ids, genome_has, rid, genome, mates, seen, hits) -> bytes:
    """the rows of --eval-classified-reads; genome_has[row]: bit r - 1 set where the genome's lineage has rank r"""
    out = []
    for e in range(len(rid)):
        g = int(genome[e])
        if hits[e] == 0:
            best = [1 if genome_has[g] >> r & 1 else 0 for r in range(RANKS)]
        else:
            best = [((int(seen[e]) >> (4 * r)) & 15).bit_length() for r in range(RANKS)]
        out.append(b"%d\t%s\t%d\t%d\t" % (int(rid[e]), genome_ids[g], int(mates[e]), int(hits[e])) + "\t".join(map(str, best)).encode() + b"\n")
    return b"".join(out)


def taxa_rows(taxid, rank, true, called, both) -> bytes:
    """the rows of --eval-classified-taxa: the nodes with a clade sum that is not zero"""
    out = ""
    for i in range(len(taxid)):
        t, c, b = int(true[i]), int(called[i]), int(both[i])
        if t or c or b:
            out += f"{int(taxid[i])}\t{RANK_NAMES[int(rank[i])]}\t{t}\t{c}\t{b}\t{ratio(b, c)}\t{ratio(b, t)}\n"
    return out.encode()


def genome_has(ev: Evaluation):
    T = ev.tree
    return [sum(1 << r for r in range(RANKS) if T.anc[node][r] != NONE) for node in T.genome_node]
