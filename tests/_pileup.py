"""numpy restatement of the allele-count definition of include/simmr_hip.h (simmr_pileup_*): counts[n][2][5] of a site list
over read columns, written from the header's text — a loop over reads with searchsorted on keys built here — and a parser
and a Python formatter of the VCF `simmr-hip --strain-vcf` writes.  Nothing here calls the library."""
import numpy as np

CLASS = np.full(256, 4, dtype=np.int64)
for _i, _b in enumerate(b"ACGT"):
    CLASS[_b] = _i
COMPLEMENT = np.array([3, 2, 1, 0, 4], dtype=np.int64)  # 0 <-> 3, 1 <-> 2, 4 stays
REVCOMP = 1
INFO_LINES = (
    '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads of the run that cover the site (mates count separately)">',
    '##INFO=<ID=AD,Number=R,Type=Integer,Description="Reads that show the reference and the alternate base">',
    '##INFO=<ID=ADF,Number=R,Type=Integer,Description="The same among forward reads">',
    '##INFO=<ID=ADR,Number=R,Type=Integer,Description="The same among reverse reads">',
    '##INFO=<ID=OTH,Number=1,Type=Integer,Description="Reads that show neither: a third base or N">',
)
COLUMNS = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"


def constants():
    """(PILEUP_WG, PILEUP_ROUND, PILEUP_WGS_PER_CU) as simmr_amd/csrc/pileup_kernels.hip states them: the seam tests size their
    reads, rounds and grid trips from these (a value is a decimal number or `1u << k`)"""
    import re
    from pathlib import Path
    src = (Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc" / "pileup_kernels.hip").read_text()
    c = {m.group(1): int(m.group(3)) << int(m.group(4)) if m.group(4) else int(m.group(2))
         for m in re.finditer(r"^constexpr uint32_t (PILEUP_\w+) = (?:(\d+)|(\d+)u << (\d+));", src, re.M)}
    return c["PILEUP_WG"], c["PILEUP_ROUND"], c["PILEUP_WGS_PER_CU"]


def firsts(lens):
    """lens: {genome slot: [contig lengths]} -> {(slot, contig): first position}: slots ascending, contigs in order, no padding"""
    out, at = {}, 0
    for g in sorted(lens):
        for c, n in enumerate(lens[g]):
            out[(g, c)] = at
            at += int(n)
    return out


def site_keys(sites, lens):
    """sites: (genome, contig, pos) arrays -> int64 keys first(slot, contig) + pos; asserts what simmr_pileup_reset demands"""
    f = firsts(lens)
    g, c, p = (np.asarray(x).astype(np.int64) for x in sites)
    for gi, ci, pi in zip(g, c, p):
        assert (int(gi), int(ci)) in f and 0 <= pi < lens[int(gi)][int(ci)], (gi, ci, pi)
    k = np.array([f[(int(gi), int(ci))] + int(pi) for gi, ci, pi in zip(g, c, p)], dtype=np.int64)
    assert np.all(np.diff(k) > 0), "sites are strictly ascending by (slot, contig, pos)"
    return k


def pileup(cols, sites, lens):
    """counts[n][2][5] of the reads of `cols`: seq, seq_off (the read's first base), start, end, contig, genome, flags"""
    f = firsts(lens)
    keys = site_keys(sites, lens)
    counts = np.zeros((keys.size, 2, 5), dtype=np.uint32)
    seq = cols["seq"]
    for r in range(len(cols["start"])):
        a, b = int(cols["start"][r]), int(cols["end"][r])
        lo, L = min(a, b), abs(b - a)
        first = f[(int(cols["genome"][r]), int(cols["contig"][r]))]
        s0, s1 = np.searchsorted(keys, [first + lo, first + lo + L], side="left")
        if s1 == s0:
            continue
        rev = int(cols["flags"][r]) & REVCOMP
        d = keys[s0:s1] - (first + lo)              # pos - lo
        j = L - 1 - d if rev else d
        cls = CLASS[seq[int(cols["seq_off"][r]) + j]]
        np.add.at(counts, (np.arange(s0, s1), 1 if rev else 0, COMPLEMENT[cls] if rev else cls), 1)
    return counts


def vcf_text(sites, ref, alt, counts, names, lens):
    """--strain-vcf FILE; names = {genome slot: (genome id, [sequence ids])}; sites in list order, ref / alt ASCII codes"""
    text = "##fileformat=VCFv4.2\n##source=simmr-hip\n"
    for g in sorted(names):
        gid, sids = names[g]
        for c, sid in enumerate(sids):
            text += f"##contig=<ID={gid}|{sid},length={int(lens[g][c])}>\n"
    text += "\n".join(INFO_LINES) + "\n" + COLUMNS + "\n"
    for s in range(len(sites[2])):
        g, c, p = int(sites[0][s]), int(sites[1][s]), int(sites[2][s])
        gid, sids = names[g]
        k = counts[s].astype(np.int64)
        r, a = int(CLASS[ref[s]]), int(CLASS[alt[s]])
        dp = int(k.sum())
        ad = (int(k[0, r] + k[1, r]), int(k[0, a] + k[1, a]))
        text += (f"{gid}|{sids[c]}\t{p + 1}\t.\t{chr(ref[s])}\t{chr(alt[s])}\t.\t.\tDP={dp};AD={ad[0]},{ad[1]};ADF={k[0, r]},{k[0, a]};"
                 f"ADR={k[1, r]},{k[1, a]};OTH={dp - ad[0] - ad[1]}\n")
    return text


def parse_vcf(text):
    """-> (meta lines without '##', [(id, length)] of the ##contig lines, records as dicts with int / tuple INFO values)"""
    meta, contigs, records, seen_columns = [], [], [], False
    for line in text.splitlines():
        if line.startswith("##"):
            assert not seen_columns, "a meta line behind the column line"
            meta.append(line[2:])
            if line.startswith("##contig=<ID="):
                body = line[len("##contig=<ID="):-1]
                cid, ln = body.rsplit(",length=", 1)
                assert line.endswith(">")
                contigs.append((cid, int(ln)))
            continue
        if line.startswith("#"):
            assert line == COLUMNS and not seen_columns, line
            seen_columns = True
            continue
        assert seen_columns
        f = line.split("\t")
        assert len(f) == 8, line  # no FORMAT / sample columns
        info = {}
        for kv in f[7].split(";"):
            k, v = kv.split("=")
            info[k] = tuple(map(int, v.split(","))) if "," in v else int(v)
        records.append({"chrom": f[0], "pos": int(f[1]), "id": f[2], "ref": f[3], "alt": f[4], "qual": f[5], "filter": f[6], "info": info})
    assert seen_columns
    return meta, contigs, records
