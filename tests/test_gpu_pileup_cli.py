"""`simmr-hip --with-ani N --strain-sites S --strain-vcf V` on the GPU box: the columns of the run are rebuilt from the FASTQ's
headers and sequences, the numpy restatement (tests/_pileup.py) is applied to them at the sites of S, and every record of V —
and its ##contig lines — must be what that gives."""
import re
import subprocess

import numpy as np
import pytest

from tests import _pileup
from tests.test_gpu_cli import EXE, workdir  # noqa: F401  (the two-genome FASTA fixture)

pytestmark = pytest.mark.gpu
HEADER = re.compile(rb"@(\d+)\|(\S+)/([12]) metadata:sid=(.*)\|sp=(\d+)\|ep=(\d+)\|rc=([tf])$")


def columns_of(fastq, names):
    """the read columns the FASTQ text holds; names = {genome slot: (genome id, [sequence ids])}"""
    slot = {gid: g for g, (gid, _) in names.items()}
    lines = fastq.split(b"\n")
    cols = {k: [] for k in ("start", "end", "contig", "genome", "flags")}
    seqs = []
    for h, s in zip(lines[0::4], lines[1::4]):
        m = HEADER.match(h)
        assert m, h
        g = slot[m.group(2).decode()]
        cols["genome"].append(g)
        cols["contig"].append(names[g][1].index(m.group(4).decode()))
        cols["start"].append(int(m.group(5)))
        cols["end"].append(int(m.group(6)))
        cols["flags"].append(1 if m.group(7) == b"t" else 0)
        seqs.append(np.frombuffer(s, dtype=np.uint8))
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([s.size for s in seqs], out=off[1:])
    out = {k: np.array(v, dtype=np.uint64 if k in ("start", "end") else np.uint32) for k, v in cols.items()}
    assert np.array_equal(np.abs(out["end"].astype(np.int64) - out["start"].astype(np.int64)), np.diff(off.astype(np.int64)))
    return dict(out, seq=np.concatenate(seqs), seq_off=off)


def test_cli_strain_vcf(workdir):
    d, genomes = workdir
    fq, tsv, vcf = d / "vcf.fq", d / "vcf_sites.tsv", d / "strain.vcf"
    vcf.write_text("an older file\n")
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "6001", "--seed", "42", "--error-profile", "minimal-short", "--with-ani", "97"]
    subprocess.check_call([str(EXE), "--output", str(fq), "--strain-sites", str(tsv), "--strain-vcf", str(vcf), "--device-chunk-reads", "334"] + argv)
    # sequences of at most 450 bases are dropped (main.rs:117-162)
    names, lens = {}, {}
    for gi, (contigs, ids) in enumerate(genomes):
        keep = [i for i, c in enumerate(contigs) if c.size > 450]
        names[gi], lens[gi] = (f"genome{gi}", [ids[i] for i in keep]), [int(contigs[i].size) for i in keep]
    cols = columns_of(fq.read_bytes(), names)
    assert len(cols["start"]) == 6000 and len(cols["start"]) > 2 * 334 * 3  # several ranges
    rows = [r.split("\t") for r in tsv.read_text().splitlines()[1:]]
    slot = {gid: g for g, (gid, _) in names.items()}
    sites = (np.array([slot[r[0]] for r in rows], dtype=np.uint32), np.array([names[slot[r[0]]][1].index(r[1]) for r in rows], dtype=np.uint32),
             np.array([int(r[2]) for r in rows], dtype=np.uint64))
    ref, alt = (np.array([ord(r[k]) for r in rows], dtype=np.uint8) for k in (3, 4))
    assert len(rows) > 5000
    want = _pileup.pileup(cols, sites, lens)
    text = vcf.read_text()
    meta, contigs, records = _pileup.parse_vcf(text)
    assert meta[0] == "fileformat=VCFv4.2" and meta[1] == "source=simmr-hip"
    assert contigs == [(f"{names[g][0]}|{sid}", n) for g in sorted(names) for sid, n in zip(names[g][1], lens[g])]
    assert [m for m in meta if m.startswith("INFO=")] == [x[2:] for x in _pileup.INFO_LINES]
    assert len(records) == len(rows)
    for s, (rec, row) in enumerate(zip(records, rows)):
        k = want[s].astype(np.int64)
        r, a = int(_pileup.CLASS[ref[s]]), int(_pileup.CLASS[alt[s]])
        dp = int(k.sum())
        info = {"DP": dp, "AD": (int(k[:, r].sum()), int(k[:, a].sum())), "ADF": (int(k[0, r]), int(k[0, a])), "ADR": (int(k[1, r]), int(k[1, a])),
                "OTH": dp - int(k[:, r].sum()) - int(k[:, a].sum())}
        assert rec == {"chrom": f"{row[0]}|{row[1]}", "pos": int(row[2]) + 1, "id": ".", "ref": row[3], "alt": row[4], "qual": ".", "filter": ".",
                       "info": info}, (s, rec, info)
    assert text == _pileup.vcf_text(sites, ref, alt, want, names, lens)
    # the reads are the strain's: most covered sites show the alternate, and both strands are there
    assert sum(r["info"]["AD"][1] for r in records) > 10 * sum(r["info"]["AD"][0] for r in records)
    assert sum(r["info"]["ADF"][1] for r in records) > 0 and sum(r["info"]["ADR"][1] for r in records) > 0
    # --strain-vcf alone, in one range: the same file
    alone = d / "alone.vcf"
    subprocess.check_call([str(EXE), "--output", str(d / "vcf2.fq"), "--strain-vcf", str(alone)] + argv)
    assert alone.read_text() == text and (d / "vcf2.fq").read_bytes() == fq.read_bytes()


def test_cli_strain_vcf_refusals(workdir):
    d, _ = workdir
    base = [str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "z.fq"), "--strain-vcf", str(d / "z.vcf")]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 2 and r.stderr.splitlines()[0] == "error: --strain-vcf needs --with-ani"
    r = subprocess.run(base + ["--with-ani", "97", "--devices", "0,0"], capture_output=True, text=True)
    assert r.returncode == 1 and "--strain-vcf does not combine with --devices" in r.stderr
