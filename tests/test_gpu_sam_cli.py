"""`simmr-hip --sam FILE` on the GPU box, on two small FASTA files written here: the SAM file is what the run's own FASTQ, its
truth TSV and the FASTA files say — nothing expected here comes from the SAM pass — and the FASTQ does not change."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _sam, _synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "simmr_amd" / "host" / "simmr-hip"
HEAD = re.compile(rb"^@(\d+)\|([^/]+)/([12]) metadata:sid=(.*)\|sp=(\d+)\|ep=(\d+)\|rc=([tf])$")
COMPLEMENT = bytes.maketrans(b"ACGTN", b"TGCAN")
IDS = [["ctgA first of g0", "ctgB|2 second"], ["plasmid=1.x the only one of g1"]]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "simmr_amd" / "host")])
    d = tmp_path_factory.mktemp("sam_cli")
    genomes = []
    for gi, (lens, seed) in enumerate((([30_011, 25_000], 3), ([41_003], 4))):
        contigs = _synth.synthetic_contigs(lens, seed)
        _synth.write_fasta(d / f"g{gi}.fna", contigs, IDS[gi])
        genomes.append(contigs)
    (d / "genomes.tsv").write_text("path\tid\n" + "".join(f"{d}/g{gi}.fna\tgenome{gi}\n" for gi in range(2)))
    return d, genomes


def fastq_records(fq):
    lines = fq.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    for i in range(0, len(lines) - 1, 4):
        m = HEAD.match(lines[i])
        assert m, lines[i]
        rid, gid, pair, sid, sp, ep, rc = m.groups()
        yield {"id": rid.decode(), "genome": gid.decode(), "sid": sid.decode(), "lo": min(int(sp), int(ep)), "hi": max(int(sp), int(ep)),
               "rev": rc == b"t", "seq": lines[i + 1], "qual": lines[i + 3]}


def check_sam(d, genomes, sam: Path, fq: bytes, truth: Path, paired, sites: Path = None):
    """every check of the file but the byte identity of the FASTQ"""
    text = sam.read_text()
    lines = text.splitlines()
    n_sq = sum(len(g) for g in genomes)
    # ---- the header: @SQ in the order of the FASTA records, RNAME the first word of the id
    want = ["@HD\tVN:1.6\tSO:unsorted"]
    want += [f"@SQ\tSN:{IDS[gi][c].split()[0]}\tLN:{genomes[gi][c].size}" for gi in range(2) for c in range(len(genomes[gi]))]
    want += ["@PG\tID:simmr-hip\tPN:simmr-hip"]
    assert lines[:n_sq + 2] == want and text.endswith("\n")
    # ---- the reference the reads were drawn from: the FASTA, with the strain's sites put in
    ref = {IDS[gi][c].split()[0]: bytearray(genomes[gi][c].tobytes()) for gi in range(2) for c in range(len(genomes[gi]))}
    if sites is not None:
        rows = sites.read_text().splitlines()[1:]
        assert len(rows) > 100
        for row in rows:
            gid, sid, pos, r, a = row.split("\t")
            chrom = ref[sid.split()[0]]
            assert chr(chrom[int(pos)]) == r
            chrom[int(pos)] = ord(a)
    nm_of = [int(row.split("\t")[8]) for row in truth.read_text().splitlines()[1:]]
    recs = [_sam.parse(l) for l in lines[n_sq + 2:]]
    fqs = list(fastq_records(fq))
    assert len(recs) == len(fqs) == len(nm_of) > 0
    n_rev = n_edit = 0
    for r, (f, q) in enumerate(zip(recs, fqs)):
        rev = bool(f["flag"] & 16)
        assert (f["qname"], f["rname"], f["pos"], rev, f["mapq"]) == (q["id"], q["sid"].split()[0], q["lo"] + 1, q["rev"], 255), r
        L = q["hi"] - q["lo"]
        assert f["cigar"] == f"{L}M" and len(f["seq"]) == L == len(f["qual"])
        assert f["seq"].encode() == (q["seq"].translate(COMPLEMENT)[::-1] if rev else q["seq"]), r
        assert f["qual"].encode() == (q["qual"][::-1] if rev else q["qual"]), r
        assert _sam.reference_from(f["seq"], f["md"]).encode() == bytes(ref[f["rname"]][q["lo"]:q["hi"]]), r
        assert f["nm"] == nm_of[r] == sum(c.isalpha() for c in f["md"]), r
        n_rev += rev
        n_edit += f["nm"]
        if paired:
            m, mq = recs[r ^ 1], fqs[r ^ 1]
            assert f["flag"] & 0x3 == 0x3 and bool(f["flag"] & 0x40) == (r % 2 == 0) and bool(f["flag"] & 0x80) == (r % 2 == 1)
            assert bool(f["flag"] & 0x20) == bool(m["flag"] & 0x10)
            assert (f["rnext"], f["pnext"], f["tlen"]) == ("=", m["pos"], -m["tlen"]) and m["rname"] == f["rname"] and m["qname"] == f["qname"]
            assert abs(f["tlen"]) == max(q["hi"], mq["hi"]) - min(q["lo"], mq["lo"])
            assert (f["tlen"] > 0) == (q["lo"] < mq["lo"] or (q["lo"] == mq["lo"] and r % 2 == 0)) or f["tlen"] == 0
        else:
            assert (f["flag"] & ~16, f["rnext"], f["pnext"], f["tlen"]) == (0, "*", 0, 0)
    return n_rev, n_edit, text


def test_short_reads_of_a_strain_and_the_same_run_in_ranges(run):
    d, genomes = run
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "3001", "--seed", "42", "--error-profile", "minimal-short", "--rng", "philox",
            "--with-ani", "99"]
    plain, fq, sam, truth, sites = d / "plain.fq", d / "s.fq", d / "s.sam", d / "s.tsv", d / "sites.tsv"
    subprocess.check_call([str(EXE), "--output", str(plain)] + argv)
    sam.write_text("an older file\n")
    subprocess.check_call([str(EXE), "--output", str(fq), "--sam", str(sam), "--truth", str(truth), "--strain-sites", str(sites)] + argv)
    assert fq.read_bytes() == plain.read_bytes()
    n_rev, n_edit, text = check_sam(d, genomes, sam, fq.read_bytes(), truth, True, sites)
    assert n_rev > 1000 and n_edit > 100
    # several ranges: the header once, the lines in range order — the same file
    fq2, sam2, truth2 = d / "c.fq", d / "c.sam", d / "c.tsv"
    subprocess.check_call([str(EXE), "--output", str(fq2), "--sam", str(sam2), "--truth", str(truth2), "--device-chunk-reads", "334"] + argv)
    assert fq2.read_bytes() == plain.read_bytes() and truth2.read_text() == truth.read_text()
    assert sam2.read_text() == text and text.startswith("@HD\t") and "\n@HD\t" not in text and text.count("\n@PG\t") == 1
    # --sam alone turns the truth pass on
    fq3, sam3 = d / "o.fq", d / "o.sam"
    subprocess.check_call([str(EXE), "--output", str(fq3), "--sam", str(sam3)] + argv)
    assert fq3.read_bytes() == plain.read_bytes() and sam3.read_text() == text and not (d / "o.tsv").exists()


def test_long_reads(run):
    d, genomes = run
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "41", "--seed", "11", "--error-profile", "minimal-long", "--rng", "philox",
            "--gamma", "3000,2500", "--per-read-lengths"]
    plain, fq, sam, truth = d / "lplain.fq", d / "l.fq", d / "l.sam", d / "l.tsv"
    subprocess.check_call([str(EXE), "--output", str(plain)] + argv)
    subprocess.check_call([str(EXE), "--output", str(fq), "--sam", str(sam), "--truth", str(truth), "--device-chunk-reads", "7"] + argv)
    assert fq.read_bytes() == plain.read_bytes()
    n_rev, n_edit, text = check_sam(d, genomes, sam, fq.read_bytes(), truth, False)
    assert n_edit > 100 and max(len(l) for l in text.splitlines()) > 8000


def test_sam_refuses_devices(run):
    d, _ = run
    r = subprocess.run([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "x.fq"), "--sam", str(d / "x.sam"),
                        "--devices", "0,0"], capture_output=True)
    assert r.returncode == 1 and b"--sam does not combine with --devices: use --device" in r.stderr
