"""`simmr-hip --gold-assembly FILE --gold-regions FILE` on the GPU box: the regions add up to what `--depth` reports as
covered, the FASTA parses back to slices of the input genomes, the TSV says what the FASTA's header lines say
(its header line is tests/_regions.py's), and with --with-ani the bases differ from the input at exactly the sites --strain-sites lists."""
import re
import subprocess

import numpy as np
import pytest

from tests import _regions
from tests.test_gpu_cli import EXE, workdir  # noqa: F401  (the two-genome FASTA fixture)

pytestmark = pytest.mark.gpu
HEADER = re.compile(rb"^>([^|]+)\|(.*):(\d+)-(\d+) depth_sum=(\d+)$")


def parse_fasta(text):
    """[(genome id, sequence id, start 0-based, end, depth_sum, bases)]; every line but a record's last holds 80 bases"""
    out = []
    for rec in text.split(b">")[1:]:
        lines = rec.split(b"\n")
        m = HEADER.match(b">" + lines[0])
        assert m and lines[-1] == b"", lines[0]
        body = lines[1:-1]
        assert all(len(x) == 80 for x in body[:-1]) and 0 < len(body[-1]) <= 80
        out.append((m.group(1).decode(), m.group(2).decode(), int(m.group(3)) - 1, int(m.group(4)), int(m.group(5)), b"".join(body)))
    return out


def test_cli_gold_assembly(workdir):
    d, genomes = workdir
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "3001", "--seed", "42", "--error-profile", "minimal-short"]
    source = {(f"genome{gi}", sid): c.tobytes() for gi, (contigs, ids) in enumerate(genomes) for sid, c in zip(ids, contigs)}
    plain, gold = d / "plain_g.fq", d / "gold.fq"
    subprocess.check_call([str(EXE), "--output", str(plain)] + argv)
    subprocess.check_call([str(EXE), "--output", str(gold), "--gold-assembly", str(d / "ga.fa"), "--gold-regions", str(d / "gr.tsv"),
                           "--depth", str(d / "gd.tsv")] + argv)
    assert gold.read_bytes() == plain.read_bytes()
    recs = parse_fasta((d / "ga.fa").read_bytes())
    rows = [x.split("\t") for x in (d / "gr.tsv").read_text().splitlines()]
    assert "\t".join(rows[0]) + "\n" == _regions.TSV_HEADER and len(rows) - 1 == len(recs) > 100
    # the FASTA is slices of the input genomes, and says what the TSV says
    at = 0
    for (gid, sid, a, b, dsum, bases), row in zip(recs, rows[1:]):
        assert bases == source[(gid, sid)][a:b] and row == [gid, sid, str(a), str(b - a), str(dsum), str(at)], (gid, sid, a, b)
        at += b - a
    # per contig: the regions at the default --gold-min-depth 1 are the covered positions of --depth
    depth_rows = [x.split("\t") for x in (d / "gd.tsv").read_text().splitlines()[1:]]
    assert len(depth_rows) == 3
    for gid, sid, length, covered, depth_sum, _ in depth_rows:
        mine = [(b - a, s) for g, q, a, b, s, _ in recs if (g, q) == (gid, sid)]
        assert sum(x for x, _ in mine) == int(covered) < int(length) and sum(s for _, s in mine) == int(depth_sum), (gid, sid)
    # regions in the order of depth[], disjoint and not touching inside a sequence
    for (g0, q0, _, b0, _, _), (g1, q1, a1, _, _, _) in zip(recs, recs[1:]):
        assert (g0, q0) != (g1, q1) or a1 > b0
    # thresholds: deeper and longer regions only (one region of the default run may hold several of them), each inside a
    # region of the default run, fewer bases in all
    subprocess.check_call([str(EXE), "--output", str(d / "gold2.fq"), "--gold-assembly", str(d / "ga2.fa"), "--gold-min-depth", "2",
                           "--gold-min-length", "50", "--device-chunk-reads", "334"] + argv)
    deep = parse_fasta((d / "ga2.fa").read_bytes())
    assert 0 < sum(b - a for _, _, a, b, _, _ in deep) < sum(b - a for _, _, a, b, _, _ in recs) and all(b - a >= 50 and s >= 2 * (b - a) and bases == source[(g, q)][a:b] for g, q, a, b, s, bases in deep)
    assert all(any((g, q) == (g1, q1) and a1 <= a and b <= b1 for g1, q1, a1, b1, _, _ in recs) for g, q, a, b, _, _ in deep)


def test_cli_gold_assembly_of_a_strain(workdir):
    d, genomes = workdir
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "3001", "--seed", "42", "--error-profile", "minimal-short"]
    source = {(f"genome{gi}", sid): np.frombuffer(c.tobytes(), dtype=np.uint8) for gi, (contigs, ids) in enumerate(genomes) for sid, c in zip(ids, contigs)}
    subprocess.check_call([str(EXE), "--output", str(d / "gold_ani.fq"), "--with-ani", "95", "--strain-sites", str(d / "g_sites.tsv"),
                           "--gold-assembly", str(d / "ga_ani.fa")] + argv)
    sites = {}
    for line in (d / "g_sites.tsv").read_text().splitlines()[1:]:
        gid, sid, pos, ref, alt = line.split("\t")
        sites.setdefault((gid, sid), {})[int(pos)] = (ref, alt)
    recs = parse_fasta((d / "ga_ani.fa").read_bytes())
    n_diff = 0
    for gid, sid, a, b, _, bases in recs:
        got, ref = np.frombuffer(bases, dtype=np.uint8), source[(gid, sid)][a:b]
        diff = set((np.flatnonzero(got != ref) + a).tolist())
        listed = {p for p in sites.get((gid, sid), {}) if a <= p < b}
        assert diff == listed, (gid, sid, a, b, sorted(diff ^ listed)[:8])
        assert all(chr(got[p - a]) == sites[(gid, sid)][p][1] and chr(ref[p - a]) == sites[(gid, sid)][p][0] for p in diff)
        n_diff += len(diff)
    assert len(recs) > 100 and n_diff > 1000


def test_cli_gold_refuses_devices(workdir):
    d, _ = workdir
    r = subprocess.run([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "zg.fq"), "--gold-assembly", str(d / "zg.fa"),
                        "--devices", "0,0"], capture_output=True)
    assert r.returncode == 1 and b"--gold-assembly does not combine with --devices" in r.stderr
