"""`simmr-hip --overlaps FILE` on the GPU box: the PAF of a run cut into several ranges is that of the run in one range, and both
are the model of tests/_overlap.py applied to the run's --sam file (QNAME, FLAG, RNAME, POS and the length)."""
import subprocess
from pathlib import Path

import pytest

from tests import _overlap, _synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "simmr_amd" / "host" / "simmr-hip"
IDS = [["ctgA first of g0", "ctgB|2 second"], ["plasmid=1.x the only one of g1"]]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "simmr_amd" / "host")])
    d = tmp_path_factory.mktemp("overlap_cli")
    for gi, (lens, seed) in enumerate((([30_011, 25_000], 3), ([41_003], 4))):
        _synth.write_fasta(d / f"g{gi}.fna", _synth.synthetic_contigs(lens, seed), IDS[gi])
    (d / "genomes.tsv").write_text("path\tid\n" + "".join(f"{d}/g{gi}.fna\tgenome{gi}\n" for gi in range(2)))
    return d


def reads_of_sam(path):
    """the model's reads, in file order, from an unsorted SAM file: the row is the index of RNAME among the @SQ lines"""
    sq, reads = [], []
    for line in path.read_text().split("\n"):
        f = line.split("\t")
        if line.startswith("@SQ"):
            sq.append(f[1][3:])
        elif line and not line.startswith("@"):
            flag, lo, L = int(f[1]), int(f[3]) - 1, 0 if f[9] == "*" else len(f[9])
            assert f[5] == ("*" if L == 0 else f"{L}M")
            reads.append((sq.index(f[2]), lo, lo + L, (flag >> 4) & 1, int(f[0]), (2 if flag & 0x80 else 1) if flag & 1 else 0))
    return reads


def ranges_against_one(d, tag, argv, chunk, min_overlap):
    cut, one, sam = d / f"{tag}_cut.paf", d / f"{tag}_one.paf", d / f"{tag}.sam"
    cut.write_text("an older file\n")
    extra = ["--min-overlap", str(min_overlap)] if min_overlap != 1 else []
    r = subprocess.run([str(EXE), "--output", str(d / f"{tag}_cut.fq"), "--overlaps", str(cut), "--sam", str(sam), "--device-chunk-reads", str(chunk)] + extra + argv,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    subprocess.check_call([str(EXE), "--output", str(d / f"{tag}_one.fq"), "--overlaps", str(one)] + extra + argv)
    assert cut.read_bytes() == one.read_bytes()
    reads = reads_of_sam(sam)
    want, ps = _overlap.paf(reads, min_overlap)
    assert len(ps) > 100 and cut.read_bytes() == want
    return reads


def test_long_reads_in_ranges_and_in_one(run):
    argv = ["--genome-file", str(run / "genomes.tsv"), "--num-reads", "300", "--seed", "11", "--error-profile", "minimal-long", "--rng", "philox",
            "--gamma", "3000,2500", "--per-read-lengths"]
    reads = ranges_against_one(run, "long", argv, 70, 500)
    assert len(reads) == 300 and 300 // 70 >= 3


def test_short_pairs_in_ranges_and_in_one(run):
    argv = ["--genome-file", str(run / "genomes.tsv"), "--num-reads", "1200", "--seed", "42", "--error-profile", "minimal-short", "--rng", "philox"]
    reads = ranges_against_one(run, "pe", argv, 334, 1)
    assert len(reads) == 1200 and {r[5] for r in reads} == {1, 2}


def test_overlaps_with_devices_is_refused(run):
    d = run
    r = subprocess.run([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "x.fq"), "--overlaps", str(d / "x.paf"), "--devices", "0"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--overlaps does not combine with --devices: use --device" in r.stderr
    assert not (d / "x.paf").exists() and not (d / "x.fq").exists()
