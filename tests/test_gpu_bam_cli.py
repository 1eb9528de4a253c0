"""`simmr-hip --bam FILE` on the GPU box: the file, read by the standard library's gzip and tests/_bam.py's reader, holds the
header and, record by record in order, the lines of the --sam file of the same run — over several ranges of short pairs, and for
long reads under a header format of the user's."""
import gzip
import shutil
import subprocess
from pathlib import Path

import pytest

from simmr_amd.sam import BGZF_EOF
from tests import _bam, _synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "simmr_amd" / "host" / "simmr-hip"
IDS = [["ctgA first of g0", "ctgB|2 second"], ["plasmid=1.x the only one of g1"]]
LENS = [[30_011, 25_000], [41_003]]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "simmr_amd" / "host")])
    d = tmp_path_factory.mktemp("bam_cli")
    for gi, seed in enumerate((3, 4)):
        _synth.write_fasta(d / f"g{gi}.fna", _synth.synthetic_contigs(LENS[gi], seed), IDS[gi])
    (d / "genomes.tsv").write_text("path\tid\n" + "".join(f"{d}/g{gi}.fna\tgenome{gi}\n" for gi in range(2)))
    return d


def compare(sam, bam, n_records):
    raw = bam.read_bytes()
    assert raw.endswith(BGZF_EOF) and not raw[:-len(BGZF_EOF)].endswith(BGZF_EOF)
    blocks = _bam.bgzf_blocks(raw[:-len(BGZF_EOF)], one_call=False)
    assert gzip.decompress(raw) == b"".join(blocks)
    text, refs, recs = _bam.parse_bam(b"".join(blocks))
    lines = sam.read_text().splitlines(keepends=True)
    head = [l for l in lines if l.startswith("@")]
    assert text == "".join(head) and head[0] == "@HD\tVN:1.6\tSO:unsorted\n"
    assert [f"@SQ\tSN:{name}\tLN:{length}\n" for name, length in refs] == [l for l in head if l.startswith("@SQ")]
    assert refs == [(i.split()[0], n) for ids, lens in zip(IDS, LENS) for i, n in zip(ids, lens)]
    assert (n_records is None or len(recs) == n_records) and [_bam.to_sam_line(r, refs) for r in recs] == lines[len(head):]
    if shutil.which("samtools"):
        subprocess.check_call(["samtools", "quickcheck", str(bam)])
        assert subprocess.check_output(["samtools", "view", "-h", "--no-PG", str(bam)]).decode() == sam.read_text()
    return blocks


def test_short_pairs_in_ranges(run):
    d = run
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "3001", "--seed", "42", "--error-profile", "minimal-short", "--rng", "philox",
            "--device-chunk-reads", "334"]
    sam, bam = d / "a.sam", d / "b.bam"
    bam.write_text("an older file\n")
    r = subprocess.run([str(EXE), "--output", str(d / "ab.fq"), "--sam", str(sam), "--bam", str(bam)] + argv, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blocks = compare(sam, bam, 3000)
    assert 3000 // 334 >= 3 and len(blocks) >= 1 + 3  # the header's block, and at least one per range
    # --bam alone gives the same file, and the FASTQ of the run does not change
    alone = d / "alone.bam"
    subprocess.check_call([str(EXE), "--output", str(d / "alone.fq"), "--bam", str(alone)] + argv)
    assert alone.read_bytes() == bam.read_bytes() and (d / "alone.fq").read_bytes() == (d / "ab.fq").read_bytes()


def test_long_reads_under_a_header_format(run):
    d = run
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "41", "--seed", "11", "--error-profile", "minimal-long", "--rng", "philox",
            "--gamma", "3000,2500", "--per-read-lengths", "--device-chunk-reads", "7", "--read-header-format", "@{:read_id:}/{:pair:} {:genome_id:}"]
    sam, bam = d / "l.sam", d / "l.bam"
    subprocess.check_call([str(EXE), "--output", str(d / "l.fq"), "--sam", str(sam), "--bam", str(bam)] + argv)
    compare(sam, bam, None)  # (the abundance profile rounds 41 up per genome)
    assert len(sam.read_text().splitlines()) >= 41 + 5


def test_bam_with_devices_is_refused_before_any_work(run):
    d = run
    r = subprocess.run([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "x.fq"), "--bam", str(d / "x.bam"), "--devices", "0"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.splitlines()[0] == "ERROR simmr-hip: --bam does not combine with --devices: use --device"
    assert not (d / "x.bam").exists() and not (d / "x.fq").exists()
