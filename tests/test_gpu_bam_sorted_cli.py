"""`simmr-hip --bam FILE --bam-sorted` on the GPU box: the file holds the records of the read-order --bam file of the same run,
stably sorted by (refID, pos) under a header that says SO:coordinate; the index beside it is the plain-Python index of
tests/_bai.py, byte for byte, and answers region queries as reading every record does — over several ranges (merged through
the temporary file), in one range, and for long reads."""
import gzip
import struct
import subprocess
from pathlib import Path

import pytest

from tests import _bai, _bam, _synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "simmr_amd" / "host" / "simmr-hip"
IDS = [["ctgA first of g0", "ctgB|2 second"], ["plasmid=1.x the only one of g1"]]
LENS = [[30_011, 25_000], [41_003]]
REFS = [(i.split()[0], n) for ids, lens in zip(IDS, LENS) for i, n in zip(ids, lens)]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "simmr_amd" / "host")])
    d = tmp_path_factory.mktemp("bam_sorted_cli")
    for gi, (lens, seed) in enumerate(zip(LENS, (3, 4))):
        _synth.write_fasta(d / f"g{gi}.fna", _synth.synthetic_contigs(lens, seed), IDS[gi])
    (d / "genomes.tsv").write_text("path\tid\n" + "".join(f"{d}/g{gi}.fna\tgenome{gi}\n" for gi in range(2)))
    return d


def raw_records(stream):
    """(the header's bytes, every record's bytes) of an uncompressed BAM stream"""
    _, refs, _ = _bam.parse_bam(stream)
    (l_text,) = struct.unpack_from("<i", stream, 4)
    at = 12 + l_text + sum(8 + len(n) + 1 for n, _ in refs)
    base, recs = at, []
    while at < len(stream):
        (size,) = struct.unpack_from("<i", stream, at)
        recs.append(stream[at:at + 4 + size])
        at += 4 + size
    return base, recs


def compare(d, unsorted, ordered, index):
    """the sorted file against the read-order file of the same run, and the index against the model and against brute force"""
    file_bytes = ordered.read_bytes()
    assert file_bytes.endswith(_bam.BGZF_EOF)
    _bam.bgzf_blocks(file_bytes[:-len(_bam.BGZF_EOF)])  # (one stream: every block but the last is full)
    su, ss = gzip.decompress(unsorted.read_bytes()), gzip.decompress(file_bytes)
    text_u, refs_u, _ = _bam.parse_bam(su)
    text_s, refs_s, _ = _bam.parse_bam(ss)
    assert text_u.splitlines()[0] == "@HD\tVN:1.6\tSO:unsorted" and text_s.splitlines()[0] == "@HD\tVN:1.6\tSO:coordinate"
    assert text_u.splitlines()[1:] == text_s.splitlines()[1:] and refs_u == refs_s == REFS
    _, recs_u = raw_records(su)
    base, recs_s = raw_records(ss)
    want = sorted(recs_u, key=lambda r: struct.unpack_from("<ii", r, 4))  # (stable)
    assert recs_s == want and recs_s != recs_u
    bai = index.read_bytes()
    assert bai == _bai.bai_bytes(len(REFS), b"".join(recs_s), base)
    parsed, stream = _bai.parse_bai(bai), _bai.Stream(file_bytes)
    found = 0
    for ref, (_, length) in enumerate(REFS):
        for beg in list(range(0, length, 1 << 14)) + [length - 1]:
            for b, e in ((max(beg - 1, 0), beg + 1), (beg, beg + 1), (beg, min(beg + (1 << 14), length)), (0, length)):
                got = _bai.query(parsed, stream, ref, b, e)
                assert got == _bai.brute(stream, base, ref, b, e), (ref, b, e)
                found += len(got)
    assert found >= len(recs_s)  # (the whole-reference queries alone return every record)
    assert sorted(p.name for p in d.iterdir() if "tmp" in p.name) == []
    return len(recs_s)


def test_short_pairs_of_a_strain_in_ranges_and_in_one(run):
    d = run
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "3001", "--seed", "42", "--error-profile", "minimal-short", "--rng", "philox",
            "--with-ani", "99"]
    u, s, one = d / "u.bam", d / "s.bam", d / "one.bam"
    subprocess.check_call([str(EXE), "--output", str(d / "u.fq"), "--bam", str(u), "--device-chunk-reads", "334"] + argv)
    s.write_text("an older file\n")
    (d / "s.bam.bai").write_text("an older index\n")
    r = subprocess.run([str(EXE), "--output", str(d / "s.fq"), "--bam", str(s), "--bam-sorted", "--device-chunk-reads", "334"] + argv, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (d / "s.fq").read_bytes() == (d / "u.fq").read_bytes()
    assert compare(d, u, s, d / "s.bam.bai") == 3000 and 3000 // 334 >= 3
    subprocess.check_call([str(EXE), "--output", str(d / "one.fq"), "--bam", str(one), "--bam-sorted", "--bam-index", str(d / "elsewhere.idx")] + argv)
    assert one.read_bytes() == s.read_bytes() and (d / "elsewhere.idx").read_bytes() == (d / "s.bam.bai").read_bytes()
    assert not (d / "one.bam.bai").exists()


def test_long_reads(run):
    d = run
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "41", "--seed", "11", "--error-profile", "minimal-long", "--rng", "philox",
            "--gamma", "3000,2500", "--per-read-lengths"]
    u, s, one = d / "lu.bam", d / "ls.bam", d / "lone.bam"
    subprocess.check_call([str(EXE), "--output", str(d / "lu.fq"), "--bam", str(u), "--device-chunk-reads", "7"] + argv)
    subprocess.check_call([str(EXE), "--output", str(d / "ls.fq"), "--bam", str(s), "--bam-sorted", "--device-chunk-reads", "7"] + argv)
    assert (d / "ls.fq").read_bytes() == (d / "lu.fq").read_bytes()
    n = compare(d, u, s, d / "ls.bam.bai")  # (as many records as the read-order file: every genome's share of the 41 is rounded up)
    assert 41 <= n <= 43 and n // 7 >= 3
    subprocess.check_call([str(EXE), "--output", str(d / "lone.fq"), "--bam", str(one), "--bam-sorted"] + argv)
    assert one.read_bytes() == s.read_bytes() and (d / "lone.bam.bai").read_bytes() == (d / "ls.bam.bai").read_bytes()
