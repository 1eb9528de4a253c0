"""`simmr-hip --sam FILE --sam-sorted` on the GPU box: the file is the unsorted --sam file of the same run, stable-sorted in
Python by (@SQ index, POS) under a header that differs in SO: alone — over several ranges (merged through the temporary file),
in one range, for a strain, and for long reads."""
import subprocess
from pathlib import Path

import pytest

from tests import _sam_sort, _synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "simmr_amd" / "host" / "simmr-hip"
IDS = [["ctgA first of g0", "ctgB|2 second"], ["plasmid=1.x the only one of g1"]]
SQ = [i.split()[0] for ids in IDS for i in ids]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "simmr_amd" / "host")])
    d = tmp_path_factory.mktemp("sam_sort_cli")
    for gi, (lens, seed) in enumerate((([30_011, 25_000], 3), ([41_003], 4))):
        _synth.write_fasta(d / f"g{gi}.fna", _synth.synthetic_contigs(lens, seed), IDS[gi])
    (d / "genomes.tsv").write_text("path\tid\n" + "".join(f"{d}/g{gi}.fna\tgenome{gi}\n" for gi in range(2)))
    return d


def split(path):
    lines = path.read_bytes().split(b"\n")
    n = next(i for i, l in enumerate(lines) if not l.startswith(b"@"))
    return lines[:n], b"\n".join(lines[n:])


def compare(d, unsorted, ordered):
    head_u, body_u = split(unsorted)
    head_s, body_s = split(ordered)
    assert head_u[0] == b"@HD\tVN:1.6\tSO:unsorted" and head_s[0] == b"@HD\tVN:1.6\tSO:coordinate" and head_u[1:] == head_s[1:]
    assert body_s == _sam_sort.stable_sort_of_text(body_u, SQ) and body_s != body_u
    assert sorted(p.name for p in d.iterdir() if "tmp" in p.name) == []


def test_short_pairs_of_a_strain_in_ranges_and_in_one(run):
    d = run
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "3001", "--seed", "42", "--error-profile", "minimal-short", "--rng", "philox",
            "--with-ani", "99"]
    u, s, one = d / "u.sam", d / "s.sam", d / "one.sam"
    subprocess.check_call([str(EXE), "--output", str(d / "u.fq"), "--sam", str(u), "--device-chunk-reads", "334"] + argv)
    s.write_text("an older file\n")
    r = subprocess.run([str(EXE), "--output", str(d / "s.fq"), "--sam", str(s), "--sam-sorted", "--device-chunk-reads", "334"] + argv, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (d / "s.fq").read_bytes() == (d / "u.fq").read_bytes()
    assert body_lines(s) == 3000 and 3000 // 334 >= 3
    compare(d, u, s)
    subprocess.check_call([str(EXE), "--output", str(d / "one.fq"), "--sam", str(one), "--sam-sorted"] + argv)
    assert one.read_bytes() == s.read_bytes()


def body_lines(path):
    return sum(1 for l in path.read_bytes().split(b"\n") if l and not l.startswith(b"@"))


def test_long_reads(run):
    d = run
    argv = ["--genome-file", str(d / "genomes.tsv"), "--num-reads", "41", "--seed", "11", "--error-profile", "minimal-long", "--rng", "philox",
            "--gamma", "3000,2500", "--per-read-lengths", "--device-chunk-reads", "7"]
    u, s = d / "lu.sam", d / "ls.sam"
    subprocess.check_call([str(EXE), "--output", str(d / "lu.fq"), "--sam", str(u)] + argv)
    subprocess.check_call([str(EXE), "--output", str(d / "ls.fq"), "--sam", str(s), "--sam-sorted"] + argv)
    compare(d, u, s)


def test_sorted_with_devices_is_refused_before_any_work(run):
    """a usage error: no file of the run, and no temporary file, is made"""
    d = run
    r = subprocess.run([str(EXE), "--genome-file", str(d / "genomes.tsv"), "--output", str(d / "x.fq"), "--sam", str(d / "x.sam"), "--sam-sorted",
                        "--devices", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and r.stderr.splitlines()[0] == "error: --sam-sorted does not combine with --devices: use --device"
    assert not (d / "x.sam").exists() and not (d / "x.fq").exists() and not (d / "x.sam.sorting.tmp").exists()
