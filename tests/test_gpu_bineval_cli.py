"""simmr-hip end to end: a run with --gold-assembly, --eval-assembly with the gold FASTA itself as contigs and --eval-assembly-contigs,
then --eval-bins on a bins file written here: a bin per genome with two contigs swapped, one left out, one unknown and one repeated.
The report's numbers follow from that construction; the two side files are the plain model's rows; the usage errors."""
import subprocess
from pathlib import Path

import pytest

from tests import _bineval
from tests._synth import synthetic_contigs, write_fasta

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "simmr_amd" / "host" / "simmr-hip"


def test_bins_of_the_gold_assembly_end_to_end(tmp_path):
    refs = []
    for i, seed in enumerate((11, 12)):
        path = tmp_path / f"g{i}.fna"
        write_fasta(path, synthetic_contigs([6000, 3000, 2000, 1500], seed), names=[f"g{i}_c{j}" for j in range(4)])
        refs.append(path)
    gold, truth = tmp_path / "gold.fa", tmp_path / "contigs.tsv"
    subprocess.run([str(EXE), "--genome", str(refs[0]), "--genome", str(refs[1]), "--num-reads", "3000", "--seed", "42", "--error-profile", "minimal-short",
                    "--output", str(tmp_path / "reads.fq"), "--gold-assembly", str(gold)], check=True, capture_output=True, timeout=120)
    subprocess.run([str(EXE), "--eval-assembly", str(gold), "--eval-assembly-truth", str(gold), "--eval-assembly-report", str(tmp_path / "asm.tsv"),
                    "--eval-assembly-contigs", str(truth)], check=True, capture_output=True, timeout=120)
    t = truth.read_bytes()
    rows = [ln.split(b"\t") for ln in t.split(b"\n") if ln]
    by_genome = {}
    for r in rows:
        assert len(r) == 8 and r[7] != b".", r   # the gold assembly scored against itself: every contig has its genome
        by_genome.setdefault(r[7], []).append((r[0], int(r[1])))
    genomes = sorted(by_genome)
    assert len(genomes) == 2 and all(len(v) >= 3 for v in by_genome.values()), "the construction below needs three contigs a genome"
    a, b = (by_genome[g] for g in genomes)
    # a bin per genome; a[0] and b[0] swapped, a[1] left out, one unknown contig, b[1] repeated (its first record wins)
    recs = [(n, b"bin_" + genomes[0]) for n, _ in a[2:]] + [(b[0][0], b"bin_" + genomes[0])]
    recs += [(n, b"bin_" + genomes[1]) for n, _ in b[1:]] + [(a[0][0], b"bin_" + genomes[1]), (b"no_such_contig", b"bin_x"), (b[1][0], b"bin_" + genomes[0])]
    bins = tmp_path / "bins.tsv"
    bins.write_bytes(b"@Version:0.9.0\n@@SEQUENCEID\tBINID\n" + _bineval.bins_text(recs))
    report, cells, contigs = tmp_path / "bins_report.tsv", tmp_path / "cells.tsv", tmp_path / "bin_contigs.tsv"
    subprocess.run([str(EXE), "--eval-bins", str(bins), "--eval-bins-truth", str(truth), "--eval-bins-report", str(report), "--eval-bins-bins", str(cells),
                    "--eval-bins-contigs", str(contigs)], check=True, capture_output=True, timeout=120)
    text = report.read_text()
    head = dict(ln[1:].split("\t", 1) for ln in text.split("\n") if ln.startswith("#") and not ln.startswith(("#G\t", "#B\t")))
    la, lb = sum(x for _, x in a), sum(x for _, x in b)
    in_a, in_b = la - a[0][1] - a[1][1], lb - b[0][1]   # what bin a holds of genome a, bin b of genome b
    assert int(head["truth_records"]) == len(rows) and int(head["truth_bases"]) == la + lb and int(head["truth_none"]) == 0
    assert int(head["records"]) == len(recs) and int(head["unknown_contig"]) == 1 and int(head["repeated"]) == 1
    assert int(head["assigned"]) == len(rows) - 1 and int(head["assigned_bases"]) == la + lb - a[1][1]
    assert int(head["bins"]) == 2 and int(head["cells"]) == 4
    top_a, top_b = max(in_a, b[0][1]), max(in_b, a[0][1])
    assert int(head["sum_top_bases"]) == top_a + top_b
    assert head["purity"] == "%d/%d\t%.6f" % (top_a + top_b, la + lb - a[1][1], (top_a + top_b) / (la + lb - a[1][1]))
    assert int(head["sum_best_bases"]) == max(in_a, a[0][1]) + max(in_b, b[0][1])
    assert head["completeness"].startswith("%d/%d\t" % (max(in_a, a[0][1]) + max(in_b, b[0][1]), la + lb))
    pairs = lambda n: n * (n - 1) // 2
    assert int(head["pairs_cells"]) == pairs(len(a) - 2) + pairs(len(b) - 1) and int(head["pairs_bins"]) == pairs(len(a) - 1) + pairs(len(b))
    assert int(head["pairs_genomes"]) == pairs(len(a) - 1) + pairs(len(b))
    assert [ln.split("\t")[1] for ln in text.split("\n") if ln.startswith("B\t")] == ["bin_" + genomes[0].decode(), "bin_" + genomes[1].decode()]
    # the side files against the model's rows
    m = _bineval.evaluate([t], [bins.read_bytes()], genomes)
    names = [g.decode() for g in m.names]
    bn = [x.decode() for x in m.bin_names]
    want_cells = "".join("%s\t%s\t%d\t%d\n" % (bn[b_], names[g] if g < len(names) else ".", c, s) for b_, g, c, s in zip(*m.cells()))
    assert cells.read_text() == want_cells
    want_contigs = "".join("%s\t%d\t%s\t%s\t%d\n" % (r[0].decode(), l, names[g] if g < len(names) else ".", bn[b_] if b_ < len(bn) else ".", k)
                           for r, g, l, b_, k in zip(rows, *m.contigs()))
    assert contigs.read_text() == want_contigs
    counts = m.read()[0]
    assert all(int(head[k]) == v for k, v in counts.items())


def test_usage_errors_and_a_missing_file(tmp_path):
    r = subprocess.run([str(EXE), "--eval-bins", "b.tsv", "--eval-bins-report", "r.tsv"], capture_output=True, text=True, cwd=tmp_path)
    assert (r.returncode, r.stderr.split("\n")[0]) == (2, "error: --eval-bins needs --eval-bins-truth")
    r = subprocess.run([str(EXE), "--eval-bins", "b.tsv", "--eval-bins-truth", "t.tsv", "--eval-bins-report", "r.tsv", "--devices", "0"], capture_output=True,
                       text=True, cwd=tmp_path)
    assert r.returncode == 2 and "('--devices' given)" in r.stderr.split("\n")[0]
    r = subprocess.run([str(EXE), "--eval-bins", "b.tsv", "--eval-bins-truth", "t.tsv", "--eval-bins-report", "r.tsv"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "--eval-bins: cannot open b.tsv" in r.stderr and not list(tmp_path.iterdir())
    (tmp_path / "b.tsv").write_bytes(b"c1\tbin\n")
    (tmp_path / "t.tsv").write_bytes(b"c1\t5\t1\t1\t1\t1\t1\tgA\nc1\t5\t1\t1\t1\t1\t1\tgA\n")
    r = subprocess.run([str(EXE), "--eval-bins", "b.tsv", "--eval-bins-truth", "t.tsv", "--eval-bins-report", "r.tsv"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "a contig name occurs twice" in r.stderr and not (tmp_path / "r.tsv").exists()
