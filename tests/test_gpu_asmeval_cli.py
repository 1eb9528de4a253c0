"""simmr-hip --gold-assembly, then --eval-assembly on what it wrote: the truth scored against itself is complete, without a novel
k-mer and every contig pure; a perturbed copy is scored and the report and the contig file are the plain model's, line by line."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _asmeval
from tests._asmeval import fasta
from tests._synth import synthetic_contigs, write_fasta

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "simmr_amd" / "host" / "simmr-hip"


def score(tmp_path, contigs: Path, gold: Path, tag: str, k=31):
    report, rows = tmp_path / f"{tag}.tsv", tmp_path / f"{tag}_contigs.tsv"
    subprocess.run([str(EXE), "--eval-assembly", str(contigs), "--eval-assembly-truth", str(gold), "--eval-assembly-report", str(report),
                    "--eval-assembly-contigs", str(rows), "--eval-assembly-k", str(k)], check=True, capture_output=True, timeout=120)
    return report.read_text(), rows.read_text()


def model_files(gold: bytes, contigs: bytes, k=31):
    words, _ = _asmeval.fasta_records(gold)
    genomes = sorted({w.split("|")[0] for w in words})
    m = _asmeval.evaluate([gold], [contigs], genomes, k)
    counts, by = m.read()
    names, _ = _asmeval.fasta_records(contigs)
    return (_asmeval.report_text(counts, by, genomes, k, m.truth_lengths, m.contigs()[0]), _asmeval.contig_rows(names, genomes, m.contigs()), counts, by)


def test_the_gold_assembly_scored_against_itself_and_a_perturbed_copy(tmp_path):
    refs = []
    for i, seed in enumerate((11, 12)):
        path = tmp_path / f"g{i}.fna"
        write_fasta(path, synthetic_contigs([6000, 3000], seed), names=[f"g{i}_c0", f"g{i}_c1"])
        refs.append(path)
    gold = tmp_path / "gold.fa"
    subprocess.run([str(EXE), "--genome", str(refs[0]), "--genome", str(refs[1]), "--num-reads", "3000", "--seed", "42", "--error-profile", "minimal-short", "--output", str(tmp_path / "reads.fq"),
                    "--gold-assembly", str(gold)], check=True, capture_output=True, timeout=120)
    text = gold.read_bytes()
    assert text.count(b">") >= 2
    report, rows = score(tmp_path, gold, gold, "self")
    want_report, want_rows, counts, by = model_files(text, text)
    assert report == want_report and rows == want_rows
    assert counts["novel"] == 0 and counts["contigs_pure"] + counts["contigs_short"] == counts["records"] and counts["contigs_pure"] > 0
    assert np.array_equal(by[:, 0], by[:, 1]) and "#qv\tinf\n" in report   # every genome's completeness is exactly 1
    assert all(line.endswith("\t1.000000") for line in report.split("\n") if line.startswith("G\t") and "\t0\t0\t0\t0\t0\t" not in line)
    # a perturbed copy: a substitution in every record, the first two records joined, one dropped, one foreign
    recs = _asmeval.records(text)
    out = []
    for i, (h, s) in enumerate(recs):
        b = bytearray(s)
        if len(b) > 40:
            b[len(b) // 2] = ord("A") if b[len(b) // 2] != ord("A") else ord("C")
        out.append((b"contig_%d" % i, bytes(b)))
    out = [(b"joined", out[0][1] + out[-1][1])] + out[2:] + [(b"foreign", synthetic_contigs([900], 99)[0].tobytes())]
    pert = tmp_path / "assembly.fa"
    pert.write_bytes(fasta(out, width=70))
    report, rows = score(tmp_path, pert, gold, "pert", k=21)
    want_report, want_rows, counts, by = model_files(text, pert.read_bytes(), k=21)
    assert report.split("\n") == want_report.split("\n")
    assert rows.split("\n") == want_rows.split("\n")
    assert counts["novel"] > 0 and counts["contigs_novel"] == 1
