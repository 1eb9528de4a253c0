"""simmr-hip --eval-placement on a small pair of files: the report, the block file and the contig file are byte-equal to the plain
model's text (tests/_asmmap.py)."""
import subprocess
from pathlib import Path

import pytest

from tests import _asmmap
from tests._asmmap import fasta
from tests.test_gpu_asmmap import community

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "simmr_amd" / "host" / "simmr-hip"


@pytest.mark.parametrize("params", [dict(k=31, band=64, relocation=1000, min_anchors=16), dict(k=21, band=16, relocation=200, min_anchors=4)], ids=["defaults", "k21"])
def test_the_three_files_are_the_models_text(tmp_path, params):
    truth, contigs = community()
    gold, asm = tmp_path / "gold.fa", tmp_path / "assembly.fa"
    gold.write_bytes(fasta(truth, width=80))
    asm.write_bytes(fasta(contigs, width=70))
    report, blocks, rows = tmp_path / "r.tsv", tmp_path / "b.tsv", tmp_path / "c.tsv"
    argv = [str(EXE), "--eval-placement", str(asm), "--eval-placement-truth", str(gold), "--eval-placement-report", str(report), "--eval-placement-blocks", str(blocks),
            "--eval-placement-contigs", str(rows)]
    if params["k"] != 31:
        argv += ["--eval-placement-k", str(params["k"]), "--eval-placement-band", str(params["band"]), "--eval-placement-relocation", str(params["relocation"]),
                 "--eval-placement-min-anchors", str(params["min_anchors"])]
    subprocess.run(argv, check=True, capture_output=True, timeout=120)
    t_words, _ = _asmmap.fasta_records(gold.read_bytes())
    c_words, _ = _asmmap.fasta_records(asm.read_bytes())
    genomes = sorted({w.split("|")[0] for w in t_words})
    m = _asmmap.evaluate([gold.read_bytes()], [asm.read_bytes()], genomes, **params)
    counts, by = m.read()
    b = m.blocks()
    lengths, rows_of = (b[4] - b[3]).tolist(), [m.truth_genome[t] for t in b[1].tolist()]
    assert counts["blocks"] > 10 and counts["breaks_inter_genome"] > 0
    assert report.read_bytes() == _asmmap.report_text(counts, by, genomes, params["k"], params["band"], params["relocation"], params["min_anchors"], lengths, rows_of).encode()
    assert blocks.read_bytes() == _asmmap.block_rows_text(c_words, t_words, b).encode()
    assert rows.read_bytes() == _asmmap.contig_rows_text(c_words, m.contigs()).encode()
