"""simmr_asmeval_* where its kernels change trips: the line-index tile and the scan's chunk of tiles, the plane's words, the sort's
tile, the prefix table's buckets, the roll's workgroup batch, the vote sort.  Every case is checked against the plain model for
exact equality of everything (tests/test_gpu_asmeval.py: against_model).  The constants are read from the sources."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _asmeval
from tests._asmeval import fasta, revcomp_bytes
from tests._synth import synthetic_contigs
from tests.test_gpu_asmeval import against_model, eng  # noqa: F401  (the engine fixture)

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def constant(file, name):
    return int(re.search(rf"#define {name} (\d+)u", (CSRC / file).read_text()).group(1))


FSAM_TILE = constant("fit_sam_kernels.hip", "FSAM_TILE")
SAMSORT_TILE = constant("sam_sort_kernels.hip", "SAMSORT_TILE")
ASM_WG, ASM_WORD, ASM_CHUNK = (constant("asmeval_kernels.hip", n) for n in ("ASM_WG", "ASM_WORD", "ASM_CHUNK"))
SCAN_CHUNK_TILES = 256   # sam_scan_chunks takes 256 sums a round
K = 15
G = ["gA", "gB", "gC"]
A, B, Cc = (x.tobytes() for x in synthetic_contigs([72000, 9000, 9000], 4242))


def test_the_constants_are_what_the_cases_assume():
    assert (FSAM_TILE, SAMSORT_TILE, ASM_WG, ASM_WORD, ASM_CHUNK) == (4096, 2048, 256, 32, 256)
    assert "base + threadIdx.x" in (CSRC / "sam_kernels.hip").read_text() and "base += 256u" in (CSRC / "sam_kernels.hip").read_text()


def padded(name: bytes, seq: bytes, start: int, width=60):
    """a record whose first sequence line starts at byte `start` of the text"""
    head = b">" + name + b" "
    return head + b"x" * (start - len(head) - 1) + b"\n" + b"".join(seq[j:j + width] + b"\n" for j in range(0, len(seq), width))


@pytest.mark.parametrize("edge", [FSAM_TILE, SCAN_CHUNK_TILES * FSAM_TILE])
def test_a_sequence_line_that_starts_around_a_tile_edge_and_a_chunk_edge(eng, edge):
    for d in (-1, 0, 1):
        truth = padded(b"gA|s", A[:300], edge + d) + fasta([(b"gB|s", B[:200])])
        contigs = padded(b"c1", A[20:280], edge + d, width=7) + fasta([(b"c2", B[:100] + A[:50])])
        against_model(eng, [truth], [contigs], f"line start at {edge} + {d}", G, K)


def test_kmers_across_tile_edges_and_across_31_one_base_lines(eng):
    truth = fasta([(b"gA|s", A[:6000]), (b"gB|s", B[:3000])], width=61)   # lines of 62 bytes: no line ends on a tile edge
    against_model(eng, [truth], [fasta([(b"c1", A[100:5900])], width=1)], "one base a line, k = 31", G, 31)
    against_model(eng, [fasta([(b"gA|s", A[:6000])], width=1)], [truth], "the truth one base a line", G, 31)


def test_a_record_boundary_directly_behind_a_tile_edge(eng):
    first = b">gA|s\n"
    seq = A[:FSAM_TILE - len(first) - 1]
    text = first + seq + b"\n" + fasta([(b"gB|s", B[:500])])   # the second '>' is byte FSAM_TILE
    assert text[FSAM_TILE:FSAM_TILE + 1] == b">"
    m = against_model(eng, [text], [text.replace(b"gA|", b"c").replace(b"gB|", b"d")], "a header on a tile's first byte", G, K)
    c = m.read()[0]
    assert c["novel"] == 0 and c["kmers"] == len(seq) - K + 1 + 500 - K + 1   # no k-mer joins two records


def test_a_record_at_every_offset_of_a_plane_word_and_a_kmer_on_the_last_base(eng):
    truth = fasta([(b"gA|s", A[:400])])
    for lead in range(0, 2 * ASM_WORD + 1):
        contigs = fasta([(b"lead", A[1000:1000 + lead]), (b"c", A[:64]), (b"tail", A[300:400])], width=50)
        m = against_model(eng, [truth], [contigs], f"{lead} bases in front", G, K)
        assert m.contigs()[2].tolist()[1:] == [50, 86]
    against_model(eng, [fasta([(b"gA|a", A[:lead]), (b"gB|b", A[:64])]) for lead in range(17)], [truth], "the truth at the offsets, an add each", G, K)


@pytest.mark.parametrize("n", [SAMSORT_TILE - 1, SAMSORT_TILE, SAMSORT_TILE + 1, SAMSORT_TILE + 2, 1, 255, 256, 257, 4097])
def test_occurrences_and_entries_around_the_sort_tile_and_the_workgroup(eng, n):
    m = against_model(eng, [fasta([(b"gA|s", A[:n + K - 1])])], [fasta([(b"c", revcomp_bytes(A[:n + K - 1]))])], f"{n} occurrences", G, K)
    assert m.read()[0]["truth_kmers"] == n and n - 3 <= len(m.order) <= n
    against_model(eng, [fasta([(b"gA|s", A[:n + K - 1])])], [fasta([(b"c", A[:n + K - 1])])], f"{n} occurrences, the plain search", G, K, plain_search=True)


def test_one_bucket_that_holds_every_entry_and_empty_buckets(eng):
    tails = [bytes(b"ACGT"[(i >> s) & 3] for s in (0, 2, 4)) for i in range(40)]
    truth = fasta([(b"gA|%d" % i, b"A" * 12 + t) for i, t in enumerate(tails)])
    m = _asmeval.evaluate([truth], [], G, K)
    assert len(m.order) == 40 and all(k.startswith("A" * 12) for k in m.order)   # 6 table bits: the first three bases, AAA for all
    # every entry, and beside every entry the keys that differ in the lowest and in the highest of the 2k bits
    probes = []
    for i, key in enumerate(m.order):
        for j, probe in enumerate((key, key[:-1] + "ACGT"[("ACGT".index(key[-1]) + 1) % 4], "CGTA"["ACGT".index(key[0])] + key[1:], "T" + key[1:])):
            probes.append((b"p%d_%d" % (i, j), probe.encode()))
    against_model(eng, [truth], [fasta(probes)], "probes at every entry and gap", G, K)
    against_model(eng, [truth], [fasta(probes)], "probes, the plain search", G, K, plain_search=True)
    spread = fasta([(b"gB|s", B[:3000])])
    m = _asmeval.evaluate([spread], [], G, K)
    probes = [(b"q%d" % i, (key[:-1] + "ACGT"[("ACGT".index(key[-1]) + 1) % 4]).encode()) for i, key in enumerate(m.order[::7])]
    against_model(eng, [spread], [fasta(probes + [(b"all", B[:3000])])], "gaps between spread entries", G, K)


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_contigs_at_the_workgroup_batch(eng, d):
    n = ASM_WG * ASM_WORD + d
    against_model(eng, [fasta([(b"gA|s", A[:9000])])], [fasta([(b"c", A[:n])], width=80)], f"{n} bases", G, K)


def test_votes_past_one_sort_tile_and_a_tie_of_the_first_and_the_last_row(eng):
    truth = fasta([(b"gA|s", A), (b"gB|s", B), (b"gC|s", Cc)], width=100)
    lanes = len(A) // ASM_WORD
    assert lanes > SAMSORT_TILE   # a vote pair a lane at least
    m = against_model(eng, [truth], [fasta([(b"long", A), (b"tie", Cc[:500] + b"N" + A[:500]), (b"b", B[:100])], width=100)], "votes", G, K)
    assert m.contigs()[4].tolist() == [0, 0, 1] and m.contigs()[5].tolist()[1] == 500 - K + 1
