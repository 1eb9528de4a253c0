"""Text staged with simmr_stage_genome (k_pack_ascii) read back against the table of tests/_fasta.py: text that is not
normalised yet, contig lengths around the 16-, 32- and 64-base words of the planes, exceptions on a contig's last base, and
the seam between two uploads of one contig."""
import numpy as np
import pytest

from simmr_amd import PerfectShortErrorProfile, SimmrError, _abi
from tests import _fasta, _oracle, _synth
from tests._fasta import COLS, assert_equal

pytestmark = pytest.mark.gpu

UPLOAD = 64 << 20  # bases per upload of simmr_stage_genome (CHUNK, simmr_amd/csrc/engine.hip)


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from simmr_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


# ---- (h) ----------------------------------------------------------------------------------------------------------------------
def test_text_that_is_not_normalised(eng):
    """Every byte of staged text is one base: lower case, u, . and ~ are mapped as in a FASTA body and any other value is an
    N — the four whitespace values too.  (In a FASTA body those four are line structure and simmr_stage_fasta drops them;
    a contig handed over as text has no lines, so nothing can be dropped without moving every base behind it.)"""
    rng = np.random.default_rng(21)
    values = np.flatnonzero(~_fasta.DROPPED).astype(np.uint8)
    assert values.size == 252
    text = np.concatenate([rng.permutation(values) for _ in range(20)])[:5000]
    blank = np.frombuffer(_fasta.WHITESPACE * 9, dtype=np.uint8)
    eng.stage_genome(0, [text, blank])
    assert eng.genome_info(0) == (2, 5000 + 36)
    assert_equal(eng.unstage(0, 0, 0, 5000), _fasta.TABLE[text], "text of every kept byte value")
    assert _fasta.normalize(text).size == 5000  # the FASTA rule drops none of these either
    assert_equal(eng.unstage(0, 1, 0, 36), np.full(36, ord("N"), np.uint8), "whitespace staged as text")


# ---- (i) ----------------------------------------------------------------------------------------------------------------------
def test_contig_lengths_1_to_130(eng, oracle):
    """The thread that packs a contig's tail always stores two code words and one mask word, whatever is left of its 32 bases."""
    rng = np.random.default_rng(22)
    contigs = []
    for n in range(1, 131):
        c = _fasta.bases(rng, n, _fasta.ACGT)
        if n % 3 == 0:
            c[0] = ord("-") if n % 2 else ord("N")
        if n % 2:
            c[-1] = ord("N")
        elif n % 4 == 0:
            c[-1] = ord("-")
        contigs.append(c)
    eng.stage_genome(1, contigs)
    assert eng.genome_info(1) == (130, 130 * 131 // 2)
    for c, want in enumerate(contigs):
        assert_equal(eng.unstage(1, c, 0, want.size), want, f"contig of {want.size}")
        with pytest.raises(SimmrError):
            eng.unstage(1, c, want.size, 1)
        for first in (1, 15, 16, 17, 31, 32, 33):
            if first < want.size:
                assert_equal(eng.unstage(1, c, first, want.size - first), want[first:], f"contig of {want.size} from {first}")
    # reads through the emit kernels' windows: the profile needs more than 2 * 7 + 3 bases, and as main.rs:117-162 (and
    # so the oracle's genome) leaves shorter sequences out, so does the genome that is drawn from
    prof = PerfectShortErrorProfile(read_length=7, insert_size=3)
    usable = [c for c in contigs if c.size > prof.minimum_genome_size()]
    assert len(usable) == 130 - 17
    eng.stage_genome(2, usable)
    dev = eng.simulate_pe_reads_from_genome(2, prof.pod(), 4000, 23, qual_offset=33).to_host()
    ora = _oracle.simulate_pe(oracle, _oracle.HostGenome(usable), prof.pod(), 4000, 23, qual_offset=33, max_len=16).trimmed()
    assert dev["start"].size == 4000
    for col in COLS:
        assert_equal(dev[col], ora[col], f"reads of the contigs longer than 17, {col}")


# ---- (j) ----------------------------------------------------------------------------------------------------------------------
def test_upload_seam(eng):
    """A contig longer than one upload: k_pack_ascii runs twice for it, the second time with dst_base = base + 64 Mi.  The
    smallest shape that crosses the seam (the upload size is a constant of the library): about 70 MB on either side."""
    n = UPLOAD + 100
    try:
        big, small = _synth.synthetic_contigs_chunked([n, 1000], 24, chunk_words=1 << 18)
        rng = np.random.default_rng(25)
        for contig in (big, small):
            at = rng.integers(0, contig.size, contig.size // 500)
            contig[at] = np.frombuffer(b"N-", dtype=np.uint8)[rng.integers(0, 2, at.size)]
        big[[UPLOAD - 33, UPLOAD - 2, UPLOAD + 1, UPLOAD + 31]] = ord("N")
        big[[UPLOAD - 1, UPLOAD, UPLOAD + 64]] = ord("-")
        big[[n - 1, 0]] = ord("N")
        eng.stage_genome(3, [big, small])
    except (SimmrError, MemoryError) as e:
        if isinstance(e, SimmrError) and e.code != _abi.ENOMEM:
            raise
        pytest.skip("the memory cannot be had")
    assert eng.genome_info(3) == (2, n + 1000)
    for first in (0, UPLOAD - 2000, n - 4096):  # (the contig ends 100 bases behind the seam: the window around it is cut there)
        count = min(4096, n - first)
        assert_equal(eng.unstage(3, 0, first, count), big[first:first + count], f"first contig from {first}")
    with pytest.raises(SimmrError):
        eng.unstage(3, 0, n, 1)
    assert_equal(eng.unstage(3, 1, 0, 1000), small, "second contig")
