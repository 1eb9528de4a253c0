"""What staging a FASTA must produce, restated from the rule alone — TEST INFRASTRUCTURE ONLY.

needletail 0.4.1 sequence::normalize(seq, iupac = false) as genome.rs:114 applies it to a record's body, as one 256-entry
table: A C G T N - stay, a c g t n become upper case, u U become T, . ~ become -, space / tab / CR / LF are dropped and
every other byte value becomes N.  On it: the sequences a genome holds after genome.rs:117-148 (--contiguous: one sequence
with an N behind every record, whose size leaves the separators out) and main.rs:117-162 (otherwise: the records with more
than min_size bases).  Nothing here is taken from the device's or the host layer's classifier.

Below the rule: builders of the record bodies that tests/test_gpu_fasta.py and tests/test_fasta_host.py feed in (numpy
throughout; no Python loop per base)."""
from collections import namedtuple

import numpy as np

TILE = 1024  # raw bytes one workgroup of the FASTA kernels owns (FASTA_TILE, simmr_amd/csrc/kernels.hip)
WHITESPACE = b" \t\r\n"

TABLE = np.full(256, ord("N"), dtype=np.uint8)
for _c in b"ACGTN-":
    TABLE[_c] = _c
for _lo, _up in zip(b"acgtn", b"ACGTN"):
    TABLE[_lo] = _up
TABLE[ord("u")] = TABLE[ord("U")] = ord("T")
TABLE[ord(".")] = TABLE[ord("~")] = ord("-")
DROPPED = np.zeros(256, dtype=bool)
DROPPED[list(WHITESPACE)] = True

Layout = namedtuple("Layout", "contigs sizes counts n_staged")
COLS = ("seq_off", "start", "end", "contig", "read_id", "flags", "qual", "seq")  # the columns of a shard of reads


def as_u8(raw) -> np.ndarray:
    return np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray)) else np.asarray(raw, dtype=np.uint8)


def normalize(raw) -> np.ndarray:
    a = as_u8(raw)
    return TABLE[a[~DROPPED[a]]]


def layout(bodies, contiguous, min_size=0) -> Layout:
    """contigs: the staged sequences (uint8 arrays); sizes: their Seq.size; counts: bases per record; n_staged"""
    norm = [normalize(b) for b in bodies]
    counts = [int(s.size) for s in norm]
    if contiguous:  # genome.rs:121-137; main.rs:117 applies no size filter here
        sep = np.frombuffer(b"N", dtype=np.uint8)
        whole = np.concatenate([x for s in norm for x in (s, sep)]) if norm else np.zeros(0, np.uint8)
        return Layout([whole], [sum(counts)], counts, 1)
    kept = [s for s in norm if s.size > min_size]  # main.rs:124: `size <= minimum` is excluded
    return Layout(kept, [int(s.size) for s in kept], counts, len(kept))


def separators(counts) -> np.ndarray:
    """positions of the separators in the --contiguous sequence of records with `counts` bases"""
    c = np.asarray(counts, dtype=np.int64)
    return np.cumsum(c) + np.arange(c.size)


def n_tiles(bodies) -> int:
    return sum(-(-len(b) // TILE) for b in bodies)


def assert_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        lo = max(i - 8, 0)
        raise AssertionError(f"{what}: {int((got != want).sum())} of {got.size} differ, the first at index {i}: "
                             f"got {got[lo:i + 8].tolist()}, expected {want[lo:i + 8].tolist()} (from index {lo})")


# ---- builders ---------------------------------------------------------------------------------------------------------------
ALPHABET30 = np.frombuffer(b"ACGTacgtNnUu-.~RYKMSWBDHVX*\t \r", dtype=np.uint8)  # the alphabet of test_gpu_fasta.bodies()
_P30 = np.r_[np.full(8, 0.11), np.full(ALPHABET30.size - 8, 0.12 / (ALPHABET30.size - 8))]
BASES = np.frombuffer(b"ACGTacgtNn-.~RUu", dtype=np.uint8)  # kept bytes only: plain, lower case, exceptions, an IUPAC code
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def text(rng, n_bytes, width=61) -> bytes:
    """a body of exactly n_bytes: ALPHABET30 in lines of `width`"""
    a = ALPHABET30[rng.choice(ALPHABET30.size, n_bytes, p=_P30)]
    a[width::width + 1] = ord("\n")
    return a.tobytes()


def bases(rng, n, alphabet=BASES) -> np.ndarray:
    return alphabet[rng.integers(0, alphabet.size, n)]


def wrap(seq, width, eol=b"\n") -> bytes:
    """seq in lines of `width`, every line (the last one too) ended by eol"""
    seq, e = as_u8(seq), as_u8(eol)
    full = seq.size // width
    head = np.concatenate([seq[:full * width].reshape(full, width), np.tile(e, (full, 1))], axis=1).reshape(-1)
    tail = seq[full * width:]
    return head.tobytes() + (tail.tobytes() + bytes(eol) if tail.size else b"")


def every_byte_value(rng, n=6000):
    """(a) all 256 values in a seeded order, repeated to n bytes and cut into lines of 61; and the same bytes without the
    four whitespace values and without line ends, so that no tile is short"""
    seq = np.concatenate([rng.permutation(256) for _ in range(-(-n // 256))]).astype(np.uint8)[:n]
    return wrap(seq, 61), seq[~DROPPED[seq]].tobytes()


def tile_loop_bodies(rng, n_cu):
    """(b) 2 * 16 * n_cu + 5 tiles: a record that alone spans more tiles than the grid has workgroups, records of 1, 2 and 3
    tiles, and one of about a grid's worth; the last tile of every record is partly filled"""
    grid = 16 * n_cu
    tiles = [grid + 3, 1, 2, 3, grid - 4]
    assert sum(tiles) == 2 * grid + 5
    return [text(rng, t * TILE - cut) for t, cut in zip(tiles, (37, 900, 1, 513, 64))]


def whitespace(rng, n) -> np.ndarray:
    return as_u8(WHITESPACE)[rng.integers(0, 4, n)]


def empty_tile_bodies(rng):
    """(c) a record with tiles of nothing but whitespace at its start (tiles 0, 1), in its middle (3, 4) and at its end (8, 9),
    between two neighbours; then records of exactly one and two tiles that end in a base, and one of a tile and a byte"""
    gaps = np.concatenate([whitespace(rng, 2048), bases(rng, 700), np.full(3 * 1024, ord("\n"), np.uint8), bases(rng, 5),
                           np.full(1024, ord(" "), np.uint8), bases(rng, 1000), np.tile(as_u8(b"\r\n"), 1024)]).tobytes()
    exact = [bases(rng, n).tobytes() for n in (1024, 2048, 1025)]
    return [text(rng, 1500), gaps, text(rng, 300)] + exact


KEPT_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024)


def _tile_keeping(rng, k, exceptions) -> np.ndarray:
    """one tile of whitespace with k bases at seeded places; `exceptions`: the first kept base is N and the last is -"""
    t = whitespace(rng, TILE)
    at = np.sort(rng.choice(TILE, k, replace=False))
    t[at] = bases(rng, k)
    if exceptions and k:
        t[at[-1]] = ord("-")
        t[at[0]] = ord("N")
    return t


def kept_count_body(rng, reverse=False) -> bytes:
    """(d) one record whose successive tiles keep KEPT_COUNTS bases (or the reverse), every other tile with an exception as
    its first and as its last kept base"""
    ks = KEPT_COUNTS[::-1] if reverse else KEPT_COUNTS
    return np.concatenate([_tile_keeping(rng, k, i % 2 == 0) for i, k in enumerate(ks)]).tobytes()


def kept_count_phases_body(rng):
    """(d) every count of KEPT_COUNTS at every phase of a 32-base mask word (and so of a 16-base code word): before each
    such tile, a tile that keeps as many bases as bring the running total to the phase.  Returns (body, (count, phase) met)."""
    tiles, met, total = [], set(), 0
    for k in KEPT_COUNTS:
        for phase in range(32):
            fill = (phase - total) % 32
            tiles += [_tile_keeping(rng, fill, False), _tile_keeping(rng, k, (k + phase) % 3 == 0)]
            total += fill
            met.add((k, total % 32))
            total += k
    return np.concatenate(tiles).tobytes(), met


def tiny_record_bodies(rng, n=5000):
    """(e) n records whose base counts cycle through 0..40; every third one pure ACGT, the others with N, - and lower case;
    every fifth one over lines of 7, every seventh one over CRLF lines of 3, every eleventh one without a final line end"""
    out = []
    for i in range(n):
        seq = bases(rng, i % 41, ACGT if i % 3 == 0 else BASES)
        if i % 5 == 0:
            b = wrap(seq, 7)
        elif i % 7 == 0:
            b = wrap(seq, 3, b"\r\n")
        else:
            b = seq.tobytes() + (b"" if i % 11 == 0 else b"\n")
        out.append(b)
    return out
