"""simmr_bineval_* where its kernels change trips, tiles and chunks, against the plain model of tests/_bineval.py: names that straddle a
line-index tile and the scan's chunk of 256 tiles, counts around a workgroup's 256 and the sort's tile, runs of equal truncated
hashes across those edges, genomes around 1024, one bin with every genome, one genome in more bins than a workgroup has threads, and
texts past one trip of every kernel's grid-stride loop.  The constants are read from the sources."""
import re
from pathlib import Path

import pytest

from simmr_amd.engine import Engine
from tests import _bineval
from tests._bineval import bins_text, truth_text
from tests.test_gpu_bineval import run

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def constant(file, pattern):
    m = re.search(pattern, (CSRC / file).read_text())
    assert m, (file, pattern)
    return int(m.group(1))


FSAM_TILE = constant("fit_sam_kernels.hip", r"#define FSAM_TILE (\d+)u")
SORT_TILE = constant("engine_internal.hpp", r"SAMSORT_PAIRS_TILE = (\d+)")
BIN_CHUNK = constant("bineval_kernels.hip", r"#define BIN_CHUNK (\d+)u")
WGS_PER_CU = constant("bineval.hip", r"constexpr uint32_t WGS_PER_CU = (\d+);")
assert (FSAM_TILE, SORT_TILE, BIN_CHUNK) == (4096, 2048, 256)
GENOMES = ["gA", "gB", "gC"]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def check(eng, t, b, label, genomes=GENOMES, hash_bits=64):
    model = _bineval.evaluate([t], [b], genomes)
    assert model.malformed is None, label
    run(eng, [t], [b], label, genomes, hash_bits, model)
    return model


@pytest.mark.parametrize("edge", [FSAM_TILE, 256 * FSAM_TILE])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_names_that_straddle_a_tile_and_a_chunk_of_tiles(eng, edge, delta):
    """the contig name of a truth line, and the contig and bin names of a record, lie across byte `edge` (+ delta); with delta 0 the
    line behind it starts on a tile's first byte"""
    name, binn = b"NODE_17_length_5231_cov_8.1", b"metabat.bin.0042"
    for side in ("truth", "candidate contig", "candidate bin"):
        def pad(prefix_len, make):
            rows, size, i = [], 0, 0
            while True:
                row = make(i)
                if size + len(row) > prefix_len - 40:
                    break
                rows.append(row)
                size += len(row)
                i += 1
            last = make(i)
            fill = prefix_len - size - len(last)
            assert fill >= 0
            return rows, i, fill
        if side == "truth":
            at = edge + delta - len(name) // 2  # the name's middle on the edge
            mk = lambda i: truth_text([(b"f%d" % i, 3, b"gB")])
            rows, i, fill = pad(at, mk)
            t = b"".join(rows) + truth_text([(b"f%d" % i + b"x" * fill, 3, b"gB")]) + truth_text([(name, 77, b"gA"), (b"after", 5, b"gC")])
            assert t.index(name) == at
            b = bins_text([(name, binn), (b"after", binn), (b"f0", b"other")])
        else:
            t = truth_text([(name, 77, b"gA"), (b"after", 5, b"gC"), (b"f0", 3, b"gB")])
            at = edge + delta - (len(name) // 2 if side == "candidate contig" else len(name) + 1 + len(binn) // 2)
            mk = lambda i: bins_text([(b"f0", b"b%d" % (i % 7))])
            rows, i, fill = pad(at, mk)
            b = b"".join(rows) + bins_text([(b"f0", b"b0" + b"y" * fill)]) + bins_text([(name, binn), (b"after", binn)])
            assert b.index(name + b"\t") == at
        m = check(eng, t, b, f"{side} at {edge}{delta:+d}")
        assert m.read()[0]["unknown_contig"] == 0 and m.read()[0]["assigned"] == 3


COUNTS = [1, 255, 256, 257, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, SORT_TILE + 2]


@pytest.mark.parametrize("n", COUNTS)
def test_contigs_records_bins_and_cells_around_a_workgroup_and_a_sort_tile(eng, n):
    """n truth contigs, n records, n bins and n cells at once (a bin per contig), then n records in three bins with 4-bit hashes: runs of
    equal truncated hashes that cross the workgroup and sort-tile edges"""
    truth = [(b"contig_%d" % i, 10 + i % 97, GENOMES[i % 3].encode()) for i in range(n)]
    t = truth_text(truth)
    m = check(eng, t, bins_text([(c, b"bin_" + c) for c, _, _ in truth]), f"{n} of each")
    assert m.read()[0]["bins"] == m.read()[0]["cells"] == n
    for bits in (4, 0):
        m = check(eng, t, bins_text([(c, b"bin_%d" % (i % 3 if i % 5 else i % 4)) for i, (c, _, _) in enumerate(truth)]), f"{n} records, {bits} bits", hash_bits=bits)
        assert m.read()[0]["assigned"] == n


@pytest.mark.parametrize("n_genomes", [1, 1024, 1025])
def test_genomes_around_1024_and_one_bin_that_holds_them_all(eng, n_genomes):
    genomes = [f"genome_{i:04d}" for i in range(n_genomes)]
    truth = [(b"c%d" % i, 1 + i, genomes[i % n_genomes].encode()) for i in range(n_genomes + 7)] + [(b"none", 9, b".")]
    m = check(eng, truth_text(truth), bins_text([(c, b"everything") for c, _, _ in truth]), f"{n_genomes} genomes in one bin", genomes)
    c, by = m.read()
    assert c["bins"] == 1 and c["cells"] == n_genomes + 1 and int(by[:n_genomes, 4].sum()) == n_genomes


def test_one_genome_spread_over_more_bins_than_a_workgroup_has_threads(eng):
    n = 3 * BIN_CHUNK + 5
    truth = [(b"c%d" % i, 50, b"gB") for i in range(n)] + [(b"tie", 50, b"gB")]
    bins = [(b"c%d" % i, b"bin%d" % i) for i in range(n)] + [(b"tie", b"bin7")]
    m = check(eng, truth_text(truth), bins_text(bins), "one genome, many bins")
    c, by = m.read()
    assert int(by[1, 4]) == n and int(by[1, 5]) == 7 and int(by[1, 6]) == 100 and c["pairs_genomes"] == (n + 1) * n // 2


def test_past_one_trip_of_every_grid_stride_loop(eng):
    """truth contigs, records, bins and cells beyond what any kernel's grid holds in one trip (WGS_PER_CU workgroups a CU: of 256 lines or
    items, of 16 records for the genomes, of a 4096-byte tile for the line index), so that every workgroup loops; short names keep
    the two texts at a few MB"""
    import torch
    trip = torch.cuda.get_device_properties(0).multi_processor_count * WGS_PER_CU * BIN_CHUNK
    n = trip + BIN_CHUNK + 3
    truth = [(b"%x" % i, i & 63, GENOMES[i % 3].encode()) for i in range(n)]
    t = truth_text(truth)
    b = bins_text([(c, b"bin_%08x" % i) for i, (c, _, _) in enumerate(truth)] + [(b"%x" % (n - 1), b"late")])
    assert trip * FSAM_TILE // BIN_CHUNK < min(len(t), len(b)) < 8 << 20, "both texts pass one trip of the line index"
    m = check(eng, t, b, "past one trip")
    c = m.read()[0]
    assert c["truth_records"] == n and c["records"] == n + 1 and c["repeated"] == 1 and c["cells"] == n
    assert c["bins"] == n + 1, "a bin that only a repeated record names is a bin, without a cell"
    # and long runs past a trip: every record in one of four bins, the truth and the records sorted over four bits of the hash
    b = bins_text([(c_, b"bin%d" % (i % 4)) for i, (c_, _, _) in enumerate(truth)])
    m = check(eng, t, b, "past one trip, four bins, 4 bits", hash_bits=4)
    assert m.read()[0]["bins"] == 4 and m.read()[0]["cells"] == 12
