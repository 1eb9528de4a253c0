"""The correval unit (simmr_correval_*; correval.hip, correval_kernels.hip) at the sizes where each of its pieces takes another path, every
case against the plain model of tests/_correval.py for exact equality: the smallest inputs that cross each loop once."""
import random
import re
from pathlib import Path

import pytest

from simmr_amd.engine import Engine
from tests import _correval as M
from tests._correval import emitted, fastq_record, make_read, sam_record, true_read
from tests.test_gpu_correval import device, invariants, same

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def _define(file, name):
    return int(re.search(r"#define %s (\d+)u" % name, (CSRC / file).read_text()).group(1))


TILE = _define("fit_sam_kernels.hip", "FSAM_TILE")
WG_RECS = _define("correval_kernels.hip", "CEV_WG_RECS")
WGS_PER_CU = int(re.search(r"constexpr uint32_t WGS_PER_CU = (\d+);", (CSRC / "correval.hip").read_text()).group(1))
SCAN_CHUNK = 256   # tile counts a round of sam_scan_chunks
SORT_WG = 256      # entries past which the sort and the gather take a second workgroup


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def reads_of(seed, n, L, first_id=1):
    rng = random.Random(seed)
    return [make_read(rng, first_id + i, L if isinstance(L, int) else rng.choice(L), rng.choice((None, 0, 1)), rng.random() < 0.5)
            for i in range(n)], rng


def with_errors(rng, R, rate):
    out = []
    for r in R:
        L = len(r["seq"])
        out.append(make_read(rng, r["rid"], L, r["mate"], r["rev"], [i for i in range(L) if rng.random() < rate], ref=r["ref"]))
    return out


def corrected(rng, r):
    e, t = list(emitted(r)), true_read(r)
    for i in range(len(e)):
        if e[i] != t[i] and rng.random() < 0.7:
            e[i] = t[i]
        elif rng.random() < 0.01:
            e[i] = rng.choice("ACGTN")
    s = "".join(e)
    return s[:rng.randrange(len(s) + 1)] if rng.random() < 0.05 else s


def check(eng, truth_adds, read_adds, what):
    want = M.score(truth_adds, read_adds)
    got = device(eng, truth_adds, read_adds)
    same(got, want, what)
    invariants(got, what)
    return got[0]


def test_past_one_sort_workgroup_and_one_batch(eng):
    R, rng = reads_of(1, SORT_WG + 44, (20, 33, 40))
    R = with_errors(rng, R, 0.05)
    truth = "".join(sam_record(r) for r in R).encode()
    reads = "".join(fastq_record(r, corrected(rng, r)) for r in R[:WG_RECS + 1]).encode()
    assert len(truth) > TILE and len(reads) < TILE
    c = check(eng, [truth], [reads], "300 entries, 17 records")
    assert c["truth_entries"] == SORT_WG + 44 and c["records"] == WG_RECS + 1 and c["missing"] == SORT_WG + 44 - WG_RECS - 1


def padded(records, pad_record, want_newline_at):
    """the records joined, with pad_record(k, n) in place of record k so that a '\\n' stands at every offset of want_newline_at"""
    text, k = "", 0
    for at in sorted(want_newline_at):
        while len(text) + len(records[k]) + 400 < at:
            text += records[k]
            k += 1
        first_line = records[k].index("\n")
        text += pad_record(k, at - len(text) - first_line)
        assert text[at] == "\n", (at, text[at - 3:at + 3])
        k += 1
    return text + "".join(records[k:])


def test_a_newline_at_a_tile_edge(eng):
    R, rng = reads_of(2, 260, 40)
    R = with_errors(rng, R, 0.04)
    fq = [fastq_record(r, corrected(rng, r)) for r in R]
    # the header line's '\n' as the last byte of the first tile, and another as the first byte of the third
    reads = padded(fq, lambda k, n: fq[k].replace("\n", " " + "c" * (n - 1) + "\n", 1), [TILE - 1, 2 * TILE])
    sam = [sam_record(r) for r in R]
    truth = padded(sam, lambda k, n: sam[k][:-1] + "\tCO:Z:" + "x" * (n - 6) + "\n", [TILE - 1, 2 * TILE])
    assert reads[TILE - 1] == "\n" and reads[2 * TILE] == "\n" and truth[TILE - 1] == "\n" and truth[2 * TILE] == "\n"
    c = check(eng, [truth.encode()], [reads.encode()], "a newline at a tile's edge")
    assert c["records"] == 260 and c["unknown_read"] == 0


def test_past_one_grid_trip_and_one_scan_round(eng):
    """more records than the capped grid holds in one trip (the cap is WGS_PER_CU workgroups a CU, 16 records each), and texts of more
    than 256 tiles, which take the scan over the tile counts into its second round"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * WGS_PER_CU * WG_RECS + 40
    R, rng = reads_of(3, n, 40)
    R = with_errors(rng, R, 0.02)
    truth = "".join(sam_record(r, rname="contig_0000001_of_the_reference") for r in R).encode()
    order = list(R)
    rng.shuffle(order)
    reads = "".join(fastq_record(r, corrected(rng, r), name=M.read_name(r) + " " + "d" * 60) for r in order).encode()
    assert len(truth) > SCAN_CHUNK * TILE and len(reads) > SCAN_CHUNK * TILE
    c = check(eng, [truth], [reads], "past one grid trip")
    assert c["scored"] == n and c["missing"] == 0


def test_two_truth_adds_the_second_growing_the_buffers(eng):
    R, rng = reads_of(4, 700, (36, 150))
    R = with_errors(rng, R, 0.03)
    first, second = "".join(sam_record(r) for r in R[:3]).encode(), "".join(sam_record(r) for r in R[3:]).encode()
    # the first add's room is its bytes; its three reads fill a part of it, so the fourth read's planes begin inside that room and the
    # later ones lie in what the second add's room adds
    used = sum(len(r["seq"]) for r in R[:3])
    assert used < len(first) < used + sum(len(r["seq"]) for r in R[3:12]) and len(second) > 20 * len(first)
    reads = "".join(fastq_record(r, corrected(rng, r)) for r in R).encode()
    c = check(eng, [first, second], [reads], "two truth adds")
    assert c["truth_entries"] == 700 and c["scored"] == 700
    ends = [i + 1 for i, b in enumerate(reads) if b == 10]
    cuts = [0] + [ends[k] for k in (4 * 100 - 1, 4 * 433 - 1)] + [len(reads)]
    check(eng, [first, second[:second.index(b"\n", len(second) // 2) + 1], second[second.index(b"\n", len(second) // 2) + 1:]],
          [reads[a:b] for a, b in zip(cuts, cuts[1:])], "three truth adds, three adds")
