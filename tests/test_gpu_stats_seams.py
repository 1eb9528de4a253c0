"""The run statistics (simmr_stats_add; stats_kernels.hip, stats.hip) at the four bounds k_read_stats' comment derives: the flush
inside the batch loop, the 16-bit halves of its packed words and per-row class counts, the whole range of a quality byte, and the
longest read.  The cases come from tests/_stats_cases.py, whose builders assert that each byte sits where it is meant to
(tests/test_stats_host.py pins where each case lands in the model without a GPU); what is expected is tests/_stats.model on the
host columns — or, for the flush case, the unit batch's model times the batches, which the host test holds to tests/_stats.model.
Every comparison is exact (tests/_stats.assert_stats).  The engine is the module's own, with its own genomes in its own slots.

Which path each test is the first to enter:
  test_flush
      the flush at since_flush == STATS_FLUSH_BATCHES in the middle of the loop: STATS_FLUSH_BATCHES x STATS_WGS_PER_CU x CUs + 3
      batches, so three workgroups take 4097; the 16-bit halves of a block's cycle-0 words stand at 16 384 and its quality sum at
      255 x 16 384 when it comes; the three batches behind it are counted too;
  test_homopolymer_reads_fill_one_half
      65 535 in one half of same01 / same23 with nothing in the other (a read that is one unedited letter, all four letters on
      both strands), nm = 65 535 with an empty diagonal, 65 535 bytes of class "other", gc = L;
  test_every_quality_byte
      q = (byte - qual_offset) & 255 below the offset (the wrap) and at 255, in qual_n, qual_mismatch and cycle_qsum at cycles 0,
      255, 256 and 511;
  test_a_65536_base_read_is_refused_by_stats_and_taken_by_truth
      the refusal at STATS_MAX_L + 1, which k_truth — the same walker without the cap — takes."""
import math
import time

import numpy as np
import pytest

from simmr_amd import SimmrError, _abi
from tests import _stats, _truth
from tests import _stats_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def genomes():
    return cases.host_genomes()


@pytest.fixture(scope="module")
def own(genomes):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from simmr_amd.engine import Engine
    e = Engine(0)
    try:
        cases.stage(e, genomes)
        yield e
    finally:
        e.close()


@pytest.fixture(params=[0, 16], ids=["compact", "slot16"])
def layout(request):
    return request.param


def device_stats(eng, reads, n_sets):
    eng.stats_reset()
    eng.stats_add(reads, n_sets)
    return eng.stats()


def test_flush(own, oracle, genomes):
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    grid_cap = cases.WGS_PER_CU * cus
    n_batches = cases.FLUSH_BATCHES * grid_cap + 3
    assert math.ceil(n_batches / min(n_batches, grid_cap)) == cases.FLUSH_BATCHES + 1 == 4097
    unit = cases.uniform_unit(oracle, genomes)
    t0 = time.perf_counter()
    try:
        dev = cases.device_tiled(unit, n_batches, own.device)
    except (SimmrError, MemoryError, torch.cuda.OutOfMemoryError) as e:
        if isinstance(e, SimmrError) and e.code != _abi.ENOMEM:
            raise
        pytest.skip("the memory cannot be had")
    assert dev.n_reads == cases.WG_READS * n_batches and dev.total_bases == 40 * n_batches == dev.seq.numel()
    for n_sets in (2, 1):
        want = cases.scaled(_stats.model(oracle, unit, genomes, n_sets, cases.QUAL_OFFSET), n_batches)
        _stats.assert_stats(device_stats(own, dev, n_sets), want, f"{n_batches} uniform batches, {n_sets} sets")
    # the same columns without a flush inside the loop: one workgroup's STATS_FLUSH_BATCHES batches, spread over the grid
    assert math.ceil(cases.FLUSH_BATCHES / min(cases.FLUSH_BATCHES, grid_cap)) <= cases.FLUSH_BATCHES
    less = cases.first_reads(dev, cases.FLUSH_BATCHES * cases.WG_READS)
    for n_sets in (2, 1):
        want = cases.scaled(_stats.model(oracle, unit, genomes, n_sets, cases.QUAL_OFFSET), cases.FLUSH_BATCHES)
        _stats.assert_stats(device_stats(own, less, n_sets), want, f"uniform batches without a flush, {n_sets} sets")
    print(f"test_flush: {dev.n_reads} reads, {time.perf_counter() - t0:.2f} s of wall time")


def test_homopolymer_reads_fill_one_half(own, oracle, genomes, layout):
    case = cases.homopolymer_reads(oracle, genomes)
    want = _stats.model(oracle, case.host, genomes, 1, cases.QUAL_OFFSET)
    got = device_stats(own, cases.device_reads(case.host, layout, own.device), 1)
    _stats.assert_stats(got, want, "reads of one letter")
    off = got["pair"].copy()
    off[np.arange(4), np.arange(4)] = 0
    off[3, 4] -= np.uint64(cases.MAX_L)  # the N read on the T contig
    off[1, 2] -= np.uint64(cases.MAX_L)  # the G read on the C contig
    assert np.array_equal(off, case.all_edit) and got["pair"][4, 4] == 0
    assert [int(got["pair"][c, c]) for c in range(4)] == 4 * [2 * cases.MAX_L]
    assert got["gc_hist"][100] == 5 and got["nm_hist"][63] == 3 and got["nm_hist"][0] == 8


@pytest.mark.parametrize("qual_offset", [33, 0])
def test_every_quality_byte(own, oracle, genomes, layout, qual_offset):
    host = cases.quality_range(oracle, genomes)
    want = _stats.model(oracle, host, genomes, 2, qual_offset)
    got = device_stats(own, cases.device_reads(host, layout, own.device, qual_offset), 2)
    _stats.assert_stats(got, want, f"every quality byte under qual_offset {qual_offset}")
    assert (got["qual_n"] > 0).all() and got["qual_mismatch"][255] >= 4


def test_a_65536_base_read_is_refused_by_stats_and_taken_by_truth(own, oracle, genomes, layout):
    case = cases.homopolymer_reads(oracle, genomes)
    bad = cases.device_reads(case.too_long, layout, own.device)
    good = cases.device_reads(case.good, layout, own.device)
    own.stats_reset()
    own.stats_add(bad, 1)  # returns: the add only enqueues
    with pytest.raises(SimmrError) as ei:
        own.stats()
    assert ei.value.code == _abi.EINVAL and "65535" in str(ei.value)
    own.stats_add(good, 1)
    with pytest.raises(SimmrError) as ei:  # sticky until the reset
        own.stats()
    assert ei.value.code == _abi.EINVAL
    nm = own.truth(bad).nm[:3].cpu().numpy()
    assert nm.tolist() == _truth.model(oracle, case.too_long, genomes)["nm"].tolist() == case.nm
    _stats.assert_stats(device_stats(own, good, 1), _stats.model(oracle, case.good, genomes, 1, cases.QUAL_OFFSET), "after the reset")
