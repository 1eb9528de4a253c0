"""Build-time guard for the scoring of an aligner's SAM (mapeval_kernels.hip, a translation unit of libsimmr_hip.so of its own), in
the manner of tests/test_fit_sam_resource_guard.py: every kernel is a k_mev_*, none uses scratch or AGPRs or spills, and the
record kernel's LDS is its by_mapq table."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="mapeval.hip")


def test_every_kernel_is_a_mapeval_kernel(kernels):
    names = sorted(k["name"] for k in kernels)
    assert names == ["k_mev_gather", "k_mev_index", "k_mev_record", "k_mev_reduce", "k_mev_scan", "k_mev_truth"], names


def test_no_scratch_no_agprs_no_spills(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k.get("sgpr_spill", 0) == 0, k


def test_lds_is_what_the_tables_need(kernels):
    """by_mapq privatised: 256 MAPQs x (correct, wrong) words; the index and the scan keep the workgroup scan's words; the truth
    pass and the gather keep nothing"""
    by = {k["name"]: k for k in kernels}
    assert by["k_mev_record"]["lds"] == 256 * 2 * 4
    assert by["k_mev_index"]["lds"] == 256 * 4 and by["k_mev_scan"]["lds"] == 256 * 8
    assert by["k_mev_truth"]["lds"] == 0 and by["k_mev_gather"]["lds"] == 0 and by["k_mev_reduce"]["lds"] == 5 * 4
    for k in kernels:
        assert k["occupancy"] >= 4, k
