"""Build-time guard for the SAM route of the model fit (fit_sam_kernels.hip, a translation unit of libsimmr_hip.so of its own), in
the manner of tests/test_fit_resource_guard.py: every kernel is a k_fsam_*, none uses scratch or AGPRs, and the two kernels with
LDS tables keep two workgroups on a CU."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="fit_sam.hip")


def test_every_kernel_is_a_sam_fit_kernel(kernels):
    names = sorted(k["name"] for k in kernels)
    assert names == ["k_fsam_expand", "k_fsam_index", "k_fsam_md", "k_fsam_record", "k_fsam_scan", "k_fsam_windows"], names


def test_no_scratch_no_agprs(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0, k


def test_lds_tables_leave_two_workgroups_a_cu(kernels):
    """the quality table of k_fsam_record (160 offsets x 96 words) and the dense table of k_fsam_windows (4^7 words)"""
    by = {k["name"]: k for k in kernels}
    assert by["k_fsam_record"]["lds"] == 160 * 96 * 4 and by["k_fsam_windows"]["lds"] == 4 ** 7 * 4 + 16
    for name in ("k_fsam_record", "k_fsam_windows"):
        assert 2 * by[name]["lds"] <= 160 * 1024 and by[name]["occupancy"] >= 2, by[name]
