"""Build-time guard for the model-fitting kernels (fit_kernels.hip), a translation unit of libsimmr_hip.so of its own, in the
manner of tests/test_pileup_resource_guard.py: every kernel is a k_fit_*, no scratch, no AGPRs, and the add kernel's LDS image is
exactly what its one-workgroup-per-CU occupancy is chosen for."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="fit.hip")


def test_every_kernel_is_a_fit_kernel(kernels):
    names = sorted(k["name"] for k in kernels)
    assert names == ["k_fit_add", "k_fit_compact", "k_fit_density", "k_fit_pairs", "k_fit_ref_scan", "k_fit_segments", "k_fit_sort_key"], names


def test_no_scratch_no_agprs(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0, k


def test_the_add_kernel_is_one_workgroup_per_cu(kernels):
    """135 168 bytes of LDS — the dense identity table of k <= 7 (64 KB), 160 offsets of the quality histogram (60 KB), lengths and
    inserts below 1024 (8 KB) — leave room for one 512-thread workgroup on a CU's 160 KB: two waves per SIMD"""
    k = next(k for k in kernels if k["name"] == "k_fit_add")
    assert k["lds"] == 135168 and k["occupancy"] == 2, k
    assert 2 * k["lds"] > 160 * 1024 >= k["lds"]


def test_engine_unit_keeps_its_kernels():
    import resource_usage
    assert len(resource_usage.collect()) == 85
