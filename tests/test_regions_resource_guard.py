"""Build-time guard for the gold-standard-assembly kernels (regions_kernels.hip), the fourth translation unit of
libsimmr_hip.so, in the manner of tests/test_depth_resource_guard.py: a budget of eight kernels of its own, no scratch, no
AGPRs, no spills."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="regions.hip")


def test_regions_translation_unit_budget(kernels):
    names = sorted(k["name"] for k in kernels)
    assert 0 < len(names) <= 8, names
    for want in ("k_regions_count", "k_regions_scan", "k_regions_runs", "k_regions_flag", "k_regions_compact", "k_regions_columns",
                 "k_regions_bases"):
        assert sum(want in n for n in names) == 1, (want, names)


def test_no_scratch_no_agprs_no_spills(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k


def test_streaming_kernels_keep_eight_waves(kernels):
    """the kernels that walk depth[] and the base stream are bound by memory: they stay light enough for eight waves per SIMD"""
    for want in ("k_regions_count", "k_regions_runs", "k_regions_bases"):
        k = next(k for k in kernels if want in k["name"])
        assert k["occupancy"] >= 8, k
