"""Build-time guard for the strain-divergence kernels (strain_kernels.hip), the third translation unit of libsimmr_hip.so, in
the manner of tests/test_depth_resource_guard.py: a budget of four kernels of its own (engine.hip's 85 and depth.hip's six are
asserted there), no scratch, no AGPRs, no spills, and draw kernels light enough for eight waves per SIMD."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="strain.hip")


def test_strain_translation_unit_budget(kernels):
    names = sorted(k["name"] for k in kernels)
    assert 0 < len(names) <= 4, names
    for want in ("k_strain_count", "k_strain_scan_tiles", "k_strain_apply"):
        assert sum(want in n for n in names) == 1, (want, names)


def test_no_scratch_no_agprs_no_spills(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k


def test_draw_kernels_occupancy(kernels):
    """four Philox blocks per lane in flight must not cost waves: the pass hides its plane and table loads behind them"""
    for want in ("k_strain_count", "k_strain_apply"):
        k = next(k for k in kernels if want in k["name"])
        assert k["occupancy"] >= 8 and k["lds"] <= 64, k
