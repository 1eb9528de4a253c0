"""Build-time guard for the run-statistics kernel (stats_kernels.hip), in the manner of tests/test_truth_resource_guard.py:
one symbol, no scratch, no AGPRs, an LDS image that lets four workgroups share a CU, four waves per SIMD; it is the one
kernel of its unit, stats.hip, and engine.hip, which it left, is at exactly its budget of 85 kernels."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="stats.hip")


def test_read_stats_kernel(kernels):
    ks = [k for k in kernels if "k_read_stats" in k["name"]]
    assert len(ks) == 1, [k["name"] for k in ks]
    k = ks[0]
    assert k["scratch"] == 0 and k["agpr"] == 0, k
    assert 0 < k["lds"] <= 40960, k
    assert k["occupancy"] >= 4, k


def test_library_size_with_the_stats_kernel(kernels):
    import resource_usage
    assert len(kernels) == 1, [k["name"] for k in kernels]
    engine = resource_usage.collect()
    assert len(engine) == 85 and not [k for k in engine if "k_read_stats" in k["name"]], len(engine)
