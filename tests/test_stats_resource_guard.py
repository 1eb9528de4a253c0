"""Build-time guard for the run-statistics kernel (stats_kernels.hip), in the manner of tests/test_truth_resource_guard.py:
one symbol, no scratch, no AGPRs, an LDS image that lets four workgroups share a CU, four waves per SIMD, and the library
at exactly its budget of 88 kernels."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect()


def test_read_stats_kernel(kernels):
    ks = [k for k in kernels if "k_read_stats" in k["name"]]
    assert len(ks) == 1, [k["name"] for k in ks]
    k = ks[0]
    assert k["scratch"] == 0 and k["agpr"] == 0, k
    assert 0 < k["lds"] <= 40960, k
    assert k["occupancy"] >= 4, k


def test_library_size_with_the_stats_kernel(kernels):
    assert len(kernels) == 88, len(kernels)
