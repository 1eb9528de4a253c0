"""Build-time guard for the ground-truth kernels (truth_kernels.hip), in the manner of tests/test_resource_guard.py: one
template, two instantiations (count, write), neither with scratch or AGPRs, both at four waves per SIMD or more; they are
the two kernels of their unit, truth.hip, and engine.hip, which they left, stays within its budget of 85 kernels."""
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="truth.hip")


def test_truth_kernels(kernels):
    ks = [k for k in kernels if re.search(r"k_truth<", k["name"])]
    assert sorted(re.search(r"k_truth<([^>]*)>", k["name"]).group(1) for k in ks) == ["false", "true"], [k["name"] for k in ks]
    for k in ks:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["occupancy"] >= 4 and k["lds"] == 0, k
    assert not [k for k in kernels if "truth" in k["name"] and k not in ks]  # at most three new symbols: there are two


def test_library_size_with_the_truth_kernels(kernels):
    import resource_usage
    assert len(kernels) == 2, [k["name"] for k in kernels]
    engine = resource_usage.collect()
    assert len(engine) <= 85 and not [k for k in engine if "truth" in k["name"]], len(engine)
