"""The budget of the SAM unit (simmr_amd/csrc/sam.hip), as the compiler reports it for gfx950: runs without a GPU."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import resource_usage  # noqa: E402


@pytest.fixture(scope="module")
def kernels():
    return resource_usage.collect(source="sam.hip")


def test_at_most_four_kernels_all_named_k_sam(kernels):
    assert 1 <= len(kernels) <= 4, [k["name"] for k in kernels]
    assert all("k_sam" in k["name"] for k in kernels), [k["name"] for k in kernels]
    assert any(k["name"].startswith("k_sam_write") for k in kernels)


def test_no_scratch_no_agprs_four_waves(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0, k
        assert k["occupancy"] >= 4, k
