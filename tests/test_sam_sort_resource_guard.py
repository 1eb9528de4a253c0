"""The budget of the sorted-SAM unit (simmr_amd/csrc/sam_sort.hip), as the compiler reports it for gfx950: runs without a GPU."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import resource_usage  # noqa: E402


@pytest.fixture(scope="module")
def kernels():
    return resource_usage.collect(source="sam_sort.hip")


def test_at_most_eight_kernels_all_named_k_samsort(kernels):
    assert 1 <= len(kernels) <= 8, [k["name"] for k in kernels]
    assert all(k["name"].startswith("k_samsort") for k in kernels), [k["name"] for k in kernels]
    names = {k["name"].split("(")[0] for k in kernels}
    assert {"k_samsort_size", "k_samsort_hist", "k_samsort_scatter", "k_samsort_write"} <= names


def test_no_scratch_no_agprs_no_vector_spills_four_waves(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0, k
        assert k["occupancy"] >= 4, k


def test_lds_is_what_the_design_states(kernels):
    lds = {k["name"].split("(")[0]: k["lds"] for k in kernels}
    assert lds["k_samsort_scatter"] == 6144 and lds["k_samsort_write"] == 6400 and lds["k_samsort_size"] == 0
    assert max(lds.values()) == 6400


def test_the_unsorted_unit_keeps_its_figures():
    """k_sam_write: 101 VGPRs, four waves, as before the record routine was shared"""
    ks = {k["name"].split("(")[0]: k for k in resource_usage.collect(source="sam.hip")}
    assert set(ks) == {"k_sam_size", "k_sam_scan", "k_sam_offsets", "k_sam_write"}
    assert (ks["k_sam_write"]["vgpr"], ks["k_sam_write"]["occupancy"], ks["k_sam_write"]["lds"]) == (101, 4, 6400)
