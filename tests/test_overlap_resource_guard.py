"""The budget of the overlap unit (simmr_amd/csrc/overlap.hip), as the compiler reports it for gfx950, and the sorted-SAM unit's
figures after its sort became a function both units call: runs without a GPU."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import resource_usage  # noqa: E402


@pytest.fixture(scope="module")
def kernels():
    return resource_usage.collect(source="overlap.hip")


def test_eight_kernels_all_named_k_ovl(kernels):
    names = {k["name"].split("(")[0] for k in kernels}
    assert names == {"k_ovl_add", "k_ovl_keys", "k_ovl_partners", "k_ovl_scan", "k_ovl_offsets", "k_ovl_size", "k_ovl_window", "k_ovl_write"}
    assert all(k["name"].startswith("k_ovl_") for k in kernels) and len(kernels) == len(names)


def test_no_scratch_no_agprs_no_vector_spills_four_waves(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0, k
        assert k["occupancy"] >= 4, k


def test_lds_is_what_the_design_states(kernels):
    lds = {k["name"].split("(")[0]: k["lds"] for k in kernels}
    assert lds == {"k_ovl_add": 0, "k_ovl_keys": 0, "k_ovl_partners": 2048, "k_ovl_scan": 2048, "k_ovl_offsets": 2048, "k_ovl_size": 1024,
                   "k_ovl_window": 1040, "k_ovl_write": 39936}
    assert 4 * lds["k_ovl_write"] <= 160 * 1024  # four workgroups of the writer a CU
    design = (ROOT / "DESIGN.md").read_text()
    assert "39 936" in design and "k_ovl_write" in design


def test_the_sorted_sam_unit_keeps_its_set_and_figures():
    ks = {k["name"].split("(")[0]: k for k in resource_usage.collect(source="sam_sort.hip")}
    assert set(ks) == {"k_samsort_size", "k_samsort_hist", "k_samsort_digit_scan", "k_samsort_scatter", "k_samsort_gather", "k_samsort_scan",
                       "k_samsort_offsets", "k_samsort_write"}
    for k in ks.values():
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k["occupancy"] >= 4, k
    lds = {n: k["lds"] for n, k in ks.items()}
    assert lds["k_samsort_scatter"] == 6144 and lds["k_samsort_write"] == 6400 and lds["k_samsort_size"] == 0 and max(lds.values()) == 6400
