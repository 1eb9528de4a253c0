"""Build-time guard for the scoring of a variant caller's VCF (vcfeval_kernels.hip, a translation unit of libsimmr_hip.so of its
own), in the manner of tests/test_ovleval_resource_guard.py: the unit's kernels are exactly the k_vce_* that DESIGN.md section 4
lists, none uses scratch or AGPRs or spills, each keeps at least four waves a SIMD, and each one's LDS is what DESIGN.md states."""
import re
import sys
from pathlib import Path

import pytest

from tests._scaffold import sorts_through_the_pair_sort

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="vcfeval.hip")


@pytest.fixture(scope="module")
def listed():
    """kernel -> LDS bytes, from the list of DESIGN.md"""
    rows = re.findall(r"^- `(k_vce_[a-z]+)` — LDS (\d+) B\b", (ROOT / "DESIGN.md").read_text(), re.M)
    assert len(rows) == len(dict(rows)) == 6, rows
    return {name: int(lds) for name, lds in rows}


def test_the_kernels_are_the_ones_design_lists(kernels, listed):
    assert sorted(k["name"] for k in kernels) == sorted(listed)
    assert set(listed) == {"k_vce_index", "k_vce_scan", "k_vce_truth", "k_vce_gather", "k_vce_record", "k_vce_reduce"}
    text = (ROOT / "simmr_amd" / "csrc" / "vcfeval_kernels.hip").read_text()
    assert set(re.findall(r"^(k_[a-z0-9_]+)\(", text, re.M)) == set(listed)


def test_no_scratch_no_agprs_no_spills(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["occupancy"] >= 4, k


def test_lds_is_what_design_states(kernels, listed):
    for k in kernels:
        assert k["lds"] == listed[k["name"]], k
    # and what the tables need: the workgroup scans' words, three counts, 17 counts and by_qual's 256 x 2, four counts and by_ad's 33 x 2
    assert listed["k_vce_index"] == 256 * 4 and listed["k_vce_scan"] == 256 * 8 and listed["k_vce_gather"] == 0
    assert listed["k_vce_truth"] == 3 * 4 and listed["k_vce_record"] == (17 + 256 * 2) * 4 and listed["k_vce_reduce"] == (4 + 33 * 2) * 4


def test_the_shared_routines_are_taken_not_restated():
    """vcfeval_kernels.hip takes the reader, the name table and the search through MEV_ROUTINES_ONLY and defines no copy of them"""
    text = (ROOT / "simmr_amd" / "csrc" / "vcfeval_kernels.hip").read_text()
    assert "#define MEV_ROUTINES_ONLY" in text and '#include "mapeval_kernels.hip"' in text
    assert not re.search(r"SIMMR_DEV \w+ (?:mev_|fsam_|sam_)\w+\(", text)
    assert "mev_lower_bound(" in text and "mev_name_row(" in text and "fsam_index_tiles(" in text and "sam_scan_chunks(" in text
    assert sorts_through_the_pair_sort("vcfeval.hip")
