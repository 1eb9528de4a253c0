"""Build-time guard for the scoring of an overlapper's PAF (ovleval_kernels.hip, a translation unit of libsimmr_hip.so of its own),
in the manner of tests/test_mapeval_resource_guard.py: the unit's kernels are exactly the k_ove_* that DESIGN.md section 4 lists,
none uses scratch or AGPRs or spills, and each one's LDS is what DESIGN.md states for it."""
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
    return resource_usage.collect(source="ovleval.hip")


@pytest.fixture(scope="module")
def listed():
    """kernel -> LDS bytes, from the list of DESIGN.md"""
    rows = re.findall(r"^- `(k_ove_[a-z]+)` — LDS (\d+) B\b", (ROOT / "DESIGN.md").read_text(), re.M)
    assert len(rows) == len(dict(rows)) == 8, rows
    return {name: int(lds) for name, lds in rows}


def test_the_kernels_are_the_ones_design_lists(kernels, listed):
    assert sorted(k["name"] for k in kernels) == sorted(listed)
    assert set(listed) == {"k_ove_index", "k_ove_scan", "k_ove_truth", "k_ove_heads", "k_ove_keys", "k_ove_gather", "k_ove_record", "k_ove_reduce"}


def test_no_scratch_no_agprs_no_spills(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["occupancy"] >= 4, k


def test_lds_is_what_design_states(kernels, listed):
    for k in kernels:
        assert k["lds"] == listed[k["name"]], k
    # and what the tables need: the workgroup scans' words, two and nine counts, four counts and by_len's 41 x 2
    assert listed["k_ove_index"] == listed["k_ove_heads"] == 256 * 4 and listed["k_ove_scan"] == 256 * 8
    assert listed["k_ove_truth"] == 2 * 4 and listed["k_ove_record"] == 9 * 4 and listed["k_ove_reduce"] == (4 + 41 * 2) * 4


def test_mapeval_keeps_its_kernels_behind_the_shared_routines():
    """ovleval_kernels.hip takes mev_lower_bound through MEV_ROUTINES_ONLY and defines no copy of it or of the reader's routines"""
    text = (ROOT / "simmr_amd" / "csrc" / "ovleval_kernels.hip").read_text()
    assert "#define MEV_ROUTINES_ONLY" in text and '#include "mapeval_kernels.hip"' in text
    assert "mev_lower_bound(" in text and not re.search(r"SIMMR_DEV \w+ (?:mev_|fsam_|sam_)\w+\(", text)
    assert "fsam_index_tiles(" in text and "sam_scan_chunks(" in text and sorts_through_the_pair_sort("ovleval.hip")
