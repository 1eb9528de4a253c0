"""Build-time guard for the scoring of a read classifier's calls (taxeval_kernels.hip, a translation unit of libsimmr_hip.so of its
own), in the manner of tests/test_vcfeval_resource_guard.py: the unit's kernels are exactly the k_txe_* that DESIGN.md section 4
lists, none uses scratch or AGPRs or spills, each keeps at least four waves a SIMD, and each one's LDS is what DESIGN.md states."""
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

NAMES = {"k_txe_index", "k_txe_scan", "k_txe_nodes", "k_txe_lineage", "k_txe_look", "k_txe_truth", "k_txe_heads", "k_txe_record", "k_txe_reduce",
         "k_txe_rollup"}


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="taxeval.hip")


@pytest.fixture(scope="module")
def listed():
    """kernel -> LDS bytes, from the list of DESIGN.md"""
    rows = re.findall(r"^- `(k_txe_[a-z]+)` — LDS (\d+) B\b", (ROOT / "DESIGN.md").read_text(), re.M)
    assert len(rows) == len(dict(rows)) == len(NAMES), rows
    return {name: int(lds) for name, lds in rows}


def test_the_kernels_are_the_ones_design_lists(kernels, listed):
    assert sorted(k["name"] for k in kernels) == sorted(listed)
    assert set(listed) == NAMES
    text = (ROOT / "simmr_amd" / "csrc" / "taxeval_kernels.hip").read_text()
    assert set(re.findall(r"^(k_[a-z0-9_]+)\(", text, re.M)) == set(listed)


def test_no_scratch_no_agprs_no_spills(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["occupancy"] >= 4, k


def test_lds_is_what_design_states(kernels, listed):
    for k in kernels:
        assert k["lds"] == listed[k["name"]], k
    # and what the tables need: the workgroup scans' words; two counts; seven counts, by_rank's 8 x 5 and the 512 slots of (key, sum);
    # three counts and reads_by_rank's 8 x 5
    assert listed["k_txe_index"] == 256 * 4 and listed["k_txe_scan"] == 256 * 8 and listed["k_txe_heads"] == 256 * 4
    assert listed["k_txe_nodes"] == listed["k_txe_lineage"] == listed["k_txe_look"] == listed["k_txe_rollup"] == 0
    assert listed["k_txe_truth"] == 2 * 4 and listed["k_txe_record"] == (7 + 8 * 5 + 2 * 512) * 4 and listed["k_txe_reduce"] == (3 + 8 * 5) * 4


def test_the_shared_routines_are_taken_not_restated():
    """taxeval_kernels.hip takes the reader, the name table and the search through MEV_ROUTINES_ONLY and defines no copy of them"""
    text = (ROOT / "simmr_amd" / "csrc" / "taxeval_kernels.hip").read_text()
    assert "#define MEV_ROUTINES_ONLY" in text and '#include "mapeval_kernels.hip"' in text
    assert not re.search(r"SIMMR_DEV \w+ (?:mev_|fsam_|sam_)\w+\(", text)
    assert "mev_lower_bound(" in text and "mev_name_row(" in text and "fsam_index_tiles(" in text and "sam_scan_chunks(" in text
    assert (ROOT / "simmr_amd" / "csrc" / "taxeval.hip").read_text().count("samsort_sort_pairs(") >= 2
