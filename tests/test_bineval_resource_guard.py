"""Build-time guard for the scoring of a binner's bins (bineval_kernels.hip, a translation unit of libsimmr_hip.so of its own), in
the manner of tests/test_asmeval_resource_guard.py: the unit's kernels are exactly the k_bin_* that DESIGN.md section 4 lists, none
uses scratch or AGPRs or spills, each has the waves a SIMD the compiler gave it at the time of the commit, and each one's LDS is what
DESIGN.md states."""
import re
import sys
from pathlib import Path

import pytest

from tests._scaffold import sorts_through_the_pair_sort

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

OCCUPANCY = {"k_bin_cand_write": 7}  # as tools/resource_usage.py --source bineval.hip shows; every other kernel: 8


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="bineval.hip")


@pytest.fixture(scope="module")
def listed():
    """kernel -> LDS bytes, from the list of DESIGN.md"""
    rows = re.findall(r"^- `(k_bin_[a-z_]+)` — LDS (\d+) B\b", (ROOT / "DESIGN.md").read_text(), re.M)
    assert len(rows) == len(dict(rows)) == 18, rows
    return {name: int(lds) for name, lds in rows}


def test_the_kernels_are_the_ones_design_lists(kernels, listed):
    assert sorted(k["name"] for k in kernels) == sorted(listed)
    text = (ROOT / "simmr_amd" / "csrc" / "bineval_kernels.hip").read_text()
    assert set(re.findall(r"^(k_[a-z0-9_]+)\(", text, re.M)) == set(listed)


def test_no_scratch_no_agprs_no_spills(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["occupancy"] == OCCUPANCY.get(k["name"], 8), k


def test_lds_is_what_design_states(kernels, listed):
    for k in kernels:
        assert k["lds"] == listed[k["name"]], k
    # and what the scans need: 256 words of 32 bits for the index, of 64 bits for the others; nothing else uses LDS
    assert listed["k_bin_index"] == 256 * 4
    with_scan = {"k_bin_scan", "k_bin_lines", "k_bin_chunks", "k_bin_truth_write", "k_bin_cand_write"}
    assert all(listed[n] == (256 * 8 if n in with_scan else 0) for n in listed if n != "k_bin_index")


def test_the_shared_routines_are_taken_not_restated():
    text = (ROOT / "simmr_amd" / "csrc" / "bineval_kernels.hip").read_text()
    assert "#define MEV_ROUTINES_ONLY" in text and '#include "mapeval_kernels.hip"' in text
    assert not re.search(r"SIMMR_DEV \w+ (?:mev_|fsam_|sam_)\w+\(", text)
    assert "mev_name_row(" in text and "fsam_index_tiles(" in text and "sam_scan_chunks(" in text and "sam_wg_scan<" in text
    unit = (ROOT / "simmr_amd" / "csrc" / "bineval.hip").read_text()
    assert sorts_through_the_pair_sort("bineval.hip") and "eng_scan_u32(" in unit and '#include "host_support.hpp"' in unit
    assert not re.search(r"struct (DevBuf|Spans)\b", unit)
    make = (ROOT / "simmr_amd" / "csrc" / "Makefile").read_text()
    assert len(re.findall(r"-shared -o \S+ .*\bbineval\.hip\b", make)) == 2, "both link lines"
