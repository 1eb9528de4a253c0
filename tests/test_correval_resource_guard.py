"""Build-time guard for the scoring of a read error corrector's output (correval_kernels.hip, a translation unit of libsimmr_hip.so of its
own), in the manner of tests/test_bineval_resource_guard.py: the unit's kernels are exactly the k_cev_* that DESIGN.md section 4 lists,
none uses scratch or AGPRs or spills, each has the waves a SIMD the compiler gave it at the time of the commit, and each one's LDS is
what DESIGN.md states."""
import re
import sys
from pathlib import Path

import pytest

from tests._scaffold import sorts_through_the_pair_sort

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

OCCUPANCY = {"k_cev_truth": 7}  # as tools/resource_usage.py --source correval.hip shows; every other kernel: 8


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="correval.hip")


@pytest.fixture(scope="module")
def listed():
    """kernel -> LDS bytes, from the list of DESIGN.md"""
    rows = re.findall(r"^- `(k_cev_[a-z_]+)` — LDS (\d+) B\b", (ROOT / "DESIGN.md").read_text(), re.M)
    assert len(rows) == len(dict(rows)) == 7, rows
    return {name: int(lds) for name, lds in rows}


def test_the_kernels_are_the_ones_design_lists(kernels, listed):
    assert sorted(k["name"] for k in kernels) == sorted(listed)
    text = (ROOT / "simmr_amd" / "csrc" / "correval_kernels.hip").read_text()
    assert set(re.findall(r"^(k_[a-z0-9_]+)\(", text, re.M)) == set(listed)


def test_no_scratch_no_agprs_no_spills(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["occupancy"] == OCCUPANCY.get(k["name"], 8), k


def test_lds_is_what_design_states(kernels, listed):
    for k in kernels:
        assert k["lds"] == listed[k["name"]], k
    # what the scans need: 256 words of 32 bits for the two indexes, of 64 bits for the scan; the scorer's privatised tables: the 29
    # counts, the cube, by_qual, by_pos and the histogram of the compared lengths, 32 bits a word; the reduce's eight sums
    assert listed["k_cev_index"] == listed["k_cev_lines"] == 256 * 4 and listed["k_cev_scan"] == 256 * 8
    assert listed["k_cev_score"] == 4 * (29 + 125 + 95 * 5 + 512 * 5 + 513) and listed["k_cev_reduce"] == 8 * 4
    assert listed["k_cev_truth"] == listed["k_cev_gather"] == 0


def test_the_shared_routines_are_taken_not_restated():
    text = (ROOT / "simmr_amd" / "csrc" / "correval_kernels.hip").read_text()
    assert "#define OVE_ROUTINES_ONLY" in text and '#include "ovleval_kernels.hip"' in text
    assert not re.search(r"SIMMR_DEV \w+ (?:mev_|fsam_|sam_|ove_)\w+\(", text)
    for taken in ("fsam_index_tiles(", "sam_scan_chunks(", "sam_wg_scan<", "mev_read_line(", "mev_lower_bound(", "fsam_field_number(", "fsam_md_lane(",
                  "fsam_row_sum(", "fsam_row_or(", "sam_row_scan(", "ove_name_key("):
        assert taken in text, taken
    ove = (ROOT / "simmr_amd" / "csrc" / "ovleval_kernels.hip").read_text()
    assert "#ifndef OVE_ROUTINES_ONLY" in ove and ove.index("ove_name_key(const") < ove.index("#ifndef OVE_ROUTINES_ONLY") < ove.index("k_ove_index(")
    unit = (ROOT / "simmr_amd" / "csrc" / "correval.hip").read_text()
    assert sorts_through_the_pair_sort("correval.hip") and '#include "host_support.hpp"' in unit and "Spans<" in unit and "DevBuf " in unit
    assert not re.search(r"struct (DevBuf|Spans)\b", unit)
    make = (ROOT / "simmr_amd" / "csrc" / "Makefile").read_text()
    assert len(re.findall(r"-shared -o \S+ .*\bcorreval\.hip\b", make)) == 2, "both link lines"
