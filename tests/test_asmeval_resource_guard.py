"""Build-time guard for the scoring of an assembler's contigs (asmeval_kernels.hip, a translation unit of libsimmr_hip.so of its
own), in the manner of tests/test_vcfeval_resource_guard.py: the unit's kernels are exactly the k_asm_* that DESIGN.md section 4
lists, none uses scratch or AGPRs or spills, each keeps the eight waves a SIMD it has at the time of the commit, and each one's LDS is
what DESIGN.md states."""
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
    return resource_usage.collect(source="asmeval.hip")


@pytest.fixture(scope="module")
def listed():
    """kernel -> LDS bytes, from the list of DESIGN.md"""
    rows = re.findall(r"^- `(k_asm_[a-z_]+)` — LDS (\d+) B\b", (ROOT / "DESIGN.md").read_text(), re.M)
    assert len(rows) == len(dict(rows)) == 18, rows
    return {name: int(lds) for name, lds in rows}


def test_the_kernels_are_the_ones_design_lists(kernels, listed):
    assert sorted(k["name"] for k in kernels) == sorted(listed)
    text = (ROOT / "simmr_amd" / "csrc" / "asmeval_kernels.hip").read_text()
    assert set(re.findall(r"^(k_[a-z0-9_]+)\(", text, re.M)) == set(listed)


def test_no_scratch_no_agprs_no_spills(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["occupancy"] >= 8, k


def test_lds_is_what_design_states(kernels, listed):
    for k in kernels:
        assert k["lds"] == listed[k["name"]], k
    # and what the tables need: the scans' words, 1024 rows of three 32-bit and of two 64-bit counters with the ten sums
    assert listed["k_asm_index"] == 256 * 4 and listed["k_asm_scan"] == listed["k_asm_lines"] == listed["k_asm_chunks"] == 256 * 8
    assert listed["k_asm_reduce_entries"] == 1024 * 3 * 4 and listed["k_asm_reduce_contigs"] == 1024 * 2 * 8 + 10 * 8
    assert listed["k_asm_roll_truth"] == listed["k_asm_roll_cand"] == listed["k_asm_pack"] == 0


def test_the_shared_routines_are_taken_not_restated():
    text = (ROOT / "simmr_amd" / "csrc" / "asmeval_kernels.hip").read_text()
    assert "#define MEV_ROUTINES_ONLY" in text and '#include "mapeval_kernels.hip"' in text
    assert not re.search(r"SIMMR_DEV \w+ (?:mev_|fsam_|sam_)\w+\(", text)
    assert "mev_name_row(" in text and "fsam_index_tiles(" in text and "sam_scan_chunks(" in text and "sam_wg_scan<" in text
    unit = (ROOT / "simmr_amd" / "csrc" / "asmeval.hip").read_text()
    assert sorts_through_the_pair_sort("asmeval.hip") and "eng_scan_u32(" in unit
    assert "min(24, bit length" in text   # the table's rule is fixed in a comment
