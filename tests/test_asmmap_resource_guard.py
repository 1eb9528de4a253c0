"""Build-time guard for the placement of an assembler's contigs (asmmap_kernels.hip, a translation unit of libsimmr_hip.so of its
own), in the manner of tests/test_asmeval_resource_guard.py: the unit's kernels are exactly the k_amap_* that DESIGN.md section 4
lists, none uses scratch or AGPRs or spills, each keeps eight waves a SIMD, each one's LDS is what DESIGN.md states, and the shared
routines are taken, not restated."""
import re
import sys
from pathlib import Path

import pytest

from tests._scaffold import sorts_through_the_pair_sort

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "simmr_amd" / "csrc"
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="asmmap.hip")


@pytest.fixture(scope="module")
def listed():
    """kernel -> LDS bytes, from the list of DESIGN.md"""
    rows = re.findall(r"^- `(k_amap_[a-z_]+)` — LDS (\d+) B\b", (ROOT / "DESIGN.md").read_text(), re.M)
    assert len(rows) == len(dict(rows)) == 20, rows
    return {name: int(lds) for name, lds in rows}


def test_the_kernels_are_the_ones_design_lists(kernels, listed):
    assert sorted(k["name"] for k in kernels) == sorted(listed)
    text = (CSRC / "asmmap_kernels.hip").read_text()
    assert set(re.findall(r"^(k_[a-z0-9_]+)\(", text, re.M)) == set(listed)
    # only the new files define a k_amap_*
    for path in CSRC.iterdir():
        if path.name not in ("asmmap_kernels.hip", "asmmap.hip") and path.suffix in (".hip", ".hpp"):
            assert not re.search(r"^k_amap_", path.read_text(), re.M), path.name


def test_no_scratch_no_agprs_no_spills(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["occupancy"] >= 8, k


def test_lds_is_what_design_states(kernels, listed):
    for k in kernels:
        assert k["lds"] == listed[k["name"]], k
    # what the tables need: 1024 rows of two 64-bit sums; seven and five 64-bit sums
    assert listed["k_amap_reduce_truth"] == 1024 * 2 * 8 and listed["k_amap_reduce_blocks"] == 7 * 8 and listed["k_amap_reduce_contigs"] == 5 * 8
    assert sum(1 for v in listed.values() if v == 0) == 17


def test_the_shared_routines_are_taken_not_restated():
    text, unit = (CSRC / "asmmap_kernels.hip").read_text(), (CSRC / "asmmap.hip").read_text()
    assert "#define ASM_ROUTINES_ONLY" in text and '#include "asmeval_kernels.hip"' in text
    for t in (text, unit):
        assert not re.search(r"SIMMR_DEV [\w ]+ (?:asm_roll\w*|mev_\w+|fsam_\w+|sam_\w+)\(", t)
    assert "asm_roll_at(" in text and "asm_find(" in text
    assert sorts_through_the_pair_sort("asmmap.hip") and "eng_scan_u32(" in unit and "asm_front_launch(" in unit and "DevBuf" in unit and "Spans<" in unit
    assert "min(24, bit length" in text   # the table's rule is fixed in a comment
    guarded = (CSRC / "asmeval_kernels.hip").read_text()
    assert guarded.index("#ifndef ASM_ROUTINES_ONLY") < guarded.index("k_asm_index(") and guarded.index("SIMMR_DEV void asm_roll(") < guarded.index("#ifndef ASM_ROUTINES_ONLY")
