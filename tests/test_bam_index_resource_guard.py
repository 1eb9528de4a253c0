"""The budget of the sorted-BAM / BAI unit (simmr_amd/csrc/bam_index.hip), as the compiler reports it for gfx950: runs without
a GPU."""
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import resource_usage  # noqa: E402

LDS = {"k_bamsort_size": 0, "k_bamsort_gather": 1024, "k_bamsort_scan": 2048, "k_bamsort_offsets": 1024, "k_bamsort_write": 0,
       "k_bai_check": 1024, "k_bai_count": 1024, "k_bai_scan": 2048, "k_bai_compact": 1024, "k_bai_refs": 0, "k_bai_layout": 2048,
       "k_bai_windows": 0, "k_bai_write_chunks": 0, "k_bai_write_refs": 1024}


@pytest.fixture(scope="module")
def kernels():
    return resource_usage.collect(source="bam_index.hip")


def test_the_kernels_are_those_the_design_lists(kernels):
    names = sorted(k["name"].split("(")[0] for k in kernels)
    assert all(n.startswith(("k_bamsort_", "k_bai_")) for n in names), names
    assert names == sorted(LDS)
    design = (ROOT / "DESIGN.md").read_text()
    listed = set(re.findall(r"\b(k_bamsort_\w+|k_bai_\w+)\b", design))
    assert listed == set(names), listed ^ set(names)


def test_no_scratch_no_agprs_no_vector_spills_four_waves(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0, k
        assert k["occupancy"] >= 4, k


def test_lds_is_what_the_design_states(kernels):
    assert {k["name"].split("(")[0]: k["lds"] for k in kernels} == LDS
    design = (ROOT / "DESIGN.md").read_text()
    for name, lds in LDS.items():
        assert re.search(rf"^\| `{name}` \|[^|\n]*\| {lds} \|", design, re.M), (name, lds)  # the table's row: kernel, work, LDS bytes


def test_the_units_whose_routines_are_included_keep_their_kernels():
    assert sorted(k["name"].split("(")[0] for k in resource_usage.collect(source="bam.hip")) == \
        ["k_bam_offsets", "k_bam_scan", "k_bam_size", "k_bam_write", "k_bgzf_frame"]
    assert {k["name"].split("(")[0] for k in resource_usage.collect(source="sam.hip")} == {"k_sam_size", "k_sam_scan", "k_sam_offsets", "k_sam_write"}
