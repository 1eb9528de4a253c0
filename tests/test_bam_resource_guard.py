"""The budget of the BAM / BGZF unit (simmr_amd/csrc/bam.hip), as the compiler reports it for gfx950: runs without a GPU."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import resource_usage  # noqa: E402


@pytest.fixture(scope="module")
def kernels():
    return resource_usage.collect(source="bam.hip")


def test_at_most_eight_kernels_all_named_k_bam_or_k_bgzf(kernels):
    names = sorted(k["name"].split("(")[0] for k in kernels)
    assert 1 <= len(names) <= 8 and all(n.startswith(("k_bam_", "k_bgzf_")) for n in names), names
    assert names == ["k_bam_offsets", "k_bam_scan", "k_bam_size", "k_bam_write", "k_bgzf_frame"]


def test_no_scratch_no_agprs_no_vector_spills_four_waves(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0, k
        assert k["occupancy"] >= 4, k


def test_lds_is_what_the_design_states(kernels):
    """the writer has none (the record's words are made in registers), the size pass 16 partial sums, the
    scans their 256 entries, the framing kernel the four CRC tables (4 KiB), the fold's 256 words and the last lane's register"""
    lds = {k["name"].split("(")[0]: k["lds"] for k in kernels}
    assert lds == {"k_bam_write": 0, "k_bam_size": 64, "k_bam_scan": 2048, "k_bam_offsets": 1024, "k_bgzf_frame": 4096 + 1024 + 4}
    design = (ROOT / "DESIGN.md").read_text()
    for needle in ("k_bam_write", "k_bgzf_frame", "5124 bytes"):
        assert needle in design, needle


def test_the_sam_units_keep_their_figures():
    """the record routine is included here without its kernels: k_sam_write stays what it was"""
    ks = {k["name"].split("(")[0]: k for k in resource_usage.collect(source="sam.hip")}
    assert set(ks) == {"k_sam_size", "k_sam_scan", "k_sam_offsets", "k_sam_write"}
    assert (ks["k_sam_write"]["vgpr"], ks["k_sam_write"]["lds"]) == (101, 6400)
