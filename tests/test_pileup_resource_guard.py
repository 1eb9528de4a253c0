"""Build-time guard for the allele-count kernels (pileup_kernels.hip), the fifth translation unit of libsimmr_hip.so, in the
manner of tests/test_regions_resource_guard.py: a budget of four kernels of its own, no scratch, no AGPRs, no spills."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="pileup.hip")


def test_pileup_translation_unit_budget(kernels):
    names = sorted(k["name"] for k in kernels)
    assert 0 < len(names) <= 4, names
    for want in ("k_pileup_keys", "k_pileup_add"):
        assert sum(want in n for n in names) == 1, (want, names)


def test_no_scratch_no_agprs_no_spills(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k


def test_the_add_keeps_eight_waves(kernels):
    """the add waits on bisections and scattered atomics: it stays light enough for eight waves per SIMD, and needs no LDS"""
    k = next(k for k in kernels if "k_pileup_add" in k["name"])
    assert k["occupancy"] >= 8 and k["lds"] == 0, k
