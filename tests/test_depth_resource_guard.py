"""Build-time guard for the coverage-depth kernels (depth_kernels.hip), the second translation unit of libsimmr_hip.so, in
the manner of tests/test_stats_resource_guard.py: a budget of six kernels of its own (engine.hip's 85 are asserted there),
no scratch, no AGPRs, and a mark kernel light enough for eight waves per SIMD."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def kernels():
    import resource_usage
    return resource_usage.collect(source="depth.hip")


def test_depth_translation_unit_budget(kernels):
    names = sorted(k["name"] for k in kernels)
    assert 0 < len(names) <= 6, names
    for want in ("k_depth_mark", "k_depth_tile_sums", "k_depth_scan_tiles", "k_depth_apply", "k_depth_summarize"):
        assert sum(want in n for n in names) == 1, (want, names)


def test_no_scratch_no_agprs(kernels):
    for k in kernels:
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k


def test_mark_kernel_occupancy(kernels):
    k = next(k for k in kernels if "k_depth_mark" in k["name"])
    assert k["occupancy"] >= 8 and k["lds"] == 0, k


def test_collect_default_is_the_engine_translation_unit():
    import inspect
    import resource_usage
    assert inspect.signature(resource_usage.collect).parameters["source"].default == "engine.hip"
