"""simmr_amd/csrc/host_support.hpp — the plumbing every host unit of libsimmr_hip.so shares — without a GPU: a stand-alone
program over counting stubs of the HIP calls, built and run under the sanitizers, and the shape the sources keep."""
import os
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "simmr_amd" / "csrc"
UNITS = ("engine.hip", "depth.hip", "strain.hip", "regions.hip", "pileup.hip", "sam.hip", "sam_sort.hip", "overlap.hip", "fit.hip", "fit_sam.hip",
         "bam.hip", "bam_index.hip", "mapeval.hip")


def test_the_support_header_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/host_support_main.cpp: ensure keeps, grows and fails clean; the engine's slack; one owner through moves and swaps and
    inside a vector; Events creates only what is missing; a state deleted through unit_state's hook leaves nothing alive.  The
    exit status is the number of allocations and events still alive."""
    exe = tmp_path / "host_support_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "host_support_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr[-2000:])
    assert re.fullmatch(rb"ok: \d+ allocations, \d+ events, 0 alive\n", r.stdout), r.stdout


def test_one_copy_of_the_plumbing():
    """one DevBuf, one check macro, one sync_check, no unit-private state accessor or destroy hook; frees and event destroys
    outside the header only where the thing freed is neither a DevBuf nor an Events set"""
    files = {f.name: f.read_text() for f in CSRC.iterdir() if f.suffix in (".hip", ".hpp")}
    everything = "\n".join(files.values())
    assert len(re.findall(r"^\s*struct DevBuf\b", everything, re.M)) == 1 and "struct DevBuf {" in files["host_support.hpp"]
    assert re.findall(r"^\s*#\s*define\s+(\w*_TRY)\b", everything, re.M) == ["HIP_TRY"]
    assert len(re.findall(r"^\s*(?:inline\s+)?int \w*sync_check\(", everything, re.M)) == 1
    assert "state_of" not in everything and not re.search(r"\w+_destroy\(void\*", everything)
    for name in UNITS:
        assert '#include "host_support.hpp"' in files[name] or '#include "sam_names.hpp"' in files[name] or \
            '#include "record_stream_host.hpp"' in files[name], name
    assert '#include "host_support.hpp"' in files["sam_names.hpp"] and '#include "sam_names.hpp"' in files["record_stream_host.hpp"]
    outside = {name: len(re.findall(r"\bhipFree\(|\bhipEventDestroy\(", text)) for name, text in files.items() if name != "host_support.hpp"}
    # engine.hip: the first event of a ring pair whose second could not be made; mapeval.hip: its growing list of spans
    assert {k: v for k, v in outside.items() if v} == {"engine.hip": 1, "mapeval.hip": 4}
    for name in ("depth.hip", "pileup.hip", "overlap.hip", "sam_names.hpp"):
        assert "staged_rows(e" in files[name] and "eng_contig_len(" not in files[name], name
    make = (CSRC / "Makefile").read_text()
    assert "host_support.hpp" in re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
