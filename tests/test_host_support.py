"""simmr_amd/csrc/host_support.hpp — the plumbing every host unit of libsimmr_hip.so shares — and scorer_host.hpp — the scaffold
of the scorer units over it — without a GPU: a stand-alone program over counting stubs of the HIP calls, built and run under the
sanitizers, and the shape the sources keep."""
import os
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "simmr_amd" / "csrc"
UNITS = ("engine.hip", "truth.hip", "stats.hip", "depth.hip", "strain.hip", "regions.hip", "pileup.hip", "sam.hip", "sam_sort.hip", "overlap.hip", "fit.hip", "fit_sam.hip",
         "bam.hip", "bam_index.hip", "mapeval.hip", "ovleval.hip", "vcfeval.hip", "taxeval.hip", "asmeval.hip", "bineval.hip", "correval.hip", "asmmap.hip")
SCORERS = UNITS[-8:]


def test_the_support_header_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/host_support_main.cpp: ensure keeps, grows and fails clean; the engine's slack; one owner through moves and swaps and
    inside a vector; Events creates only what is missing; Spans adds up exactly the spans that are marked; a state deleted
    through unit_state's hook leaves nothing alive.  Of scorer_host.hpp, what stands without a unit's kernels: bits_of and the grids at
    their edges; grow_zero; check_add_text's three refusals in their order, to the byte; FoldedSpans (two adds are one span, a fold adds
    the marked spans once and closes them, a begin after it opens a new one, a failed launch leaves the span as it was, reset zeroes
    the sum); sorted_names (the refusals' texts, a name given twice, a prefix first, bytes from 128 on as unsigned, the order that
    std::sort gave the units before, the order array, the blob's eight zero bytes) and DeviceNames; the rooms of LineIndex and
    PairSort; scorer_create and scorer_destroy.  The exit status is the number of allocations and events still alive."""
    exe = tmp_path / "host_support_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "host_support_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr[-2000:])
    assert re.fullmatch(rb"ok: \d+ allocations, \d+ events, 0 alive\n", r.stdout), r.stdout


def test_one_copy_of_the_plumbing():
    """one DevBuf, one check macro, one sync_check, one Spans, no unit-private state accessor or destroy hook; frees and event
    destroys outside the header only where the thing freed is neither a DevBuf nor an Events set; elapsed times read outside the
    header only where the pair is not a unit's span; truth and statistics keep nothing in the engine"""
    files = {f.name: f.read_text() for f in CSRC.iterdir() if f.suffix in (".hip", ".hpp")}
    everything = "\n".join(files.values())
    assert len(re.findall(r"^\s*struct DevBuf\b", everything, re.M)) == 1 and "struct DevBuf {" in files["host_support.hpp"]
    assert len(re.findall(r"^\s*(?:template\s*<[^>]*>\s*)?struct Spans\b", everything, re.M)) == 1 and "struct Spans {" in files["host_support.hpp"]
    assert re.findall(r"^\s*#\s*define\s+(\w*_TRY)\b", everything, re.M) == ["HIP_TRY"]
    assert len(re.findall(r"^\s*(?:inline\s+)?int \w*sync_check\(", everything, re.M)) == 1
    assert "state_of" not in everything and not re.search(r"\w+_destroy\(void\*", everything)
    for name in UNITS:
        assert '#include "host_support.hpp"' in files[name] or '#include "sam_names.hpp"' in files[name] or \
            '#include "record_stream_host.hpp"' in files[name] or '#include "truth_host.hpp"' in files[name], name
    assert '#include "host_support.hpp"' in files["truth_host.hpp"]
    assert '#include "host_support.hpp"' in files["sam_names.hpp"] and '#include "sam_names.hpp"' in files["record_stream_host.hpp"]
    outside = {name: len(re.findall(r"\bhipFree\(|\bhipEventDestroy\(", text)) for name, text in files.items() if name != "host_support.hpp"}
    # engine.hip: the first event of a ring pair whose second could not be made; mapeval.hip: its growing list of spans
    assert {k: v for k, v in outside.items() if v} == {"engine.hip": 1, "mapeval.hip": 4}
    elapsed = {name: len(re.findall(r"\bhipEventElapsedTime\(", text)) for name, text in files.items() if name != "host_support.hpp"}
    # engine.hip: the plan's, the FASTQ plan's and the emit's pairs and the ring of emits, none of them a unit's span;
    # overlap.hip: an emit call, measured call by call into a sum; mapeval.hip: its growing list of spans
    assert {k: v for k, v in elapsed.items() if v} == {"engine.hip": 4, "overlap.hip": 1, "mapeval.hip": 2}
    assert len(re.findall(r"\bhipEventElapsedTime\(", files["host_support.hpp"])) == 1
    assert not re.search(r"\b(?:tr|st)_(?:nm|off|err|ev|ready|emitted|reads|edits|seq|seq_off|slot|tab|timed)\b", files["engine.hip"])
    assert "truth_kernels.hip" not in files["engine.hip"] and "stats_kernels.hip" not in files["engine.hip"]
    for name in ("depth.hip", "pileup.hip", "overlap.hip", "sam_names.hpp"):
        assert "staged_rows(e" in files[name] and "eng_contig_len(" not in files[name], name
    # the scorers' scaffold: one copy of what they share, in scorer_host.hpp, and none left in a unit
    scaffold = files["scorer_host.hpp"]
    assert '#include "host_support.hpp"' in scaffold and "__global__" not in scaffold and "__device__" not in scaffold
    for name in SCORERS + ("bam_index.hip", "sam_sort.hip"):
        assert '#include "scorer_host.hpp"' in files[name], name

    def defined(fn):
        return [name for name, text in files.items() if re.search(r"^(?:template\s*<[^>]*>\s*)?(?:inline\s+)?[\w:]+[\s*&]+%s\(" % fn, text, re.M)]
    for fn in ("bits_of", "grow_zero", "check_add_text", "sorted_names", "scorer_create", "scorer_destroy"):
        assert defined(fn) == ["scorer_host.hpp"], fn
    assert sorted(defined("grid_for")) == ["asmmap.hip", "engine.hip", "scorer_host.hpp"]  # asmmap's: under SIMMR_ASMMAP_MAX_WGS; the engine's: blocks of a count
    for fn in ("check_text", "fold_spans", "sort_room"):
        assert defined(fn) == [], fn
    assert defined("begin_span") == defined("end_span") == ["mapeval.hip"]  # its growing list of per-add spans
    for struct in ("FoldedSpans", "LineIndex", "PairSort", "DeviceNames"):
        assert len(re.findall(r"^\s*(?:template\s*<[^>]*>\s*)?struct %s\b" % struct, everything, re.M)) == 1 and "struct %s {" % struct in scaffold
    for once in ("new (std::nothrow)", "blob.resize(blob.size() + 8"):
        assert [name for name, text in files.items() if once in text] == ["scorer_host.hpp"], once
    for name in SCORERS:
        assert re.search(r"^int simmr_\w+_create\(simmr_engine\* e, simmr_\w+\*\* out\) \{", files[name], re.M), name  # the entry points stay in their units
    make = (CSRC / "Makefile").read_text()
    assert "scorer_host.hpp" in re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
    assert "host_support.hpp" in re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
