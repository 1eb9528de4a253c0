"""CPU-only checks of the BAM surface: the plain-Python record and reader (tests/_bam.py) against the SAM model, reg2bin at its
level edges, the header writer, the end-of-file block, the new symbols, the build, the option on the command line, and the host
tables of the BGZF CRC in a stand-alone program under the sanitizers."""
import ctypes as C
import gzip
import re
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from simmr_amd.sam import BGZF_EOF, bam_header, sam_header
from tests import _bam, _oracle, _sam, _synth, _truth
from tests._hand_built import hand_built

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"
CSRC = ROOT / "simmr_amd" / "csrc"
NAMES = ("simmr_bam_plan", "simmr_bam_emit", "simmr_last_bam_ms", "simmr_bgzf_frame")


@pytest.fixture(scope="module")
def genomes():
    rng = np.random.default_rng(21)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30000)].copy()
    seq[rng.integers(0, 30000, 3000)] = ord("N")
    seq[rng.integers(0, 30000, 500)] = ord("-")
    seq[12_000:12_400] = ord("N")
    return {1: _oracle.HostGenome(_synth.synthetic_contigs([300_000, 90_001, 30_017, 70_000, 123_457], 7)), 3: _oracle.HostGenome([seq])}


def rnames_of(genomes):
    return [(g, [f"g{g}.c{c}|x" for c in range(len(genomes[g].contigs))]) for g in sorted(genomes)]


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "unpaired"])
def test_the_model_read_back_is_the_sam_model(oracle, genomes, paired):
    """forward and reverse, lengths 0 .. 513 on both sides of the packing's and the windows' edges, N and '-' in the reference"""
    _, o = hand_built(oracle, genomes, 0, "cpu", np.random.default_rng(5))
    t = _truth.model(oracle, o, genomes)
    rn = rnames_of(genomes)
    names = {(g, c): name for g, ns in rn for c, name in enumerate(ns)}
    refs = [(name, len(genomes[g].contigs[c])) for g, ns in rn for c, name in enumerate(ns)]
    want = _sam.sam_text(o, t, names, paired).decode("latin-1").splitlines(keepends=True)
    recs = _bam.parse_records(_bam.bam_records(o, t, rn, paired))
    assert len(recs) == len(want) == len(o["start"])
    assert [_bam.to_sam_line(r, refs) for r in recs] == want
    assert {len(r["seq"]) for r in recs} >= {0, 1, 15, 16, 17, 511, 512, 513} and {r["flag"] & 16 for r in recs} == {0, 16}
    assert any("N" in r["seq"] for r in recs) and max(r["tags"]["NM"][1] for r in recs) >= 73
    # the whole stream: header, references, records
    head = bam_header([n for n, _ in refs], [l for _, l in refs])
    text, refs2, recs2 = _bam.parse_bam(head + _bam.bam_records(o, t, rn, paired))
    assert text == sam_header([n for n, _ in refs], [l for _, l in refs]) and refs2 == refs and recs2 == recs


def test_a_record_written_by_hand():
    """one reverse read of three bases, unpaired, with one edit: every byte"""
    o = {"start": np.array([9], np.uint64), "end": np.array([6], np.uint64), "contig": np.zeros(1, np.uint32), "genome": np.array([2], np.uint32),
         "read_id": np.array([41], np.uint32), "flags": np.array([1], np.uint8), "seq_off": np.array([0, 3], np.uint64),
         "seq": np.frombuffer(b"AC-", np.uint8), "qual": np.frombuffer(b"!5I", np.uint8)}
    t = {"edit_off": np.array([0, 1], np.uint64), "edit_pos": np.array([0], np.uint32), "edit_ref": np.frombuffer(b"G", np.uint8)}
    # forward strand: SEQ = revcomp("AC-") with '-' shown as N = N G T; QUAL reversed; the edit at forward offset 2 over C (G complemented)
    body = struct.pack("<iiBBHHHiiii", 1, 6, 3, 255, 4681, 1, 16, 3, -1, -1, 0) + b"41\0" + struct.pack("<I", 3 << 4) + bytes([0xf4, 0x80]) + \
        bytes([40, 20, 0]) + b"NMC\x01" + b"MDZ2C0\0"
    assert _bam.bam_records(o, t, [(0, ["a"]), (2, ["b"])], False) == struct.pack("<i", len(body)) + body


def test_reg2bin_at_the_level_edges():
    assert _bam.reg2bin(0, 1) == 4681 and _bam.reg2bin(0, 1 << 14) == 4681 and _bam.reg2bin(0, (1 << 14) + 1) == 585
    assert _bam.reg2bin((1 << 14) - 1, (1 << 14) + 1) == 585 and _bam.reg2bin(1 << 14, (1 << 14) + 1) == 4682
    assert _bam.reg2bin(0, (1 << 17) + 1) == 73 and _bam.reg2bin(0, (1 << 20) + 1) == 9 and _bam.reg2bin(0, (1 << 23) + 1) == 1
    assert _bam.reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0 and _bam.reg2bin(1 << 26, (1 << 26) + 1) == 4681 + (1 << 12)
    assert _bam.reg2bin((1 << 29) - 1, 1 << 29) == 37448  # the last bin of the scheme


def test_header_writer_round_trips_and_refuses():
    rn, ln = ["chr1", "plasmid|2", "x=*"], [1000, 2 ** 31 - 1, 0]
    for order in ("unsorted", "coordinate"):
        text, refs, recs = _bam.parse_bam(bam_header(rn, ln, order))
        assert text == sam_header(rn, ln, order) and refs == list(zip(rn, ln)) and recs == []
    assert bam_header([], []) == b"BAM\1" + struct.pack("<i", len(sam_header([], []))) + sam_header([], []).encode() + struct.pack("<i", 0)
    for bad in (["a", "a"], ["has space"], ["=x"], ["*"], [""], ["x" * 255]):
        with pytest.raises(ValueError):
            bam_header(bad, [1] * len(bad))
    for bad_len in (2 ** 31, 2 ** 33):
        with pytest.raises(ValueError):
            bam_header(["a"], [bad_len])
    with pytest.raises(ValueError):
        bam_header(["a"], [1], "queryname")


def test_the_end_of_file_block():
    assert gzip.decompress(BGZF_EOF) == b"" and len(BGZF_EOF) == 28 and BGZF_EOF == _bam.BGZF_EOF
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lit = re.search(r'^#define SIMMR_BGZF_EOF "((?:\\x[0-9a-f]{2})+)"', header, re.M).group(1)
    assert bytes.fromhex(lit.replace("\\x", "")) == BGZF_EOF and "#define SIMMR_BGZF_EOF_BYTES 28" in header
    # the model's own framing, read by the standard library
    data = bytes(range(256)) * 600
    framed = _bam.bgzf_frame(data)
    assert len(framed) == _bam.bgzf_bound(len(data)) and b"".join(_bam.bgzf_blocks(framed)) == data
    assert gzip.decompress(framed + BGZF_EOF) == data


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, re.M) and name in _abi.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"^uint64_t simmr_bgzf_bound\(", header, re.M) and "simmr_bgzf_bound" in _abi.SYMBOLS
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)]).decode()
    assert "simmr_bam_emit" in dyn and "simmr_bgzf_frame" in dyn and "eng_ext_slot" not in dyn and "k_bam_write" in dyn and "k_bgzf_frame" in dyn
    assert "SIMMR_ABI_VERSION 1" in header
    for n in (0, 1, 65279, 65280, 65281, 2 * 65280, 2 * 65280 + 7, 10 ** 12):
        assert lib.simmr_bgzf_bound(n) == _bam.bgzf_bound(n) == n + 31 * -(-n // 65280)


def test_the_unit_is_built_and_has_its_slot():
    make = (CSRC / "Makefile").read_text()
    assert make.count("bam.hip fit_sam.hip fit.hip overlap.hip sam_sort.hip sam.hip pileup.hip engine.hip depth.hip strain.hip regions.hip\n") == 2
    srcs = re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
    assert {"bam.hip", "bam_kernels.hip", "bgzf_tables.hpp"} <= set(srcs)
    internal = (CSRC / "engine_internal.hpp").read_text()
    assert "ENG_EXT_BAM = 9," in internal and "ENG_EXT_COUNT = 12" in internal
    unit = (CSRC / "bam.hip").read_text()
    assert "unit_state<BamState, ENG_EXT_BAM>" in unit and '#include "engine.hip"' not in unit and '#include "kernels.hip"' not in unit
    k = (CSRC / "bam_kernels.hip").read_text()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(BGZF_\w+)\s+(\d+)u?\b", k, re.M)}
    assert defines["BGZF_BLOCK"] == 0xff00 and defines["BGZF_SEG"] * (defines["BGZF_LANES"] - 1) == defines["BGZF_BLOCK"]
    assert "#define SAM_ROUTINES_ONLY" in k and "bam_record<false>" in k and "bam_record<true>" in k
    # one routine behind the sizes and the bytes: both kernels go through the policy that names it
    assert "rec_size_chunks<BamRec>" in k and "rec_write_places<BamRec, false>" in k


def test_bam_calls_need_an_engine():
    lib = _abi.load()
    ms, total = C.c_float(), C.c_uint64()
    names, reads, truth = _abi.SamNames(0, None, None, None), _abi.ReadsOut(), _abi.TruthOut()
    assert lib.simmr_bam_plan(None, C.byref(names), C.byref(reads), C.byref(truth), 0, 0, C.byref(total)) == _abi.EINVAL
    assert lib.simmr_bam_emit(None, C.byref(reads), C.byref(truth), None, 0) == _abi.EINVAL
    assert lib.simmr_last_bam_ms(None, C.byref(ms)) == _abi.EINVAL
    assert lib.simmr_bgzf_frame(None, None, 0, None, 0, C.byref(total)) == _abi.EINVAL


# (pattern, length, zlib.crc32): pattern 0 is zeros, 1 is 0xff, 2 is byte i = (131 i + 7 + 29 (i >> 8)) & 0xff
CRC_VECTORS = [(2, 1, 0x4c667a2e), (2, 15, 0xa4762116), (2, 16, 0xea7e5b68), (2, 17, 0x293cddb3), (2, 255, 0x17ad3b28), (2, 256, 0x0d75ad75),
               (2, 257, 0xce63fb42), (2, 65279, 0xdba6a6c5), (2, 65280, 0xafded79a), (0, 65280, 0xfed3d2c7), (1, 65280, 0xf6f1c172),
               (1, 300, 0x1c0a1881), (0, 1, 0xd202ef8d)]


def _pattern(p, n):
    return bytes(n) if p == 0 else b"\xff" * n if p == 1 else bytes((131 * i + 7 + 29 * (i >> 8)) & 0xff for i in range(n))


def test_crc_tables_and_fold_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """the host tables of k_bgzf_frame and the fold as a CPU runs it, lane by lane: the vectors above, and every kind of length
    (whole segments, a segment and some, fewer bytes than a segment, fewer than 16) against zlib"""
    for p, n, crc in CRC_VECTORS:
        assert zlib.crc32(_pattern(p, n)) == crc  # (the vectors are zlib's)
    exe = tmp_path / "bgzf_fold_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "bgzf_fold_main.cpp")])
    more = [(p, n) for p in (0, 1, 2) for n in (2, 3, 4, 5, 31, 32, 33, 511, 512, 513, 4095, 4096, 4097, 32768, 65023, 65024, 65025, 65265)]
    cases = [(p, n) for p, n, _ in CRC_VECTORS] + more
    text = f"{len(cases)}\n" + "".join(f"{p} {n}\n" for p, n in cases)
    r = subprocess.run([str(exe)], input=text.encode(), capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    got = [int(x, 16) for x in r.stdout.split()]
    assert got[:len(CRC_VECTORS)] == [crc for _, _, crc in CRC_VECTORS]
    assert got[len(CRC_VECTORS):] == [zlib.crc32(_pattern(p, n)) for p, n in more]


@pytest.fixture(scope="module")
def host_exe():
    subprocess.check_call(["make", "-s", "-C", str(HOST)])
    return str(HOST / "simmr-hip")


USAGE_ROWS = [
    (["--bam"], 2, "error: a value is required for '--bam'"),
    (["--bam="], 2, "error: a file name is required for '--bam'"),
    (["--genome", "a.fna", "--bam", "x.bam"], 2, "error: --output is required"),
    (["--genome", "a.fna", "--output", "x.fq", "--bam", "x.bam", "--devices", "0,1"], 1, "ERROR simmr-hip: --bam does not combine with --devices: use --device"),
    # the refusals that were there come first
    (["--genome", "a.fna", "--output", "x.fq", "--sam", "x.sam", "--bam", "x.bam", "--devices", "0,1"], 1,
     "ERROR simmr-hip: --sam does not combine with --devices: use --device"),
    (["--fit-from-sam", "x.sam", "--fit-model", "m", "--bam", "x.bam"], 2, None),
]


@pytest.mark.parametrize("argv,status,line", USAGE_ROWS, ids=[" ".join(r[0]) for r in USAGE_ROWS])
def test_cli_usage_rows(host_exe, argv, status, line):
    r = subprocess.run([host_exe] + argv, capture_output=True, text=True)
    assert r.returncode == status, r.stderr
    if line is None:
        assert "--fit-from-sam runs no simulation" in r.stderr and "'--bam' given" in r.stderr
    else:
        assert r.stderr.splitlines()[0] == line


def test_help_describes_the_flag(host_exe):
    helptext = subprocess.check_output([host_exe, "--help"]).decode()
    row = helptext.split("--bam <FILE>")[1].split("--overlaps <FILE>")[0]
    assert "not compressed" in row and "samtools sort" in row and "not with --devices" in row and "read order" in row


def test_illegal_rnames_end_the_run_before_any_device_work(host_exe, tmp_path):
    (tmp_path / "c.fna").write_text(">fine\nACGT\n>=odd name\nACGT\n")
    r = subprocess.run([host_exe, "--genome", str(tmp_path / "c.fna"), "--output", str(tmp_path / "x.fq"), "--bam", str(tmp_path / "x.bam")],
                       capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.splitlines() == [
        f"ERROR simmr-hip: --bam: sequence '=odd name' of {tmp_path}/c.fna gets the RNAME '=odd', which is not a SAM reference name"]
    assert not (tmp_path / "x.bam").exists() and not (tmp_path / "x.fq").exists()
