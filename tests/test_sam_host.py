"""CPU-only checks of the SAM surface: the plain-Python record (tests/_sam.py) pinned by a case written by hand and read back
through MD, the struct as gcc lays it out against _abi, the new symbols in the library, the header writers of Python and of
libsimmr_host.so, and the option on the command line."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import _abi
from simmr_amd.sam import rname_of, sam_header
from tests import _sam

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"
NAMES = ("simmr_sam_plan", "simmr_sam_emit", "simmr_last_sam_ms")

# one contig of 40 bases with an N at position 12; a forward mate at 2..22 and its reverse mate at 10..30
GENOME = "ACGTACGTACGTNCGTACGTTTGACCAGTAGGCATCGATCG"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def hand_case():
    """edits at offsets 0 and L - 1, two adjacent edits and an N in the reference, on both strands"""
    fwd_ref = GENOME[2:22]                                    # GTACGTACGTNCGTACGTTT
    fwd = list(fwd_ref)
    fwd_edits = ((0, "T"), (5, "A"), (6, "G"), (10, "A"), (19, "C"))  # offset 0, adjacent 5 and 6, the reference's N, offset L - 1
    for j, ch in fwd_edits:
        assert fwd[j] != ch
        fwd[j] = ch
    rev_ref = "".join(COMP[c] for c in reversed(GENOME[10:30]))  # the reverse mate as written
    rev = list(rev_ref)
    assert rev_ref == "TACTGGTCAAACGTACGNAC"
    rev_edits = ((0, "A"), (8, "C"), (9, "G"), (17, "T"), (19, "T"))
    for j, ch in rev_edits:
        assert rev[j] != ch
        rev[j] = ch
    seq = "".join(fwd) + "".join(rev)
    qual = "".join(chr(33 + i) for i in range(40))
    o = {"start": np.array([2, 30], np.uint64), "end": np.array([22, 10], np.uint64), "contig": np.zeros(2, np.uint32),
         "genome": np.zeros(2, np.uint32), "read_id": np.array([7, 7], np.uint32), "flags": np.array([0, 1], np.uint8),
         "seq_off": np.array([0, 20, 40], np.uint64), "seq": np.frombuffer(seq.encode(), np.uint8), "qual": np.frombuffer(qual.encode(), np.uint8)}
    pos = [j for j, _ in fwd_edits] + [j for j, _ in rev_edits]
    ref = [fwd_ref[j] for j, _ in fwd_edits] + [rev_ref[j] for j, _ in rev_edits]
    t = {"edit_off": np.array([0, 5, 10], np.uint64), "edit_pos": np.array(pos, np.uint32), "edit_ref": np.frombuffer("".join(ref).encode(), np.uint8)}
    return o, t


def test_hand_written_pair():
    o, t = hand_case()
    lines = _sam.sam_text(o, t, {(0, 0): "chr1"}, True).decode().splitlines(keepends=True)
    q = "".join(chr(33 + i) for i in range(40))
    want = [
        "7\t99\tchr1\t3\t255\t20M\t=\t11\t28\tTTACGAGCGTACGTACGTTC\t" + q[:20] + "\tNM:i:5\tMD:Z:0G4T0A3N8T0\n",
        # the reverse mate as written is revcomp(GENOME[10:30]) = TACTGGTCAAACGTACGNAC with offsets 0, 8, 9, 17 and 19 altered: on
        # the forward strand the alterations sit at 19, 11, 10, 2 and 0, over the genome's A, T, T, N and G
        "7\t147\tchr1\t11\t255\t20M\t=\t3\t-28\tATACGTACGTCGGACCAGTT\t" + q[20:][::-1] + "\tNM:i:5\tMD:Z:0G1N7T0T7A0\n",
    ]
    g = GENOME[10:30]
    assert (g[0], g[2], g[10], g[11], g[19]) == ("G", "N", "T", "T", "A")
    assert lines[0] == want[0]
    assert lines[1] == want[1]
    # unpaired: the flag and the mate fields change, nothing else
    single = _sam.sam_text(o, t, {(0, 0): "chr1"}, False).decode().splitlines()
    assert single[0].split("\t")[:9] == ["7", "0", "chr1", "3", "255", "20M", "*", "0", "0"]
    assert single[1].split("\t")[:9] == ["7", "16", "chr1", "11", "255", "20M", "*", "0", "0"]
    assert single[1].split("\t")[9:] == want[1].rstrip("\n").split("\t")[9:]


def test_a_read_without_bases_and_a_tie():
    o = {"start": np.array([5, 5], np.uint64), "end": np.array([5, 5], np.uint64), "contig": np.zeros(2, np.uint32), "genome": np.zeros(2, np.uint32),
         "read_id": np.array([0, 0], np.uint32), "flags": np.array([0, 1], np.uint8), "seq_off": np.zeros(3, np.uint64),
         "seq": np.zeros(0, np.uint8), "qual": np.zeros(0, np.uint8)}
    t = {"edit_off": np.zeros(3, np.uint64), "edit_pos": np.zeros(0, np.uint32), "edit_ref": np.zeros(0, np.uint8)}
    assert _sam.sam_text(o, t, {(0, 0): "c"}, True) == (b"0\t99\tc\t6\t255\t*\t=\t6\t0\t*\t*\tNM:i:0\tMD:Z:0\n"
                                                         b"0\t147\tc\t6\t255\t*\t=\t6\t0\t*\t*\tNM:i:0\tMD:Z:0\n")


def test_reference_rebuilt_from_seq_and_md_is_the_genome():
    """the second reading: for every record, SEQ with MD's bases put back is the genome slice at POS ('-' shown as N)"""
    o, t = hand_case()
    for line in _sam.sam_text(o, t, {(0, 0): "chr1"}, True).decode().splitlines():
        f = _sam.parse(line)
        assert _sam.reference_from(f["seq"], f["md"]) == GENOME[f["pos"] - 1: f["pos"] - 1 + len(f["seq"])]
        assert f["nm"] == sum(c.isalpha() for c in f["md"]) and f["cigar"] == "%dM" % len(f["seq"])
    # random reads over a genome with N and '-': edits drawn at random, the truth columns built by comparing
    rng = np.random.default_rng(3)
    genome = np.frombuffer(b"ACGTN-", np.uint8)[rng.choice(6, 5000, p=[.23, .23, .23, .23, .05, .03])]
    gs = bytes(genome).decode()
    comp = {**COMP, "-": "-"}
    starts, ends, flags, seqs, pos, ref, eoff = [], [], [], [], [], [], [0]
    for r in range(300):
        L = int(rng.integers(0, 70))
        lo = int(rng.integers(0, 5000 - L))
        rev = int(rng.integers(0, 2))
        want = gs[lo:lo + L]
        if rev:
            want = "".join(comp[c] for c in reversed(want))
        have = list(want)
        for j in np.flatnonzero(rng.random(L) < 0.15):
            have[j] = "ACGT"[("ACGT".find(want[j]) + 1) % 4] if want[j] in "ACGT" else "A"
        d = [j for j in range(L) if have[j] != want[j]]
        pos += d; ref += [want[j] for j in d]; eoff.append(eoff[-1] + len(d))
        starts.append(lo + L if rev else lo); ends.append(lo if rev else lo + L); flags.append(rev); seqs.append("".join(have))
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    o = {"start": np.array(starts, np.uint64), "end": np.array(ends, np.uint64), "contig": np.zeros(300, np.uint32), "genome": np.zeros(300, np.uint32),
         "read_id": np.arange(300, dtype=np.uint32) // 2, "flags": np.array(flags, np.uint8), "seq_off": off,
         "seq": np.frombuffer("".join(seqs).encode(), np.uint8), "qual": np.full(int(off[-1]), 40 + 33, np.uint8)}
    t = {"edit_off": np.array(eoff, np.uint64), "edit_pos": np.array(pos, np.uint32), "edit_ref": np.frombuffer("".join(ref).encode(), np.uint8)}
    shown = gs.replace("-", "N")
    n_rev_edits = 0
    for r, line in enumerate(_sam.sam_text(o, t, {(0, 0): "g"}, True).decode().splitlines()):
        f = _sam.parse(line)
        L = 0 if f["seq"] == "*" else len(f["seq"])
        assert _sam.reference_from(f["seq"], f["md"]) == shown[f["pos"] - 1: f["pos"] - 1 + L], r
        assert f["nm"] == eoff[r + 1] - eoff[r] == sum(c.isalpha() for c in f["md"])
        n_rev_edits += f["nm"] if f["flag"] & 16 else 0
        m = _sam.parse(_sam.record(o, t, {(0, 0): "g"}, r ^ 1, True))
        assert f["rnext"] == "=" and f["pnext"] == m["pos"] and f["tlen"] == -m["tlen"]
    assert n_rev_edits > 100


def test_struct_layout_matches_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "simmr_hip.h"\nint main(void){\n'
    src += ' printf("%zu ", sizeof(simmr_sam_names));\n'
    want = [C.sizeof(_abi.SamNames)]
    for f, _ in _abi.SamNames._fields_:
        src += f' printf("%zu %zu ", offsetof(simmr_sam_names, {f}), sizeof(((simmr_sam_names*)0)->{f}));\n'
        want += [getattr(_abi.SamNames, f).offset, getattr(_abi.SamNames, f).size]
    src += ' printf("%d", SIMMR_ABI_VERSION); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "t.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/t", f"{d}/t.c"])
        got = list(map(int, subprocess.check_output([f"{d}/t"]).decode().split()))
    assert got == want + [1]  # (the change only adds symbols: the ABI version stays)
    assert [f for f, _ in _abi.SamNames._fields_] == ["n_genomes", "genome_idx", "n_contigs", "rname"]


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "simmr_hip.h").read_text()
    lib = _abi.load()
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, re.M) and name in _abi.SYMBOLS and hasattr(lib, name), name
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)]).decode()
    assert "simmr_sam_emit" in dyn and "eng_ext_slot" not in dyn and "k_sam_write" in dyn


def test_sam_calls_need_an_engine():
    lib = _abi.load()
    ms, total = C.c_float(), C.c_uint64()
    names, reads, truth = _abi.SamNames(0, None, None, None), _abi.ReadsOut(), _abi.TruthOut()
    assert lib.simmr_sam_plan(None, C.byref(names), C.byref(reads), C.byref(truth), 0, 0, C.byref(total)) == _abi.EINVAL
    assert lib.simmr_sam_emit(None, C.byref(reads), C.byref(truth), None, 0) == _abi.EINVAL
    assert lib.simmr_last_sam_ms(None, C.byref(ms)) == _abi.EINVAL


def test_kernel_constants():
    k = (ROOT / "simmr_amd" / "csrc" / "sam_kernels.hip").read_text()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(SAM_\w+)\s+(\d+)u?\b", k, re.M)}
    assert defines["SAM_LANES"] * defines["SAM_WG_READS"] == 256 and defines["SAM_CHUNK"] % defines["SAM_WG_READS"] == 0
    assert defines["SAM_CHUNK"] == 4 * 256  # k_sam_offsets: four reads per thread
    assert defines["SAM_WGS_PER_CU"] >= 1


def test_header_writer():
    assert sam_header(["chr1", "plasmid|2"], [1000, 2**33]) == ("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:plasmid|2\tLN:8589934592\n"
                                                                "@PG\tID:simmr-hip\tPN:simmr-hip\n")
    assert rname_of("NC_000913.3 Escherichia coli K-12") == "NC_000913.3" and rname_of("a\tb") == "a"
    for bad in (["a", "a"], ["has space"], ["=x"], ["*"], [""], ["x" * 255]):
        with pytest.raises(ValueError):
            sam_header(bad, [1] * len(bad))
    assert sam_header(["x=*"], [1]).count("@SQ") == 1


@pytest.fixture(scope="module")
def host_lib():
    subprocess.check_call(["make", "-s", "-C", str(HOST)])
    lib = C.CDLL(str(HOST / "libsimmr_host.so"))
    lib.simmr_host_sam_header.restype = C.c_void_p
    lib.simmr_host_sam_header.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p]
    lib.simmr_host_sam_rname.restype = C.c_void_p
    lib.simmr_host_sam_rname.argtypes = [C.c_char_p]
    lib.simmr_host_free.argtypes = [C.c_void_p]
    return lib


def host_header(lib, rnames, lengths):
    lens = np.array(lengths, dtype=np.uint64)
    p = lib.simmr_host_sam_header(len(rnames), (C.c_char_p * max(len(rnames), 1))(*[r.encode() for r in rnames]), lens.ctypes.data)
    text = C.string_at(p).decode()
    lib.simmr_host_free(p)
    return text


def test_host_header_writer_equals_the_python_one(host_lib):
    for rnames, lengths in ((["chr1", "plasmid|2", "x=*"], [1000, 2**33, 1]), (["a"], [0]), ([], [])):
        assert host_header(host_lib, rnames, lengths) == sam_header(rnames, lengths)
    for bad in (["a", "a"], ["has space"], ["=x"], ["*"], [""], ["x" * 255]):
        assert host_header(host_lib, bad, [1] * len(bad)).startswith("ERR\t"), bad
        with pytest.raises(ValueError):
            sam_header(bad, [1] * len(bad))
    for sid in ("NC_000913.3 Escherichia coli K-12", "a\tb", "  lead", "", "one"):
        p = host_lib.simmr_host_sam_rname(sid.encode())
        assert C.string_at(p).decode() == rname_of(sid), sid
        host_lib.simmr_host_free(p)


USAGE_ROWS = [
    (["--sam"], 2, "error: a value is required for '--sam'"),
    (["--sam="], 2, "error: a file name is required for '--sam'"),
    (["--genome", "a.fna", "--sam", "x.sam"], 2, "error: --output is required"),
    (["--genome", "a.fna", "--output", "x.fq", "--sam", "x.sam", "--devices", "0,1"], 1, "ERROR simmr-hip: --sam does not combine with --devices: use --device"),
    # the refusals that were there come first
    (["--genome", "a.fna", "--output", "x.fq", "--sam", "x.sam", "--truth", "t.tsv", "--devices", "0,1"], 1,
     "ERROR simmr-hip: --truth does not combine with --devices: use --device"),
]


@pytest.mark.parametrize("argv,status,line", USAGE_ROWS, ids=[" ".join(r[0]) for r in USAGE_ROWS])
def test_cli_usage_rows(host_lib, argv, status, line):
    r = subprocess.run([str(HOST / "simmr-hip")] + argv, capture_output=True, text=True)
    assert (r.returncode, r.stderr.splitlines()[0]) == (status, line)


def test_help_describes_the_flag(host_lib):
    helptext = subprocess.check_output([str(HOST / "simmr-hip"), "--help"]).decode()
    assert "--sam <FILE>" in helptext and "MD:Z:" in helptext and "not with --devices" in helptext.split("--sam <FILE>")[1].split("--stats")[0]


def test_duplicate_and_illegal_rnames_end_the_run_before_any_device_work(host_lib, tmp_path):
    """no device is needed to be refused: the check reads the FASTA records' ids"""
    (tmp_path / "a.fna").write_text(">chr1 first assembly\nACGTACGT\n>chr2\nACGT\n")
    (tmp_path / "b.fna").write_text(">other\nACGT\n>chr1 second assembly\nACGTAC\n")
    (tmp_path / "c.fna").write_text(">fine\nACGT\n>=odd name\nACGT\n")
    exe, out = str(HOST / "simmr-hip"), ["--output", str(tmp_path / "x.fq"), "--sam", str(tmp_path / "x.sam")]
    r = subprocess.run([exe, "--genome", str(tmp_path / "a.fna"), "--genome", str(tmp_path / "b.fna")] + out, capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.splitlines() == [
        f"ERROR simmr-hip: --sam: sequence 'chr1 second assembly' of {tmp_path}/b.fna gets the RNAME 'chr1', which sequence "
        f"'chr1 first assembly' of {tmp_path}/a.fna has already"]
    r = subprocess.run([exe, "--genome", str(tmp_path / "c.fna")] + out, capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.splitlines() == [
        f"ERROR simmr-hip: --sam: sequence '=odd name' of {tmp_path}/c.fna gets the RNAME '=odd', which is not a SAM reference name"]
    assert not (tmp_path / "x.sam").exists() and not (tmp_path / "x.fq").exists()
    (tmp_path / "g.tsv").write_text("path\tid\n" + f"{tmp_path}/a.fna\tgA\n{tmp_path}/a.fna\tgB\n")
    r = subprocess.run([exe, "--genome-file", str(tmp_path / "g.tsv")] + out, capture_output=True, text=True)
    assert r.returncode == 1 and "gets the RNAME 'chr1', which sequence 'chr1 first assembly'" in r.stderr
