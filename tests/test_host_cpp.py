"""C++ host layer (simmr_amd/host): FASTA ingest + normalisation, genome TSV,
FASTQ header interpolation, metadata float formatting, CLI surface and usage errors, failed writes — CPU only.
Mirrors the reference's genome_tests.rs and the formats of fastq.rs / files.rs."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"
GOLDEN = Path(__file__).parent / "golden"
DEFAULT_FMT = ("@{:read_id:}|{:genome_id:}/{:pair:} metadata:sid={:sequence_id:}|sp={:start_position:}"
               "|ep={:end_position:}|rc={:reverse_complement:}")


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-s", "-C", str(HOST), "libsimmr_host.so"])
    import os
    # SIMMR_HOST_LIB: another build of the same sources (a -fsanitize=address,undefined build for sanitizer runs)
    lib = C.CDLL(os.environ.get("SIMMR_HOST_LIB") or str(HOST / "libsimmr_host.so"))
    for f in ("simmr_host_normalize", "simmr_host_format_f64", "simmr_host_format_header",
              "simmr_host_load_fasta", "simmr_host_parse_genome_file"):
        getattr(lib, f).restype = C.c_void_p
    lib.simmr_host_format_f64.argtypes = [C.c_double]
    lib.simmr_host_normalize.argtypes = [C.c_char_p, C.c_uint64]
    lib.simmr_host_format_header.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint64,
                                             C.c_uint64, C.c_int, C.c_int]
    lib.simmr_host_load_fasta.argtypes = [C.c_char_p, C.c_int]
    lib.simmr_host_parse_genome_file.argtypes = [C.c_char_p]
    lib.simmr_host_free.argtypes = [C.c_void_p]

    def s(ptr):
        v = C.string_at(ptr).decode()
        lib.simmr_host_free(ptr)
        return v
    lib.s = s
    return lib


def test_genome_from_fasta_reference_unit_test(host):
    # genome_tests.rs:7-20 on the reference's own fixture (data copied to tests/golden)
    out = host.s(host.simmr_host_load_fasta(str(GOLDEN / "sample.fna").encode(), 0)).split("\n")
    assert out[0] == "2\t320"
    h1 = out[1].split("\t")
    h2 = out[2].split("\t")
    assert (h1[0], h1[1], h2[0], h2[1]) == ("header1", "160", "header2", "160")
    assert h1[3].startswith("AGCTTTTCATTCTGACTGCAACGGGCAATATGTCTCTG") and len(h1[3]) == 160
    # --contiguous: one 'whole genome' sequence, 'N' after every record, size excludes the separators
    out = host.s(host.simmr_host_load_fasta(str(GOLDEN / "sample.fna").encode(), 1)).split("\n")
    assert out[0] == "1\t320"
    w = out[1].split("\t")
    assert w[0] == "whole genome" and w[1] == "320" and w[2] == "322"
    assert w[3][160] == "N" and w[3][321] == "N" and w[3][:160] == h1[3]


def test_normalize_needletail_semantics(host):
    raw = b"acgtn ACGTN-\n.~uUxRyY*\r\n\tGG"
    assert host.s(host.simmr_host_normalize(raw, len(raw))) == "ACGTNACGTN---TTNNNNNGG"


def test_fasta_edge_cases(host, tmp_path):
    p = tmp_path / "a.fna"
    p.write_bytes(b">id one two\r\nACGT\r\nacgt\r\n>empty\n>last\nNN--")
    out = host.s(host.simmr_host_load_fasta(str(p).encode(), 0)).split("\n")
    assert out[0] == "3\t12"
    assert out[1].split("\t")[:3] == ["id one two", "8", "8"] and out[1].endswith("ACGTACGT")
    assert out[2].split("\t")[:3] == ["empty", "0", "0"]
    assert out[3].split("\t") == ["last", "4", "4", "NN--"]
    assert host.s(host.simmr_host_load_fasta(str(tmp_path / "missing").encode(), 0)).startswith("ERR\t")
    (tmp_path / "bad").write_bytes(b"ACGT\n")
    assert host.s(host.simmr_host_load_fasta(str(tmp_path / "bad").encode(), 0)).startswith("ERR\t")


def test_genome_file_variants(host, tmp_path):
    p = tmp_path / "g.tsv"
    p.write_text("path\tid\tabundance\n/a/b.fna\tg1\t0.25\n/c.fna\t\t\n")
    assert host.s(host.simmr_host_parse_genome_file(str(p).encode())) == "/a/b.fna\tg1\t0.25\n/c.fna\t<none>\t<none>\n"
    p.write_text("abundance\tgenome_id\tfilepath\n1e-3\tx\t/z.fna\n")  # any column order, serde aliases
    assert host.s(host.simmr_host_parse_genome_file(str(p).encode())) == "/z.fna\tx\t0.001\n"
    p.write_text("/plain/one.fna\n/plain/two.fna\n")  # plain list (extension; the reference mis-detects it)
    assert host.s(host.simmr_host_parse_genome_file(str(p).encode())) == "/plain/one.fna\t<none>\t<none>\n/plain/two.fna\t<none>\t<none>\n"


@pytest.mark.parametrize("v,s", [(100.0, "100"), (20.0, "20"), (33.333333333333336, "33.333333333333336"),
                                 (0.1, "0.1"), (1e-7, "0.0000001"), (1.5e21, "1500000000000000000000"),
                                 (0.015625, "0.015625"), (2.5, "2.5"), (1 / 3, "0.3333333333333333")])
def test_f64_display_like_rust(host, v, s):
    assert host.s(host.simmr_host_format_f64(v)) == s


def test_header_interpolation(host):
    h = host.s(host.simmr_host_format_header(DEFAULT_FMT.encode(), b"abc123", 7, b"NC_000913.3 Escherichia coli", 10,
                                             160, 0, 1))
    assert h == "@7|abc123/1 metadata:sid=NC_000913.3 Escherichia coli|sp=10|ep=160|rc=f"
    h = host.s(host.simmr_host_format_header(b"@{:read_id:}/{:pair:} {:read_id:}", b"g", 5, b"s", 9, 3, 1, 2))
    assert h == "@5/2 5"


def test_cli_surface():
    subprocess.check_call(["make", "-s", "-C", str(HOST), "simmr-hip"])
    exe = str(HOST / "simmr-hip")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--genome", "--genome-file", "--output", "--num-reads", "--read-length", "--read-length-std",
                 "--insert-size", "--mean-phred-score", "--error-profile", "--abundance-profile", "--custom-profile",
                 "--with-ani", "--read-header-format", "--seed", "--size-adjusted", "--contiguous"):
        assert flag in r.stdout, flag
    assert subprocess.run([exe, "--output", "x"], capture_output=True).returncode == 2       # genomes group required
    assert subprocess.run([exe, "--genome", "a"], capture_output=True).returncode == 2       # --output required
    assert subprocess.run([exe, "--genome", "a", "--output", "x", "--error-profile", "ont"], capture_output=True).returncode == 2
    assert subprocess.run([exe, "--genome", "/nonexistent.fna", "--output", "/tmp/x.fq"], capture_output=True).returncode == 1


# argv -> (exit status, first line of stderr), recorded from the command line as it was before its parser and its side outputs
# were put in order: a missing value, a value out of range or malformed, the zero cases, the four file-name flags, --devices
# lists, the enumerations, unknown arguments, the three group errors at the end of the parser, and the side outputs with
# --devices.  None of them gets as far as a device.
USAGE_ERRORS = [
    (['--genome'], 2, "error: a value is required for '--genome'"),
    (['--genome-file'], 2, "error: a value is required for '--genome-file'"),
    (['--output'], 2, "error: a value is required for '--output'"),
    (['--num-reads'], 2, 'error: invalid value for --num-reads'),
    (['--read-length'], 2, 'error: invalid value for --read-length'),
    (['--read-length-std'], 2, "error: a value is required for '--read-length-std'"),
    (['--seed'], 2, 'error: invalid value for --seed'),
    (['--devices'], 2, "error: a value is required for '--devices'"),
    (['--device'], 2, 'error: invalid value for --device'),
    (['--depth-window'], 2, 'error: invalid value for --depth-window (1 .. 2^30 - 1)'),
    (['--rng'], 2, "error: a value is required for '--rng'"),
    (['--gamma'], 2, "error: a value is required for '--gamma'"),
    (['--error-profile'], 2, "error: a value is required for '--error-profile'"),
    (['--num-reads', '-1'], 2, 'error: invalid value for --num-reads'),
    (['--num-reads='], 2, 'error: invalid value for --num-reads'),
    (['--num-reads', '18446744073709551616'], 2, 'error: one of --genome / --genome-file is required'),
    (['--seed', '1x'], 2, 'error: invalid value for --seed'),
    (['--read-length', '65536'], 2, 'error: invalid value for --read-length'),
    (['--insert-size', '70000'], 2, 'error: invalid value for --insert-size'),
    (['--mean-phred-score', '256'], 2, 'error: invalid value for --mean-phred-score'),
    (['--with-ani', '300'], 2, 'error: invalid value for --with-ani'),
    (['--device', '1024'], 2, 'error: invalid value for --device'),
    (['--depth-window', '1073741824'], 2, 'error: invalid value for --depth-window (1 .. 2^30 - 1)'),
    (['--depth-window', '0'], 2, 'error: invalid value for --depth-window (1 .. 2^30 - 1)'),
    (['--device-chunk-reads', '0'], 2, 'error: invalid value for --device-chunk-reads'),
    (['--truth'], 2, "error: a value is required for '--truth'"),
    (['--truth='], 2, "error: a file name is required for '--truth'"),
    (['--stats'], 2, "error: a value is required for '--stats'"),
    (['--stats='], 2, "error: a file name is required for '--stats'"),
    (['--depth'], 2, "error: a value is required for '--depth'"),
    (['--depth='], 2, "error: a file name is required for '--depth'"),
    (['--depth-track'], 2, "error: a value is required for '--depth-track'"),
    (['--depth-track='], 2, "error: a file name is required for '--depth-track'"),
    (['--devices', '0,x'], 2, 'error: invalid value for --devices (a comma-separated list of device ordinals)'),
    (['--devices='], 2, 'error: invalid value for --devices (a comma-separated list of device ordinals)'),
    (['--devices', '0,,1'], 2, 'error: invalid value for --devices (a comma-separated list of device ordinals)'),
    (['--devices', '0,1024'], 2, 'error: invalid value for --devices (a comma-separated list of device ordinals)'),
    (['--devices', ','.join(['0'] * 65)], 2, 'error: invalid value for --devices'),
    (['--rng', 'mt19937'], 2, 'error: invalid value for --rng (reference, philox, philox-full)'),
    (['--gamma', '5'], 2, 'error: --gamma expects mean,std'),
    (['--gamma', '0,1'], 2, 'error: --gamma expects mean,std'),
    (['--gamma', 'a,b'], 2, 'error: --gamma expects mean,std'),
    (['--error-profile', 'ont'], 2, "error: invalid value 'ont' for '--error-profile'"),
    (['--abundance-profile', 'foo'], 2, "error: invalid value 'foo' for '--abundance-profile'"),
    (['--bogus'], 2, "error: Found argument '--bogus' which wasn't expected"),
    (['--bogus=1'], 2, "error: Found argument '--bogus' which wasn't expected"),
    (['reads.fq'], 2, "error: Found argument 'reads.fq' which wasn't expected"),
    (['--output', 'x.fq'], 2, 'error: one of --genome / --genome-file is required'),
    (['--genome', 'a.fna', '--genome-file', 'g.tsv', '--output', 'x.fq'], 2, 'error: --genome and --genome-file cannot be used together'),
    (['--genome', 'a.fna'], 2, 'error: --output is required'),
    (['--genome', 'a.fna', '--output', 'x.fq', '--devices', '0,1', '--truth', 't.tsv'], 1, 'ERROR simmr-hip: --truth does not combine with --devices: use --device'),
    (['--genome', 'a.fna', '--output', 'x.fq', '--devices', '0,1', '--stats', 's.tsv'], 1, 'ERROR simmr-hip: --stats does not combine with --devices: use --device'),
    (['--genome', 'a.fna', '--output', 'x.fq', '--devices', '0,1', '--depth', 'd.tsv'], 1, 'ERROR simmr-hip: --depth does not combine with --devices: use --device'),
    (['--genome', 'a.fna', '--output', 'x.fq', '--devices', '0,1', '--depth-track', 'w.tsv'], 1, 'ERROR simmr-hip: --depth does not combine with --devices: use --device'),
    (['--genome', 'a.fna', '--output', 'x.fq', '--devices', '0', '--truth', 't.tsv', '--stats', 's.tsv', '--depth', 'd.tsv'], 1, 'ERROR simmr-hip: --truth does not combine with --devices: use --device'),
]


@pytest.mark.parametrize("argv,status,first", USAGE_ERRORS, ids=[" ".join(a)[:60] for a, _, _ in USAGE_ERRORS])
def test_cli_usage_errors(argv, status, first, tmp_path):
    subprocess.check_call(["make", "-s", "-C", str(HOST), "simmr-hip"])
    r = subprocess.run([str(HOST / "simmr-hip")] + argv, capture_output=True, text=True, cwd=tmp_path)
    assert (r.returncode, r.stderr.split("\n")[0]) == (status, first)
    assert not list(tmp_path.iterdir())  # nothing was written


@pytest.mark.skipif(not Path("/dev/full").exists(), reason="no /dev/full on this system")
def test_every_writer_reports_a_failed_write(host):
    """A device that takes no byte: each TSV writer answers the one message of the output-file helper."""
    import numpy as np
    from simmr_amd import _abi
    full = b"/dev/full"
    n, gids, ncs, sids = 10, (C.c_char_p * 1)(b"g"), (C.c_uint32 * 1)(2), (C.c_char_p * 2)(b"c0", b"c1")
    for f in ("simmr_host_truth_tsv", "simmr_host_stats_tsv", "simmr_host_depth_tsv"):
        getattr(host, f).restype = C.c_void_p
    # truth: ten reads on two contigs, one edit each
    host.simmr_host_truth_tsv.argtypes = [C.c_uint64, C.c_int] + [C.c_void_p] * 12 + [C.c_uint32, C.c_uint32, C.POINTER(C.c_char_p),
                                                                                       C.POINTER(C.c_uint32), C.POINTER(C.c_char_p), C.c_int, C.c_char_p]
    r = np.arange(n)
    cols = [r.astype(np.uint32), np.zeros(n, np.uint32), (r % 2).astype(np.uint32), (r * 10).astype(np.uint64), (r * 10 + 50).astype(np.uint64),
            np.zeros(n, np.uint8), np.ones(n, np.uint32), np.arange(n + 1, dtype=np.uint64), (r % 50).astype(np.uint32),
            np.full(n, ord("A"), np.uint8), np.full(n, ord("C"), np.uint8), np.full(n, 33 + 30, np.uint8)]
    assert host.s(host.simmr_host_truth_tsv(n, 1, *[c.ctypes.data for c in cols], 33, 1, gids, ncs, sids, 1, full)) == "ERR\tshort write to /dev/full"
    # statistics: a few non-zero entries
    host.simmr_host_stats_tsv.argtypes = [C.POINTER(_abi.RunStats), C.c_char_p]
    st = _abi.RunStats()
    st.reads[0], st.reads[1], st.bases[0], st.bases[1] = 5, 5, 750, 750
    assert host.s(host.simmr_host_stats_tsv(C.byref(st), full)) == "ERR\tshort write to /dev/full"
    # depth: two contigs, three windows; the per-contig file, then (with a good first file) the track
    host.simmr_host_depth_tsv.argtypes = [C.POINTER(_abi.DepthContig), C.c_uint64, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_char_p), C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p]
    rows = (_abi.DepthContig * 2)()
    rows[0].genome, rows[0].contig, rows[0].len, rows[0].first_window = 0, 0, 150, 0
    rows[1].genome, rows[1].contig, rows[1].len, rows[1].first_window = 0, 1, 80, 2
    ws, wc, wm = np.ones(3, np.uint64), np.ones(3, np.uint32), np.ones(3, np.uint32)
    win = (100, ws.ctypes.data, wc.ctypes.data, wm.ctypes.data)
    assert host.s(host.simmr_host_depth_tsv(rows, 2, 1, gids, ncs, sids, full, *win, full)) == "ERR\tshort write to /dev/full"
    assert host.s(host.simmr_host_depth_tsv(rows, 2, 1, gids, ncs, sids, None, *win, full)) == "ERR\tshort write to /dev/full"
