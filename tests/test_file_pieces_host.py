"""The piece reader of host.cpp (PieceReader, piece_cut), which the nine commands of simmr-hip that run no simulation read their files
with, without a GPU: a stand-alone program under the sanitizers at piece sizes of a few bytes, against a plain statement of the three
cut rules.  At the CLI's 64 MiB a piece only files of that size reach the carry; here every branch is a file of a few lines."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "simmr_amd" / "host"
PIECES = (1, 7, 16, 64)
BIG = 1 << 20


@pytest.fixture(scope="module")
def pieces_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("file_pieces") / "file_pieces_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "file_pieces_main.cpp"), str(HOST / "host.cpp")])
    return exe


def cut(buf: bytes, rule: str) -> int:
    """where a buffer of a file that has not ended is cut; 0: nowhere, read on"""
    if rule == "newline":  # behind the last newline
        return buf.rfind(b"\n") + 1
    if rule == "fasta":  # in front of the last '>' that begins a line; the buffer's first byte begins the piece and is no cut
        return buf.rfind(b"\n>") + 1
    k = int(rule.split(":")[1])  # behind the last newline whose number is a multiple of the record's lines
    ends = [i + 1 for i, b in enumerate(buf) if b == 10]
    return ends[len(ends) // k * k - 1] if len(ends) >= k else 0


def model(data: bytes, rule: str, piece: int, limit: int):
    """(the pieces, the end, the bytes of the file consumed)"""
    out, buf, at = [], b"", 0
    while True:
        chunk = data[at:at + piece]
        at += len(chunk)
        buf += chunk
        eof = len(chunk) < piece
        c = len(buf) if eof else cut(buf, rule)
        if c == 0 and not eof:
            if rule == "fasta" and len(buf) > limit:  # the only rule that looks at the limit while it reads on
                return out, "too-long", at
            continue
        if c > limit:
            return out, "too-long", at
        if c:
            out.append(buf[:c])
        if eof:
            return out, "done", at
        buf = buf[c:]


def run(exe, path, rule, piece, limit):
    r = subprocess.run([str(exe), str(path), rule, str(piece), str(limit)], capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    out, pieces, at = r.stdout, [], 0
    while out.startswith(b"piece ", at):
        nl = out.index(b"\n", at)
        n = int(out[at + 6:nl])
        pieces.append(out[nl + 1:nl + 1 + n])
        assert out[nl + 1 + n:nl + 2 + n] == b"\n"
        at = nl + 2 + n
    word, end, consumed = out[at:].split()
    assert word == b"end" and out.endswith(b"\n")
    return pieces, end.decode(), int(consumed)


def on_boundary(piece: bytes, following: bytes, rule: str) -> bool:
    if rule == "newline":
        return piece.endswith(b"\n")
    if rule == "fasta":
        return piece.endswith(b"\n") and following.startswith(b">")
    return piece.endswith(b"\n") and piece.count(b"\n") % int(rule.split(":")[1]) == 0


FASTQ = b"".join(b"@r%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % i for i in range(5))
TWO_LINE = b"".join(b">r%d\nACGTAC\n" % i for i in range(7))
FASTA = b">a|1 first\nACGT\nAC\n>b|2\nGGGGGGGGGGGGGGGGGGGGGG\n>c|3\n\n>d|4\nT\n"
LONG_FASTA = b">a\n" + b"A" * 50 + b"\n>b\n" + b"C" * 30 + b"\n"

# name: (the file, the rules, the limit, the end every piece size must meet or None where it depends on the size)
CASES = {
    "an empty file": (b"", ("newline", "fasta", "record:2", "record:4"), BIG, "done"),
    "one byte, no newline": (b"x", ("newline", "fasta", "record:2"), BIG, "done"),
    "lines, the last with its newline": (b"ab\ncdefgh\n\nij\nklmnopqrstuvw\nx\n", ("newline", "record:2", "record:4"), BIG, "done"),
    "lines, the last without its newline": (b"ab\ncdefgh\n\nij\nklmnopqrstuvw\nx", ("newline", "record:2", "record:4"), BIG, "done"),
    "exactly 16 bytes": (b"abc\ndefg\nhijklm\n", ("newline", "fasta", "record:2"), BIG, "done"),
    "exactly 16 bytes of one open line": (b"abcdefghijklmnop", ("newline", "fasta", "record:4"), BIG, "done"),
    "a line of many pieces between short ones": (b"ab\n" + b"x" * 200 + b"\ncd\n", ("newline", "record:2"), BIG, "done"),
    "a line longer than the limit, behind lines that fit": (b"ab\ncd\n" + b"x" * 50 + b"\nef\n", ("newline", "record:2"), 20, "too-long"),
    "a last line longer than the limit, without its newline": (b"ab\ncd\n" + b"x" * 50, ("newline", "record:2", "fasta"), 20, "too-long"),
    "records of 4 lines, whole": (FASTQ, ("record:4", "newline"), BIG, "done"),
    "records of 4 lines, the last one short of two": (FASTQ + b"@r9\nACGT\n", ("record:4",), BIG, "done"),
    "records of 2 lines, whole": (TWO_LINE, ("record:2", "fasta"), BIG, "done"),
    "records of 2 lines, the last one short, no newline": (TWO_LINE + b">r9", ("record:2", "fasta"), BIG, "done"),
    "a record of 4 lines longer than the limit": (FASTQ[:28] + b"@big\n" + b"A" * 40 + b"\n+\n" + b"I" * 40 + b"\n", ("record:4",), 60, "too-long"),
    "a FASTA of records, empty ones among them": (FASTA, ("fasta",), BIG, "done"),
    "a FASTA with '>' inside its header lines": (b">a x>y >z\nAC\n>b>c\nGT>\n>\nA\n", ("fasta",), BIG, "done"),
    "a FASTA whose only '>' is its first byte": (b">only one\n" + b"ACGTACGTAC\n" * 9, ("fasta",), BIG, "done"),
    "a FASTA without its last newline": (FASTA[:-1], ("fasta",), BIG, "done"),
    "a FASTA that begins with sequence lines": (b"ACGT\nAC\n>a\nGG\n>b\nT\n", ("fasta",), BIG, "done"),
    "a FASTA record longer than the limit": (LONG_FASTA, ("fasta",), 20, "too-long"),
    "a FASTA record longer than the limit behind one that fits": (b">s\nAC\n" + LONG_FASTA, ("fasta",), 20, "too-long"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_pieces_against_the_rules(pieces_main, tmp_path, case):
    data, rules, limit, want_end = CASES[case]
    path = tmp_path / "file"
    path.write_bytes(data)
    for rule in rules:
        for piece in PIECES:
            pieces, end, consumed = run(pieces_main, path, rule, piece, limit)
            want = model(data, rule, piece, limit)
            assert (pieces, end, consumed) == want, (rule, piece)
            if want_end is not None:
                assert end == want_end, (rule, piece)
            assert all(0 < len(p) <= limit for p in pieces), (rule, piece)
            text = b"".join(pieces)
            assert data.startswith(text) and (text == data) == (end == "done"), (rule, piece)
            rest = [data[len(b"".join(pieces[:i + 1])):] for i in range(len(pieces))]
            last = len(pieces) - 1 if end == "done" else len(pieces)  # the last piece of a whole walk is the remainder
            assert all(on_boundary(p, rest[i], rule) for i, p in enumerate(pieces[:last])), (rule, piece)


def test_the_branches_the_cases_are_there_for(pieces_main, tmp_path):
    """what the cases above rely on, said once by hand, so that a model wrong in the reader's way does not pass with it"""
    path = tmp_path / "file"
    # the cut inside a line: the first read of 7 bytes is "ab\ncdef", and "cdef" is carried in front of the second
    path.write_bytes(b"ab\ncdefgh\n\nij\n")
    assert run(pieces_main, path, "newline", 7, BIG) == ([b"ab\n", b"cdefgh\n\nij\n"], "done", 14)
    assert run(pieces_main, path, "newline", 6, BIG) == ([b"ab\n", b"cdefgh\n\n", b"ij\n"], "done", 14)
    # a file of exactly one piece: the second read finds the end and nothing left; one byte shorter, and the carry is the last piece
    assert run(pieces_main, path, "newline", 14, BIG) == ([b"ab\ncdefgh\n\nij\n"], "done", 14)
    path.write_bytes(b"ab\ncdefgh\n\nij")
    assert run(pieces_main, path, "newline", 13, BIG) == ([b"ab\ncdefgh\n\n", b"ij"], "done", 13)
    # a record of 2 lines: three lines in the buffer give two; a last record short of a line is the remainder
    path.write_bytes(b">a\nAC\n>b\nGT\n>c\n")
    assert run(pieces_main, path, "record:2", 10, BIG) == ([b">a\nAC\n", b">b\nGT\n>c\n"], "done", 15)
    assert run(pieces_main, path, "fasta", 10, BIG) == ([b">a\nAC\n", b">b\nGT\n>c\n"], "done", 15)
    assert run(pieces_main, path, "fasta", 5, BIG) == ([b">a\nAC\n", b">b\nGT\n", b">c\n"], "done", 15)
    # FASTA: with reads of 16 the buffer passes the limit of 20 with no cut in sight, and the walk ends at 32 bytes; with reads of 64
    # the first buffer holds a cut at 54, which passes the limit; the newline rule reads the whole line before it says so
    path.write_bytes(LONG_FASTA)
    assert run(pieces_main, path, "fasta", 16, 20) == ([], "too-long", 32)
    assert run(pieces_main, path, "fasta", 64, 20) == ([], "too-long", 64)
    assert run(pieces_main, path, "newline", 16, 20) == ([b">a\n"], "too-long", 64)
    assert run(pieces_main, path, "fasta", 16, 54) == ([b">a\n" + b"A" * 50 + b"\n", b">b\n" + b"C" * 30 + b"\n"], "done", len(LONG_FASTA))
    assert run(pieces_main, path, "fasta", 16, 53)[:2] == ([], "too-long")
    # a record of four lines that passes the limit only as a whole
    data = CASES["a record of 4 lines longer than the limit"][0]
    path.write_bytes(data)
    assert run(pieces_main, path, "record:4", 7, 60)[:2] == ([FASTQ[:28]], "too-long")
    assert run(pieces_main, path, "record:4", 7, len(data) - 28)[:2] == ([FASTQ[:28], data[28:]], "done")


def test_a_file_that_cannot_be_read(pieces_main, tmp_path):
    """a directory opens and does not read: the third end"""
    pieces, end, _ = run(pieces_main, tmp_path, "newline", 16, BIG)
    assert pieces == [] and end == "cannot-read"
