"""The reference's FASTQ framing (fastq.rs:32-121) restated on the host over SoA columns: the chained String::replace of
the header template, then bases, "+", qualities.  Shared by the tests that compare the device's text with it."""
import numpy as np


def header(fmt, gid, sid, read_id, start, end, rev, pair):
    h = fmt  # fastq.rs:34-56: the replace calls in the reference's order
    for k, v in (("{:genome_id:}", gid), ("{:read_id:}", str(read_id)), ("{:sequence_id:}", sid),
                 ("{:start_position:}", str(start)), ("{:end_position:}", str(end)),
                 ("{:reverse_complement:}", "t" if rev else "f"), ("{:pair:}", pair)):
        h = h.replace(k, v)
    return h


def expected_text(d, names, fmt, paired, lo=0, hi=None, seq_base=0) -> bytes:
    """Records of reads [lo, hi) of the columns `d` (numpy, as Reads.to_host() gives them).  `names` = [(engine genome
    slot, genome id, [sequence id per contig]), ...].  `seq_base`: d["seq"] / d["qual"] start at that offset of the CSR
    (a window copied out of a larger run)."""
    by_slot = {slot: (gid, sids) for slot, gid, sids in names}
    hi = len(d["start"]) if hi is None else hi
    want = bytearray()
    for r in range(lo, hi):
        gid, sids = by_slot[int(d["genome"][r])]
        h = header(fmt, gid, sids[int(d["contig"][r])], int(d["read_id"][r]), int(d["start"][r]), int(d["end"][r]),
                   d["flags"][r] & 1, "2" if (paired and r & 1) else "1")
        a, b = int(d["seq_off"][r]) - seq_base, int(d["seq_off"][r + 1]) - seq_base
        want += h.encode() + b"\n" + d["seq"][a:b].tobytes() + b"\n+\n" + d["qual"][a:b].tobytes() + b"\n"
    return bytes(want)


def assert_same_text(got: bytes, want: bytes, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    if got != want:
        g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        i = int(np.flatnonzero(g != w)[0])
        raise AssertionError(f"{what}first difference at byte {i}: {got[max(0, i - 60):i + 20]!r} vs {want[max(0, i - 60):i + 20]!r}")
