"""The BAI index of include/simmr_hip.h (simmr_bai_plan) restated in plain Python — TEST INFRASTRUCTURE ONLY: the standard
library and tests/_bam.py.

Two halves that share no code.  A writer (bai_bytes) that follows the rules the header states, from parsed records; and a
reader (parse_bai, reg2bins, query) written from SAM spec 5.2 / 5.3 alone, which uses an index the way a consumer does: the
candidate bins' chunks, the linear index's lower bound, a seek by virtual offset, records parsed until the chunk ends."""
import bisect
import struct

from tests import _bam

BLOCK = 65280
FRAMED = 65311
META_BIN = 37450


# ---- the writer -----------------------------------------------------------------------------------------------------------
def voff(p):
    """the virtual offset of uncompressed position p of a stream whose blocks, but the last, hold 65280 bytes"""
    return ((p // BLOCK) * FRAMED) << 16 | (p % BLOCK)


def record_columns(records_bytes):
    """(ref_id, lo, end, offset) of every record of an unframed record stream, and the stream's length behind the last"""
    recs = _bam.parse_records(records_bytes)
    cols, at = [], 0
    for r in recs:
        (size,) = struct.unpack_from("<i", records_bytes, at)
        cols.append((r["ref_id"], r["pos"], r["pos"] + max(len(r["seq"]), 1), at))
        at += 4 + size
    assert at == len(records_bytes)
    return cols, at


def bai_bytes(n_ref, records_bytes, base):
    """the index of header (base bytes) + records_bytes framed as one stream; the records are coordinate-sorted"""
    cols, total = record_columns(records_bytes)
    assert all(a[:2] <= b[:2] for a, b in zip(cols, cols[1:])), "the records are not sorted"
    offs = [c[3] for c in cols] + [total]
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for ref in range(n_ref):
        mine = [i for i, c in enumerate(cols) if c[0] == ref]
        if not mine:
            out.append(struct.pack("<ii", 0, 0))
            continue
        bins = {}  # bin -> chunks, a chunk a maximal run of consecutive records of the bin
        prev_bin = None
        for i in mine:
            _, lo, end, _ = cols[i]
            b = _bam.reg2bin(lo, end)
            if b == prev_bin:
                bins[b][-1][1] = i + 1
            else:
                bins.setdefault(b, []).append([i, i + 1])
            prev_bin = b
        out.append(struct.pack("<i", len(bins) + 1))
        for b in sorted(bins):
            out.append(struct.pack("<Ii", b, len(bins[b])))
            for i0, i1 in bins[b]:
                out.append(struct.pack("<QQ", voff(base + offs[i0]), voff(base + offs[i1])))
        out.append(struct.pack("<IiQQQQ", META_BIN, 2, voff(base + offs[mine[0]]), voff(base + offs[mine[-1] + 1]), len(mine), 0))
        n_intv = 1 + ((max(cols[i][2] for i in mine) - 1) >> 14)
        first = [None] * n_intv
        for i in mine:
            _, lo, end, _ = cols[i]
            for w in range(lo >> 14, ((end - 1) >> 14) + 1):
                v = voff(base + offs[i])
                first[w] = v if first[w] is None else min(first[w], v)
        last = 0
        lin = []
        for w in range(n_intv):
            if first[w] is not None:
                last = first[w]
            lin.append(last)
        out.append(struct.pack(f"<i{n_intv}Q", n_intv, *lin))
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


# ---- the reader (SAM spec 5.2, 5.3) ------------------------------------------------------------------------------------------
def parse_bai(buf):
    """[{'bins': {bin: [(chunk_beg, chunk_end), ...]}, 'ioffset': [...]}, ...] per reference, and n_no_coor"""
    assert buf[:4] == b"BAI\1"
    (n_ref,) = struct.unpack_from("<i", buf, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", buf, at)
        at += 4
        bins, order = {}, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", buf, at)
            at += 8
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", buf, at + 16 * k) for k in range(n_chunk)]
            order.append(b)
            at += 16 * n_chunk
        (n_intv,) = struct.unpack_from("<i", buf, at)
        ioffset = list(struct.unpack_from(f"<{n_intv}Q", buf, at + 4))
        at += 4 + 8 * n_intv
        refs.append({"bins": bins, "order": order, "ioffset": ioffset})
    (n_no_coor,) = struct.unpack_from("<Q", buf, at)
    assert at + 8 == len(buf), (at, len(buf))
    return refs, n_no_coor


def reg2bins(beg, end):
    """SAM spec 5.3: the bins that may hold a record overlapping the zero-based half-open [beg, end)"""
    end -= 1
    out = [0]
    for first, shift in ((1, 26), (9, 23), (73, 20), (585, 17), (4681, 14)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


class Stream:
    """a BGZF file's blocks: where each starts in the file, and in the uncompressed stream"""

    def __init__(self, file_bytes):
        assert file_bytes.endswith(_bam.BGZF_EOF)
        payloads = _bam.bgzf_blocks(file_bytes[:-len(_bam.BGZF_EOF)])
        self.coff, self.ustart = [], []
        c = u = 0
        for d in payloads:
            self.coff.append(c)
            self.ustart.append(u)
            c += len(d) + 31
            u += len(d)
        self.coff.append(c)  # the EOF block
        self.ustart.append(u)
        self.data = b"".join(payloads)

    def upos(self, v):
        k = bisect.bisect_left(self.coff, v >> 16)
        assert k < len(self.coff) and self.coff[k] == v >> 16, ("no block starts there", v >> 16)
        return self.ustart[k] + (v & 0xffff)


def read_at(data, at):
    """(ref_id, pos, end, next offset) of the record at uncompressed offset `at`"""
    size, ref_id, pos = struct.unpack_from("<iii", data, at)
    (l_seq,) = struct.unpack_from("<i", data, at + 20)
    return ref_id, pos, pos + max(l_seq, 1), at + 4 + size


def query(bai, file_bytes, ref, beg, end):
    """the uncompressed offsets of the records of reference `ref` that overlap [beg, end), found through the index"""
    refs, _ = parse_bai(bai) if isinstance(bai, (bytes, bytearray)) else bai
    stream = file_bytes if isinstance(file_bytes, Stream) else Stream(file_bytes)
    idx = refs[ref]
    w = beg >> 14
    min_off = idx["ioffset"][w] if w < len(idx["ioffset"]) else (idx["ioffset"][-1] if idx["ioffset"] else 0)
    hits = []
    for b in reg2bins(beg, end):
        for c_beg, c_end in idx["bins"].get(b, ()):
            if c_end <= min_off:
                continue
            at, stop = stream.upos(c_beg), stream.upos(c_end)
            while at < stop:
                ref_id, pos, rend, nxt = read_at(stream.data, at)
                if ref_id == ref and pos < end and rend > beg:
                    hits.append(at)
                at = nxt
            assert at == stop, "a chunk ends inside a record"
    return sorted(hits)


def brute(stream, base, ref, beg, end):
    """the same by reading every record behind the header"""
    hits, at = [], base
    while at < len(stream.data):
        ref_id, pos, rend, nxt = read_at(stream.data, at)
        if ref_id == ref and pos < end and rend > beg:
            hits.append(at)
        at = nxt
    return hits
