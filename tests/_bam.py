"""The BAM record and the BGZF block of include/simmr_hip.h (simmr_bam_plan, simmr_bgzf_frame) restated in plain Python — TEST
INFRASTRUCTURE ONLY: numpy and the standard library.

A writer (bam_records, from the columns tests/_sam.py takes), a reader written separately from it (parse_bam, to_sam_line) and a
walker of BGZF blocks that checks every field of every block.  Nothing here comes from the code under test."""
import struct
import zlib

import numpy as np

from tests import _sam

CODE = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15}
LETTER = "=ACMGRSVTWYHKDBN"
BGZF_BLOCK = 0xff00
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def reg2bin(beg, end):
    """SAM spec 5.3, for the zero-based half-open [beg, end)"""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def rows_of(rnames):
    """{(genome slot, contig): refID} for [(slot, [RNAME per contig]), ...]: flattened entry by entry"""
    rows, k = {}, 0
    for slot, names in rnames:
        for c in range(len(names)):
            rows[(int(slot), c)] = k
            k += 1
    return rows


def record(o, t, rows, r, paired):
    a, b = int(o["start"][r]), int(o["end"][r])
    lo, hi = min(a, b), max(a, b)
    L = hi - lo
    rev = bool(int(o["flags"][r]) & 1)
    ref_id = rows[(int(o["genome"][r]), int(o["contig"][r]))]
    if paired:
        m = r ^ 1
        ma, mb = int(o["start"][m]), int(o["end"][m])
        mlo, mhi = min(ma, mb), max(ma, mb)
        mrev = bool(int(o["flags"][m]) & 1)
        flag = 0x1 | 0x2 | (0x10 if rev else 0) | (0x20 if mrev else 0) | (0x80 if r & 1 else 0x40)
        span = max(hi, mhi) - min(lo, mlo)
        positive = lo < mlo or (lo == mlo and not r & 1)
        mate = (ref_id, mlo, span if positive else -span)
    else:
        flag = 16 if rev else 0
        mate = (-1, -1, 0)
    s0, s1 = int(o["seq_off"][r]), int(o["seq_off"][r + 1])
    assert s1 - s0 == L
    seq = bytes(o["seq"][s0:s1]).decode("latin-1")
    qual = bytes(o["qual"][s0:s1])
    if rev:
        seq, qual = seq[::-1], qual[::-1]
    codes = [CODE[_sam._base(ch, rev)] for ch in seq] + [0]
    packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, L, 2))
    e0, e1 = int(t["edit_off"][r]), int(t["edit_off"][r + 1])
    n = e1 - e0
    md = _sam.md_string(L, rev, t["edit_pos"][e0:e1], t["edit_ref"][e0:e1])
    name = str(int(o["read_id"][r])).encode() + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref_id, lo, len(name), 255, reg2bin(lo, hi if L else lo + 1) & 0xffff, 1 if L else 0, flag, L, *mate)
    body += name + (struct.pack("<I", L << 4) if L else b"") + packed + bytes(max(q, 33) - 33 for q in qual)
    body += (b"NMC" + struct.pack("<B", n) if n <= 255 else b"NMS" + struct.pack("<H", n)) + b"MDZ" + md.encode() + b"\0"
    return struct.pack("<i", len(body)) + body


def bam_records(o, t, rnames, paired):
    """the records of every read back to back; rnames = [(genome slot, [RNAME per contig]), ...]"""
    rows = rows_of(rnames)
    return b"".join(record(o, t, rows, r, paired) for r in range(len(o["start"])))


# ---- the reader -------------------------------------------------------------------------------------------------------
def parse_records(buf, at=0):
    """every record of buf[at:] as a dict of its fields"""
    out = []
    while at < len(buf):
        (size,) = struct.unpack_from("<i", buf, at)
        rec = buf[at + 4:at + 4 + size]
        assert size >= 32 and len(rec) == size, (at, size)
        ref_id, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, next_ref, next_pos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 0)
        p = 32
        name = rec[p:p + l_name]
        assert name.endswith(b"\0") and b"\0" not in name[:-1]
        p += l_name
        cigar = struct.unpack_from(f"<{n_cigar}I", rec, p)
        p += 4 * n_cigar
        packed = rec[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        if l_seq & 1:
            assert packed[-1] & 0xf == 0
        seq = "".join(LETTER[packed[i >> 1] >> 4 if i % 2 == 0 else packed[i >> 1] & 0xf] for i in range(l_seq))
        qual = rec[p:p + l_seq]
        p += l_seq
        tags = {}
        while p < size:
            tag, typ = rec[p:p + 2].decode(), chr(rec[p + 2])
            p += 3
            if typ in "CS":
                width = {"C": 1, "S": 2}[typ]
                tags[tag] = (typ, int.from_bytes(rec[p:p + width], "little"))
                p += width
            else:
                assert typ == "Z", typ
                end = rec.index(b"\0", p)
                tags[tag] = (typ, rec[p:end].decode())
                p = end + 1
        assert p == size
        out.append({"ref_id": ref_id, "pos": pos, "mapq": mapq, "bin": bin_, "cigar": cigar, "flag": flag, "next_ref": next_ref, "next_pos": next_pos,
                    "tlen": tlen, "name": name[:-1].decode(), "seq": seq, "qual": qual, "tags": tags})
        at += 4 + size
    assert at == len(buf)
    return out


def parse_bam(stream):
    """(header text, [(name, length)], records) of an uncompressed BAM stream"""
    assert stream[:4] == b"BAM\1"
    (l_text,) = struct.unpack_from("<i", stream, 4)
    text = stream[8:8 + l_text].decode()
    at = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", stream, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", stream, at)
        name = stream[at + 4:at + 4 + l_name]
        assert name.endswith(b"\0")
        (l_ref,) = struct.unpack_from("<i", stream, at + 4 + l_name)
        refs.append((name[:-1].decode(), l_ref))
        at += 8 + l_name
    return text, refs, parse_records(stream, at)


def to_sam_line(rec, refs):
    """the SAM line of a parsed record, as samtools view prints one of these (tags in the record's order)"""
    ops = "".join(f"{c >> 4}{'MIDNSHP=X'[c & 0xf]}" for c in rec["cigar"]) or "*"
    rname = refs[rec["ref_id"]][0]
    rnext = "*" if rec["next_ref"] < 0 else ("=" if rec["next_ref"] == rec["ref_id"] else refs[rec["next_ref"]][0])
    assert rec["bin"] == reg2bin(rec["pos"], rec["pos"] + max(len(rec["seq"]), 1)) & 0xffff
    fields = [rec["name"], str(rec["flag"]), rname, str(rec["pos"] + 1), str(rec["mapq"]), ops, rnext, str(rec["next_pos"] + 1), str(rec["tlen"]),
              rec["seq"] or "*", "".join(chr(q + 33) for q in rec["qual"]) or "*"]
    for tag, (typ, v) in rec["tags"].items():
        fields.append(f"{tag}:{'Z' if typ == 'Z' else 'i'}:{v}")
    return "\t".join(fields) + "\n"


# ---- BGZF -------------------------------------------------------------------------------------------------------------
def bgzf_blocks(buf, one_call=True):
    """the payloads of the blocks of buf, every field of every block checked; one_call: buf is what ONE simmr_bgzf_frame wrote, so
    every block but the last is full (a file is several calls' blocks back to back)"""
    out, at = [], 0
    while at < len(buf):
        assert buf[at:at + 4] == b"\x1f\x8b\x08\x04" and buf[at + 4:at + 8] == b"\0\0\0\0" and buf[at + 8:at + 10] == b"\x00\xff", at
        assert buf[at + 10:at + 12] == b"\x06\x00" and buf[at + 12:at + 16] == b"BC\x02\x00", at
        (bsize,) = struct.unpack_from("<H", buf, at + 16)
        total = bsize + 1
        assert at + total <= len(buf), (at, total)
        assert buf[at + 18] == 1, "one stored deflate block, the last"
        ln, nln = struct.unpack_from("<HH", buf, at + 19)
        assert ln ^ nln == 0xffff and ln == total - 31 and 1 <= ln <= BGZF_BLOCK, (at, ln, nln, total)
        data = buf[at + 23:at + 23 + ln]
        crc, isize = struct.unpack_from("<II", buf, at + 23 + ln)
        assert isize == ln and crc == zlib.crc32(data), (at, ln, hex(crc), hex(zlib.crc32(data)))
        out.append(data)
        at += total
    assert at == len(buf)
    assert not one_call or all(len(d) == BGZF_BLOCK for d in out[:-1])
    return out


def bgzf_bound(n):
    return n + 31 * ((n + BGZF_BLOCK - 1) // BGZF_BLOCK)


def bgzf_frame(data):
    """the blocks simmr_bgzf_frame writes for `data`"""
    out = []
    for at in range(0, len(data), BGZF_BLOCK):
        d = bytes(data[at:at + BGZF_BLOCK])
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(d) + 30) + b"\x01" +
                   struct.pack("<HH", len(d), len(d) ^ 0xffff) + d + struct.pack("<II", zlib.crc32(d), len(d)))
    return b"".join(out)
