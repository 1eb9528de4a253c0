"""The header of a SAM file for the alignment lines Engine.sam() makes on the device (the host writes these few lines), and
that of a BAM file for the records of Engine.bam()."""
from __future__ import annotations

import re
import struct
from typing import Sequence

RNAME = re.compile(r"[0-9A-Za-z!#$%&+./:;?@^_|~-][0-9A-Za-z!#$%&*+./:;=?@^_|~-]*")


def rname_of(sequence_id: str) -> str:
    """RNAME of a contig: the first whitespace-delimited token of its sequence id."""
    parts = sequence_id.split()
    return parts[0] if parts else ""


def sam_header(rnames: Sequence[str], lengths: Sequence[int], sort_order: str = "unsorted") -> str:
    """@HD, one @SQ per contig in names order, @PG.  The records carry no read group.  `sort_order`: "unsorted" for the lines of
    Engine.sam() (read order), "coordinate" for those of Engine.sam_sorted()."""
    if sort_order not in ("unsorted", "coordinate"):
        raise ValueError("sort_order is 'unsorted' or 'coordinate'")
    if len(rnames) != len(lengths):
        raise ValueError("one length per RNAME")
    seen = set()
    for name in rnames:
        if not RNAME.fullmatch(name) or len(name) > 254:
            raise ValueError(f"'{name}' is not a SAM reference name")
        if name in seen:
            raise ValueError(f"two contigs share the RNAME '{name}'")
        seen.add(name)
    lines = [f"@HD\tVN:1.6\tSO:{sort_order}"]
    lines += [f"@SQ\tSN:{name}\tLN:{int(n)}" for name, n in zip(rnames, lengths)]
    lines.append("@PG\tID:simmr-hip\tPN:simmr-hip")
    return "\n".join(lines) + "\n"


# the end-of-file marker of a BGZF stream (SIMMR_BGZF_EOF, SAM spec 4.1.2): an empty block, appended behind the last one
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bam_header(rnames: Sequence[str], lengths: Sequence[int], sort_order: str = "unsorted") -> bytes:
    """What a BAM file holds before its records, unframed: the magic BAM\1, l_text, the text of sam_header, n_ref, and per
    reference l_name, the name with its NUL, and l_ref.  Framed through Engine.bgzf it is the head of the stream whose records
    Engine.bam() makes.  The checks of sam_header; a length of 2^31 or more does not fit l_ref."""
    text = sam_header(rnames, lengths, sort_order).encode()
    for n in lengths:
        if not 0 <= int(n) < 2 ** 31:
            raise ValueError(f"a reference of {int(n)} bases does not fit BAM's l_ref")
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(rnames))]
    for name, n in zip(rnames, lengths):
        out += [struct.pack("<i", len(name) + 1), name.encode() + b"\0", struct.pack("<i", int(n))]
    return b"".join(out)
