"""The header of a SAM file for the alignment lines Engine.sam() makes on the device (the host writes these few lines)."""
from __future__ import annotations

import re
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
