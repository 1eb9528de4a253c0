"""The definition of an edit (include/simmr_hip.h, simmr_truth_out) restated in numpy — TEST INFRASTRUCTURE ONLY.

Same model as tests/test_gpu_blockloop.py::count_substitutions: the expected byte at offset j of read r is the genome's
byte at lo + j, or the complement of the byte at lo + L - 1 - j for a reverse-complemented read; an edit is an offset
whose byte differs.  Nothing here comes from the code under test."""
import numpy as np

from simmr_amd import _abi

_comp = None


def complement_lut(lib):
    global _comp
    if _comp is None:
        _comp = np.array([lib.orc_complement(b) for b in range(256)], dtype=np.uint8)
        assert _comp[ord("N")] == ord("N") and _comp[ord("-")] == ord("-")
    return _comp


def model(lib, o, genomes, chunk=20_000):
    """o: compact host columns (seq_off is a CSR of the lengths); genomes: {slot: HostGenome}.
    Returns nm, edit_off and the four edit columns as the header defines them."""
    comp = complement_lut(lib)
    n = len(o["start"])
    st, en = o["start"].astype(np.int64), o["end"].astype(np.int64)
    lo, L = np.minimum(st, en), np.abs(en - st)
    off = o["seq_off"].astype(np.int64)
    assert np.array_equal(np.diff(off), L)
    rev = (o["flags"] & _abi.FLAG_REVCOMP) != 0
    nm = np.zeros(n, dtype=np.uint32)
    pos, ref, alt, qual = [], [], [], []
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        for r in range(a, b):
            if L[r] == 0:
                continue
            g = genomes[int(o["genome"][r])].contigs[int(o["contig"][r])]
            want = g[lo[r]: lo[r] + L[r]]
            assert want.size == L[r], "a read leaves its contig"
            if rev[r]:
                want = comp[want[::-1]]
            have = o["seq"][off[r]: off[r + 1]]
            d = np.flatnonzero(have != want)
            nm[r] = d.size
            if d.size:
                pos.append(d.astype(np.uint32)); ref.append(want[d]); alt.append(have[d])
                qual.append(o["qual"][off[r] + d])
    edit_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(nm, out=edit_off[1:])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    return {"nm": nm, "edit_off": edit_off, "edit_pos": cat(pos, np.uint32), "edit_ref": cat(ref, np.uint8),
            "edit_alt": cat(alt, np.uint8), "edit_qual": cat(qual, np.uint8)}


def assert_truth(got, want, what=""):
    for col in ("nm", "edit_off", "edit_pos", "edit_ref", "edit_alt", "edit_qual"):
        assert got[col].shape == want[col].shape, f"{what}: {col} has {got[col].shape}, the model {want[col].shape}"
        if not np.array_equal(got[col], want[col]):
            i = int(np.flatnonzero(got[col] != want[col])[0])
            raise AssertionError(f"{what}: {col} differs first at {i}: {got[col][i]} against {want[col][i]}")


def edits_text(t, r, qual_offset=33):
    """the `edits` field of the truth TSV for read r: `*` or pos:REF>ALT:Q joined by commas"""
    a, b = int(t["edit_off"][r]), int(t["edit_off"][r + 1])
    if a == b:
        return "*"
    return ",".join("%d:%s>%s:%d" % (int(t["edit_pos"][i]), chr(int(t["edit_ref"][i])), chr(int(t["edit_alt"][i])),
                                     int(t["edit_qual"][i]) - qual_offset) for i in range(a, b))
