"""Thin Python host over the C ABI (include/simmr_hip.h).

PyTorch is used only for device memory, streams and torch.distributed; every
byte of simulated read content is produced by the HIP kernels in
simmr_amd/csrc through libsimmr_hip.so.  No fallback path exists.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _abi
from ._abi import (ErrorProfilePOD, PlanInfo, Range, ReadsOut, SimmrError, U64_MAX)


def _torch():
    import torch  # deferred: importing the package must not need a GPU
    return torch


@dataclass
class Reads:
    """SoA replacement of Vec<SimulatedRead> (simulate.rs:27-75) in HBM.

    PE shards interleave mates: read r is mate (r & 1) of pair (r >> 1)."""
    seq: "object"
    qual: "object"
    seq_off: "object"
    start: "object"
    end: "object"
    contig: "object"
    genome: "object"
    read_id: "object"
    flags: "object"
    n_reads: int
    total_bases: int
    qual_offset: int = 0
    slot_bytes: int = 0  # 0: compact streams; 16: SIMMR_SLOT16 (include/simmr_hip.h, simmr_reads_out)

    @classmethod
    def allocate(cls, n_reads: int, total_bases: int, device, qual_offset: int = 0, slot_bytes: int = 0) -> "Reads":
        torch = _torch()
        n = max(int(n_reads), 1)
        # the library needs exactly total_bases bytes (include/simmr_hip.h); the slack only keeps torch views of
        # whole 16-byte rows possible for the tests' checksums
        nb = (int(total_bases) + 15) // 16 * 16 + 16
        return cls(
            seq=torch.empty(nb, dtype=torch.uint8, device=device),
            qual=torch.empty(nb, dtype=torch.uint8, device=device),
            seq_off=torch.empty(n + 1, dtype=torch.int64, device=device),
            start=torch.empty(n, dtype=torch.int64, device=device),
            end=torch.empty(n, dtype=torch.int64, device=device),
            contig=torch.empty(n, dtype=torch.int32, device=device),
            genome=torch.empty(n, dtype=torch.int32, device=device),
            read_id=torch.empty(n, dtype=torch.int32, device=device),
            flags=torch.empty(n, dtype=torch.uint8, device=device),
            n_reads=int(n_reads), total_bases=int(total_bases), qual_offset=int(qual_offset),
            slot_bytes=int(slot_bytes))

    def pod(self) -> ReadsOut:
        o = ReadsOut()
        o.seq = self.seq.data_ptr()
        o.qual = self.qual.data_ptr()
        o.seq_off = self.seq_off.data_ptr()
        o.start = self.start.data_ptr()
        o.end = self.end.data_ptr()
        o.contig = self.contig.data_ptr()
        o.genome = self.genome.data_ptr()
        o.read_id = self.read_id.data_ptr()
        o.flags = self.flags.data_ptr()
        o.seq_capacity = self.seq.numel()
        o.reads_capacity = self.start.numel()
        o.qual_offset = self.qual_offset
        o.slot_bytes = self.slot_bytes
        return o

    def to_host(self) -> dict:
        """numpy copies, trimmed to the planned sizes.  Reads emitted into 16-byte slots (SIMMR_SLOT16) come back in
        the compact form — seq / qual without the padding, CSR seq_off — so that a consumer sees one layout; the
        columns as they lie in HBM are `raw_to_host()`."""
        h = self.raw_to_host()
        if self.slot_bytes != 16:
            return h
        n = self.n_reads
        a, b = h["start"].astype(np.int64), h["end"].astype(np.int64)
        L = np.abs(b - a)                                   # a read's length in this layout
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(L, out=off[1:])
        first = h["seq_off"][:n].astype(np.int64)           # first base; the qualities start at first & ~15
        within = np.arange(int(off[n]), dtype=np.int64) - np.repeat(off[:n], L)
        h["seq"] = h["seq"][np.repeat(first, L) + within]
        h["qual"] = h["qual"][np.repeat(first & ~np.int64(15), L) + within]
        h["seq_off"] = off.astype(np.uint64)
        return h

    def raw_to_host(self) -> dict:
        n, tb = self.n_reads, self.total_bases
        return {
            "seq": self.seq[:tb].cpu().numpy(),
            "qual": self.qual[:tb].cpu().numpy(),
            "seq_off": self.seq_off[: n + 1].cpu().numpy().astype(np.uint64),
            "start": self.start[:n].cpu().numpy().astype(np.uint64),
            "end": self.end[:n].cpu().numpy().astype(np.uint64),
            "contig": self.contig[:n].cpu().numpy().astype(np.uint32),
            "genome": self.genome[:n].cpu().numpy().astype(np.uint32),
            "read_id": self.read_id[:n].cpu().numpy().astype(np.uint32),
            "flags": self.flags[:n].cpu().numpy(),
        }


@dataclass
class Truth:
    """Ground truth per read (simmr_truth_plan / simmr_truth_emit) in HBM: nm[r] altered bases of read r, and their CSR
    edit lists — offset in the read as written, the base the unaltered read would carry, the base it carries, and the
    byte of qual[] there."""
    nm: "object"
    edit_off: "object"
    edit_pos: "object"
    edit_ref: "object"
    edit_alt: "object"
    edit_qual: "object"
    n_reads: int
    n_edits: int

    def pod(self) -> "_abi.TruthOut":
        return _abi.TruthOut(self.nm.data_ptr(), self.edit_off.data_ptr(), self.edit_pos.data_ptr(), self.edit_ref.data_ptr(),
                             self.edit_alt.data_ptr(), self.edit_qual.data_ptr(), self.n_reads, self.n_edits)

    def to_host(self) -> dict:
        n, m = self.n_reads, self.n_edits
        return {
            "nm": self.nm[:n].cpu().numpy().astype(np.uint32),
            "edit_off": self.edit_off[: n + 1].cpu().numpy().astype(np.uint64),
            "edit_pos": self.edit_pos[:m].cpu().numpy().astype(np.uint32),
            "edit_ref": self.edit_ref[:m].cpu().numpy(),
            "edit_alt": self.edit_alt[:m].cpu().numpy(),
            "edit_qual": self.edit_qual[:m].cpu().numpy(),
        }


class Mapeval:
    """An aligner's SAM scored against the true alignments on the device (simmr_mapeval_*, include/simmr_hip.h states the rules).
    truth_add() the truth text, truth_plan(), add() the aligner's text, then read() and entries().  A text is bytes (copied up) or a
    contiguous CUDA uint8 tensor; the adds only enqueue, so every text is kept until a call that synchronises."""

    def __init__(self, engine: "Engine", names, min_overlap_pct: int = 10):
        self.engine, self.lib = engine, engine.lib
        self._texts = []
        h = C.c_void_p()
        engine._check(self.lib.simmr_mapeval_create(engine._h, C.byref(h)))
        self._h = h
        try:
            self.reset(names, min_overlap_pct)
        except Exception:
            self.close()
            raise

    def _check(self, rc: int):
        self.engine._check(rc)

    def reset(self, names, min_overlap_pct: int = 10):
        raw = [n if isinstance(n, bytes) else str(n).encode() for n in names]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        cfg = _abi.MapevalConfig(len(raw), int(min_overlap_pct), arr)
        try:
            self._check(self.lib.simmr_mapeval_reset(self._h, C.byref(cfg)))
        finally:
            self._texts = []  # the reset has synchronised

    def _text(self, text):
        torch = _torch()
        if isinstance(text, (bytes, bytearray, memoryview)):
            host = np.frombuffer(bytes(text), dtype=np.uint8)
            dev = self.engine.device
            text = torch.from_numpy(host.copy()).to(dev) if host.size else torch.empty(0, dtype=torch.uint8, device=dev)
        if text.dtype != torch.uint8 or not text.is_cuda or not text.is_contiguous():
            raise ValueError("a SAM text is bytes or a contiguous CUDA uint8 tensor")
        self._texts.append(text)
        n = int(text.numel())
        return C.c_void_p(text.data_ptr() if n else None), n

    def truth_add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_mapeval_truth_add(self._h, p, n))

    def truth_plan(self) -> int:
        n = C.c_uint64(0)
        try:
            self._check(self.lib.simmr_mapeval_truth_plan(self._h, C.byref(n)))
        finally:
            self._texts = []  # the plan has synchronised
        self.n_entries = int(n.value)
        return self.n_entries

    def add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_mapeval_add(self._h, p, n))

    def read(self):
        """(counts by the names of struct simmr_mapeval_counts, by_mapq as a (256, 2) uint64 array: correct, wrong)"""
        c = _abi.MapevalCounts()
        by = np.zeros((256, 2), dtype=np.uint64)
        try:
            self._check(self.lib.simmr_mapeval_read(self._h, C.byref(c), by.ctypes.data_as(C.POINTER(C.c_uint64))))
        finally:
            self._texts = []
        return {n: int(getattr(c, n)) for n in _abi.MAPEVAL_COUNTS}, by

    def entries(self):
        """(key uint64, best uint32, hits uint32) of every truth entry, ascending by key, as numpy arrays"""
        torch = _torch()
        n = getattr(self, "n_entries", 0)
        dev = self.engine.device
        key = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        best = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        hits = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        self._check(self.lib.simmr_mapeval_emit(self._h, C.c_void_p(key.data_ptr()), C.c_void_p(best.data_ptr()), C.c_void_p(hits.data_ptr()), n))
        self._texts = []
        return key[:n].cpu().numpy().view(np.uint64), best[:n].cpu().numpy().view(np.uint32), hits[:n].cpu().numpy().view(np.uint32)

    def last_ms(self) -> float:
        return self.engine._ms(self.lib.simmr_last_mapeval_ms, self._h)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.simmr_mapeval_destroy(self._h)  # synchronises the stream before it frees: enqueued adds have read their texts
            self._h = None
            self._texts = []
            if self in getattr(self.engine, "_mapevals", []):
                self.engine._mapevals.remove(self)


class OverlapEval:
    """An overlapper's PAF scored against the true overlaps on the device (simmr_ovleval_*, include/simmr_hip.h states the rules).
    truth_add() the truth text (what Engine.overlaps() gives), truth_plan(), add() the overlapper's text, then read() and pairs().
    A text is bytes (copied up) or a contiguous CUDA uint8 tensor; the adds only enqueue, so every text is kept until a call that
    synchronises."""

    def __init__(self, engine: "Engine", min_pct: int = 10):
        self.engine, self.lib = engine, engine.lib
        self._texts = []
        self.n_entries = self.n_reads = 0
        h = C.c_void_p()
        engine._check(self.lib.simmr_ovleval_create(engine._h, C.byref(h)))
        self._h = h
        try:
            self.reset(min_pct)
        except Exception:
            self.close()
            raise

    def _check(self, rc: int):
        self.engine._check(rc)

    def reset(self, min_pct: int = 10):
        if not 0 <= int(min_pct) < 2 ** 32:
            raise ValueError("min_pct is 1 .. 100")
        try:
            self._check(self.lib.simmr_ovleval_reset(self._h, int(min_pct)))
        finally:
            self._texts = []  # the reset has synchronised
        self.n_entries = self.n_reads = 0

    def _text(self, text):
        torch = _torch()
        if isinstance(text, (bytes, bytearray, memoryview)):
            host = np.frombuffer(bytes(text), dtype=np.uint8)
            dev = self.engine.device
            text = torch.from_numpy(host.copy()).to(dev) if host.size else torch.empty(0, dtype=torch.uint8, device=dev)
        if text.dtype != torch.uint8 or not text.is_cuda or not text.is_contiguous():
            raise ValueError("a PAF text is bytes or a contiguous CUDA uint8 tensor")
        self._texts.append(text)
        n = int(text.numel())
        return C.c_void_p(text.data_ptr() if n else None), n

    def truth_add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_ovleval_truth_add(self._h, p, n))

    def truth_plan(self):
        """(true pairs, distinct reads among them)"""
        n, r = C.c_uint64(0), C.c_uint64(0)
        self.n_entries = self.n_reads = 0
        try:
            self._check(self.lib.simmr_ovleval_truth_plan(self._h, C.byref(n), C.byref(r)))
        finally:
            self._texts = []  # the plan has synchronised
        self.n_entries, self.n_reads = int(n.value), int(r.value)
        return self.n_entries, self.n_reads

    def add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_ovleval_add(self._h, p, n))

    def read(self):
        """(counts by the names of struct simmr_ovleval_counts, by_len as a (41, 2) uint64 array: found, not found)"""
        c = _abi.OvlevalCounts()
        by = np.zeros((_abi.OVLEVAL_LEN_ROWS, 2), dtype=np.uint64)
        try:
            self._check(self.lib.simmr_ovleval_read(self._h, C.byref(c), by.ctypes.data_as(C.POINTER(C.c_uint64))))
        finally:
            self._texts = []
        return {n: int(getattr(c, n)) for n in _abi.OVLEVAL_COUNTS}, by

    def pairs(self):
        """The true pairs ascending by (key_a, key_b), as numpy arrays: key_a, key_b, ov (uint64), best, hits (uint32)"""
        torch = _torch()
        n, dev = self.n_entries, self.engine.device
        wide = [torch.zeros(max(n, 1), dtype=torch.int64, device=dev) for _ in range(3)]
        narrow = [torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for _ in range(2)]
        self._check(self.lib.simmr_ovleval_emit(self._h, *[C.c_void_p(t.data_ptr()) for t in wide + narrow], n))
        self._texts = []
        return tuple(t[:n].cpu().numpy().view(np.uint64) for t in wide) + tuple(t[:n].cpu().numpy().view(np.uint32) for t in narrow)

    def last_ms(self) -> float:
        return self.engine._ms(self.lib.simmr_last_ovleval_ms, self._h)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.simmr_ovleval_destroy(self._h)  # synchronises the stream before it frees: enqueued adds have read their texts
            self._h = None
            self._texts = []
            if self in getattr(self.engine, "_mapevals", []):
                self.engine._mapevals.remove(self)


class VcfEval:
    """A variant caller's VCF scored against the strain's sites on the device (simmr_vcfeval_*, include/simmr_hip.h states the
    rules).  truth_add() the truth text (the file of --strain-vcf), truth_plan(), add() the caller's text, then read() and sites().
    A text is bytes (copied up) or a contiguous CUDA uint8 tensor; the adds only enqueue, so every text is kept until a call that
    synchronises."""

    def __init__(self, engine: "Engine", names, use_filtered: bool = False):
        self.engine, self.lib = engine, engine.lib
        self._texts = []
        self.n_entries = 0
        h = C.c_void_p()
        engine._check(self.lib.simmr_vcfeval_create(engine._h, C.byref(h)))
        self._h = h
        try:
            self.reset(names, use_filtered)
        except Exception:
            self.close()
            raise

    def _check(self, rc: int):
        self.engine._check(rc)

    def reset(self, names, use_filtered: bool = False):
        raw = [n if isinstance(n, bytes) else str(n).encode() for n in names]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        cfg = _abi.VcfevalConfig(len(raw), 1 if use_filtered else 0, arr)
        try:
            self._check(self.lib.simmr_vcfeval_reset(self._h, C.byref(cfg)))
        finally:
            self._texts = []  # the reset has synchronised
        self.n_entries = 0

    _text = Mapeval._text

    def truth_add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_vcfeval_truth_add(self._h, p, n))

    def truth_plan(self) -> int:
        n = C.c_uint64(0)
        self.n_entries = 0
        try:
            self._check(self.lib.simmr_vcfeval_truth_plan(self._h, C.byref(n)))
        finally:
            self._texts = []  # the plan has synchronised
        self.n_entries = int(n.value)
        return self.n_entries

    def add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_vcfeval_add(self._h, p, n))

    def read(self):
        """(counts by the names of struct simmr_vcfeval_counts, by_qual as a (256, 2) uint64 array: correct, wrong, by_ad as a
        (33, 2) uint64 array: found, not found)"""
        c = _abi.VcfevalCounts()
        by_qual = np.zeros((256, 2), dtype=np.uint64)
        by_ad = np.zeros((_abi.VCFEVAL_AD_ROWS, 2), dtype=np.uint64)
        try:
            self._check(self.lib.simmr_vcfeval_read(self._h, C.byref(c), by_qual.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                    by_ad.ctypes.data_as(C.POINTER(C.c_uint64))))
        finally:
            self._texts = []
        return {n: int(getattr(c, n)) for n in _abi.VCFEVAL_COUNTS}, by_qual, by_ad

    def sites(self):
        """The truth entries ascending by key, as numpy arrays: key (uint64), alleles, ad, best, hits (uint32)"""
        torch = _torch()
        n, dev = self.n_entries, self.engine.device
        key = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        narrow = [torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for _ in range(4)]
        self._check(self.lib.simmr_vcfeval_emit(self._h, *[C.c_void_p(t.data_ptr()) for t in [key] + narrow], n))
        self._texts = []
        return (key[:n].cpu().numpy().view(np.uint64),) + tuple(t[:n].cpu().numpy().view(np.uint32) for t in narrow)

    def last_ms(self) -> float:
        return self.engine._ms(self.lib.simmr_last_vcfeval_ms, self._h)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.simmr_vcfeval_destroy(self._h)  # synchronises the stream before it frees: enqueued adds have read their texts
            self._h = None
            self._texts = []
            if self in getattr(self.engine, "_mapevals", []):
                self.engine._mapevals.remove(self)


class AsmEval:
    """An assembler's contigs scored against the gold-standard assembly on the device (simmr_asmeval_*, include/simmr_hip.h states
    the rules).  truth_add() the truth FASTA (the file of --gold-assembly), truth_plan(), add() the contigs, then read(), entries()
    and contigs().  A text is bytes (copied up) or a contiguous CUDA uint8 tensor and holds whole records; truth_add only enqueues,
    so every text is kept until a call that synchronises."""

    def __init__(self, engine: "Engine", genomes, k: int = 31, plain_search: bool = False):
        self.engine, self.lib = engine, engine.lib
        self._texts = []
        self.n_entries = self.n_genomes = 0
        h = C.c_void_p()
        engine._check(self.lib.simmr_asmeval_create(engine._h, C.byref(h)))
        self._h = h
        try:
            self.reset(genomes, k, plain_search)
        except Exception:
            self.close()
            raise

    def _check(self, rc: int):
        self.engine._check(rc)

    def reset(self, genomes, k: int = 31, plain_search: bool = False):
        raw = [n if isinstance(n, bytes) else str(n).encode() for n in genomes]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        cfg = _abi.AsmevalConfig(len(raw), int(k), 1 if plain_search else 0, arr)
        try:
            self._check(self.lib.simmr_asmeval_reset(self._h, C.byref(cfg)))
        finally:
            self._texts = []  # the reset has synchronised
        self.n_entries, self.n_genomes, self.k = 0, len(raw), int(k)

    _text = Mapeval._text

    def truth_add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_asmeval_truth_add(self._h, p, n))

    def truth_plan(self) -> int:
        n = C.c_uint64(0)
        self.n_entries = 0
        try:
            self._check(self.lib.simmr_asmeval_truth_plan(self._h, C.byref(n)))
        finally:
            self._texts = []  # the plan has synchronised
        self.n_entries = int(n.value)
        return self.n_entries

    def add(self, text):
        p, n = self._text(text)
        try:
            self._check(self.lib.simmr_asmeval_add(self._h, p, n))
        finally:
            self._texts = []  # the add has synchronised

    def read(self):
        """(counts by the names of struct simmr_asmeval_counts, by_genome as an (n_genomes + 1, 5) uint64 array: distinct,
        distinct_found, over, contigs, contig_bases; the last row is "shared")"""
        c = _abi.AsmevalCounts()
        by = np.zeros((self.n_genomes + 1, len(_abi.ASMEVAL_GENOME_COLS)), dtype=np.uint64)
        try:
            self._check(self.lib.simmr_asmeval_read(self._h, C.byref(c), by.ctypes.data_as(C.POINTER(C.c_uint64))))
        finally:
            self._texts = []
        return {n: int(getattr(c, n)) for n in _abi.ASMEVAL_COUNTS}, by

    def entries(self):
        """The distinct k-mers of the truth ascending by key, as numpy arrays: key (uint64), genome, mult, hits (uint32)"""
        torch = _torch()
        n, dev = self.n_entries, self.engine.device
        key = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        narrow = [torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for _ in range(3)]
        self._check(self.lib.simmr_asmeval_emit(self._h, *[C.c_void_p(t.data_ptr()) for t in [key] + narrow], n))
        self._texts = []
        return (key[:n].cpu().numpy().view(np.uint64),) + tuple(t[:n].cpu().numpy().view(np.uint32) for t in narrow)

    def n_contigs(self) -> int:
        n = C.c_uint64(0)
        rc = self.lib.simmr_asmeval_contigs(self._h, None, None, None, None, None, None, 0, C.byref(n))
        if rc not in (0, -34):  # (SIMMR_ERANGE: capacity 0 asks for the number alone)
            self._check(rc)
        return int(n.value)

    def contigs(self):
        """The contigs in row order, as numpy arrays: length (uint64), kmers, found, shared, top_genome, top_kmers (uint32)"""
        torch = _torch()
        n, dev = self.n_contigs(), self.engine.device
        length = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        narrow = [torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for _ in range(5)]
        self._check(self.lib.simmr_asmeval_contigs(self._h, *[C.c_void_p(t.data_ptr()) for t in [length] + narrow], n, None))
        self._texts = []
        return (length[:n].cpu().numpy().view(np.uint64),) + tuple(t[:n].cpu().numpy().view(np.uint32) for t in narrow)

    def ms(self):
        """(the device time of the unit's calls since the reset, the sort's share of the last plan), in ms"""
        a, b = C.c_float(), C.c_float()
        self._check(self.lib.simmr_last_asmeval_ms(self._h, C.byref(a), C.byref(b)))
        self._texts = []
        return a.value, b.value

    def close(self):
        if getattr(self, "_h", None):
            self.lib.simmr_asmeval_destroy(self._h)  # synchronises the stream before it frees: enqueued adds have read their texts
            self._h = None
            self._texts = []
            if self in getattr(self.engine, "_mapevals", []):
                self.engine._mapevals.remove(self)


class AsmMap:
    """An assembler's contigs placed on the gold-standard assembly on the device (simmr_asmmap_*, include/simmr_hip.h states the
    rules): anchors, collinear blocks and the breakpoints between them.  truth_add() the truth FASTA (the file of --gold-assembly),
    truth_plan(), add() the contigs, then read(), anchors(), blocks() and contigs().  A text is bytes (copied up) or a contiguous
    CUDA uint8 tensor and holds whole records; truth_add only enqueues, so every text is kept until a call that synchronises."""

    def __init__(self, engine: "Engine", genomes, k: int = 31, band: int = 64, relocation: int = 1000, min_anchors: int = 16):
        self.engine, self.lib = engine, engine.lib
        self._texts = []
        self.n_anchors = self.n_genomes = 0
        h = C.c_void_p()
        engine._check(self.lib.simmr_asmmap_create(engine._h, C.byref(h)))
        self._h = h
        try:
            self.reset(genomes, k, band, relocation, min_anchors)
        except Exception:
            self.close()
            raise

    def _check(self, rc: int):
        self.engine._check(rc)

    def reset(self, genomes, k: int = 31, band: int = 64, relocation: int = 1000, min_anchors: int = 16):
        raw = [n if isinstance(n, bytes) else str(n).encode() for n in genomes]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        cfg = _abi.AsmmapConfig(len(raw), int(k), int(band), int(relocation), int(min_anchors), arr)
        try:
            self._check(self.lib.simmr_asmmap_reset(self._h, C.byref(cfg)))
        finally:
            self._texts = []  # the reset has synchronised
        self.n_anchors, self.n_genomes, self.k = 0, len(raw), int(k)

    _text = Mapeval._text

    def truth_add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_asmmap_truth_add(self._h, p, n))

    def truth_plan(self) -> int:
        n = C.c_uint64(0)
        self.n_anchors = 0
        try:
            self._check(self.lib.simmr_asmmap_truth_plan(self._h, C.byref(n)))
        finally:
            self._texts = []  # the plan has synchronised
        self.n_anchors = int(n.value)
        return self.n_anchors

    def add(self, text):
        p, n = self._text(text)
        try:
            self._check(self.lib.simmr_asmmap_add(self._h, p, n))
        finally:
            self._texts = []  # the add has synchronised

    def read(self):
        """(counts by the names of struct simmr_asmmap_counts, by_genome as an (n_genomes, 5) uint64 array: truth_bases,
        truth_anchors, blocks, block_bases, longest_block)"""
        c = _abi.AsmmapCounts()
        by = np.zeros((self.n_genomes, len(_abi.ASMMAP_GENOME_COLS)), dtype=np.uint64)
        try:
            self._check(self.lib.simmr_asmmap_read(self._h, C.byref(c), by.ctypes.data_as(C.POINTER(C.c_uint64))))
        finally:
            self._texts = []
        return {n: int(getattr(c, n)) for n in _abi.ASMMAP_COUNTS}, by

    def anchors(self):
        """The anchor index ascending by key, as numpy arrays: key (uint64), t, p, o (uint32)"""
        torch = _torch()
        n, dev = self.n_anchors, self.engine.device
        key = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        narrow = [torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for _ in range(3)]
        self._check(self.lib.simmr_asmmap_anchors(self._h, *[C.c_void_p(t.data_ptr()) for t in [key] + narrow], n))
        self._texts = []
        return (key[:n].cpu().numpy().view(np.uint64),) + tuple(t[:n].cpu().numpy().view(np.uint32) for t in narrow)

    def n_blocks(self) -> int:
        n = C.c_uint64(0)
        self._check(self.lib.simmr_asmmap_blocks(self._h, None, 2 ** 64 - 1, C.byref(n)))  # (no column: the number alone, and no capacity to miss)
        return int(n.value)

    def blocks(self):
        """The blocks in row order, nine uint32 numpy arrays: contig, truth_record, strand, q_start, q_end, p_start, p_end, hits, join"""
        torch = _torch()
        n, dev = self.n_blocks(), self.engine.device
        cols = [torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for _ in _abi.ASMMAP_BLOCK_COLS]
        ptrs = (C.c_void_p * len(cols))(*[t.data_ptr() for t in cols])
        self._check(self.lib.simmr_asmmap_blocks(self._h, ptrs, n, None))
        self._texts = []
        return tuple(t[:n].cpu().numpy().view(np.uint32) for t in cols)

    def n_contigs(self) -> int:
        n = C.c_uint64(0)
        self._check(self.lib.simmr_asmmap_contigs(self._h, None, None, None, None, None, None, 2 ** 64 - 1, C.byref(n)))  # (no column: the number alone)
        return int(n.value)

    def contigs(self):
        """The contigs in row order, as numpy arrays: length (uint64), hits, blocks, first_block (uint32), block_bases (uint64),
        worst_join (uint32)"""
        torch = _torch()
        n, dev = self.n_contigs(), self.engine.device
        wide = [torch.zeros(max(n, 1), dtype=torch.int64, device=dev) for _ in range(2)]
        narrow = [torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for _ in range(4)]
        order = [wide[0], narrow[0], narrow[1], narrow[2], wide[1], narrow[3]]
        self._check(self.lib.simmr_asmmap_contigs(self._h, *[C.c_void_p(t.data_ptr()) for t in order], n, None))
        self._texts = []
        return tuple(t[:n].cpu().numpy().view(np.uint64 if t.dtype == torch.int64 else np.uint32) for t in order)

    def ms(self) -> float:
        """the device time of the unit's calls since the reset, in ms"""
        a = C.c_float()
        self._check(self.lib.simmr_last_asmmap_ms(self._h, C.byref(a)))
        self._texts = []
        return a.value

    def close(self):
        if getattr(self, "_h", None):
            self.lib.simmr_asmmap_destroy(self._h)  # synchronises the stream before it frees: enqueued adds have read their texts
            self._h = None
            self._texts = []
            if self in getattr(self.engine, "_mapevals", []):
                self.engine._mapevals.remove(self)


class BinEval:
    """A binner's contig bins scored against each contig's true genome on the device (simmr_bineval_*, include/simmr_hip.h states
    the rules).  truth_add() the truth text (the file of --eval-assembly-contigs), truth_plan(), add() the binner's assignment, then
    read(), bins(), cells() and contigs().  A text is bytes (copied up) or a contiguous CUDA uint8 tensor cut behind a line end;
    truth_add only enqueues, so every text is kept until a call that synchronises."""

    def __init__(self, engine: "Engine", genomes, hash_bits: int = 64):
        self.engine, self.lib = engine, engine.lib
        self._texts = []
        self.n_contigs = self.n_genomes = 0
        h = C.c_void_p()
        engine._check(self.lib.simmr_bineval_create(engine._h, C.byref(h)))
        self._h = h
        try:
            self.reset(genomes, hash_bits)
        except Exception:
            self.close()
            raise

    def _check(self, rc: int):
        self.engine._check(rc)

    def reset(self, genomes, hash_bits: int = 64):
        raw = [n if isinstance(n, bytes) else str(n).encode() for n in genomes]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        cfg = _abi.BinevalConfig(len(raw), int(hash_bits), arr)
        try:
            self._check(self.lib.simmr_bineval_reset(self._h, C.byref(cfg)))
        finally:
            self._texts = []  # the reset has synchronised
        self.n_contigs, self.n_genomes, self.hash_bits = 0, len(raw), int(hash_bits)

    _text = Mapeval._text

    def truth_add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_bineval_truth_add(self._h, p, n))

    def truth_plan(self) -> int:
        n = C.c_uint64(0)
        self.n_contigs = 0
        try:
            self._check(self.lib.simmr_bineval_truth_plan(self._h, C.byref(n)))
        finally:
            self._texts = []  # the plan has synchronised
        self.n_contigs = int(n.value)
        return self.n_contigs

    def add(self, text):
        p, n = self._text(text)  # (kept: the add waits in its middle, and its lookups read the text behind that wait)
        self._check(self.lib.simmr_bineval_add(self._h, p, n))

    def read(self):
        """(counts by the names of struct simmr_bineval_counts, by_genome as an (n_genomes + 1, 7) uint64 array: truth_contigs,
        truth_bases, assigned_contigs, assigned_bases, bins, best_bin, best_bases; the last row is "none")"""
        c = _abi.BinevalCounts()
        by = np.zeros((self.n_genomes + 1, len(_abi.BINEVAL_GENOME_COLS)), dtype=np.uint64)
        try:
            self._check(self.lib.simmr_bineval_read(self._h, C.byref(c), by.ctypes.data_as(C.POINTER(C.c_uint64))))
        finally:
            self._texts = []
        return {n: int(getattr(c, n)) for n in _abi.BINEVAL_COUNTS}, by

    def _columns(self, fn, wide):
        """the columns of one of the three tables as numpy arrays; wide[i]: column i is 64-bit"""
        torch = _torch()
        n = C.c_uint64(0)
        none = [None] * len(wide)
        rc = fn(self._h, *none, 0, C.byref(n))
        if rc not in (0, -34):  # (SIMMR_ERANGE: capacity 0 asks for the number alone)
            self._check(rc)
        n, dev = int(n.value), self.engine.device
        cols = [torch.zeros(max(n, 1), dtype=torch.int64 if w else torch.int32, device=dev) for w in wide]
        self._check(fn(self._h, *[C.c_void_p(t.data_ptr()) for t in cols], n, None))
        return tuple(t[:n].cpu().numpy().view(np.uint64 if w else np.uint32) for t, w in zip(cols, wide))

    def bins(self):
        """The bins of the last read in row order: contigs (uint32), bases, none_bases (uint64), first_record, top_genome (uint32),
        top_bases (uint64)"""
        return self._columns(self.lib.simmr_bineval_bins, (False, True, True, False, False, True))

    def cells(self):
        """The cells of the last read in (bin, genome) order: bin, genome, contigs (uint32), bases (uint64)"""
        return self._columns(self.lib.simmr_bineval_cells, (False, False, False, True))

    def contigs(self):
        """The truth contigs in truth order: genome (uint32), length (uint64), bin or 0xffffffff, records (uint32)"""
        return self._columns(self.lib.simmr_bineval_contigs, (False, True, False, False))

    def ms(self):
        """(the device time of the unit's calls since the reset, the sort's share of the last plan), in ms"""
        a, b = C.c_float(), C.c_float()
        self._check(self.lib.simmr_last_bineval_ms(self._h, C.byref(a), C.byref(b)))
        self._texts = []
        return a.value, b.value

    def close(self):
        if getattr(self, "_h", None):
            self.lib.simmr_bineval_destroy(self._h)  # synchronises the stream before it frees: enqueued adds have read their texts
            self._h = None
            self._texts = []
            if self in getattr(self.engine, "_mapevals", []):
                self.engine._mapevals.remove(self)


class TaxEval:
    """A read classifier's calls scored against each read's true genome on the device (simmr_taxeval_*, include/simmr_hip.h
    states the rules).  truth_add() the truth text (the file of --truth), truth_plan(), add() the classifier's per-read text, then
    read(), reads() and taxa().  A text is bytes (copied up) or a contiguous CUDA uint8 tensor; the adds only enqueue, so every
    text is kept until a call that synchronises."""

    def __init__(self, engine: "Engine", taxonomy, genomes):
        self.engine, self.lib = engine, engine.lib
        self._texts = []
        self.n_entries = self.n_nodes = 0
        self.genome_ids = []
        h = C.c_void_p()
        engine._check(self.lib.simmr_taxeval_create(engine._h, C.byref(h)))
        self._h = h
        try:
            self.reset(taxonomy, genomes)
        except Exception:
            self.close()
            raise

    def _check(self, rc: int):
        self.engine._check(rc)

    def reset(self, taxonomy, genomes):
        """`taxonomy`: (taxid, parent, rank) arrays of one length; `genomes`: a list of (genome_id, taxid)"""
        taxid, parent = (np.ascontiguousarray(a, dtype=np.uint32) for a in taxonomy[:2])
        rank = np.ascontiguousarray(taxonomy[2], dtype=np.uint8)
        if not (taxid.ndim == parent.ndim == rank.ndim == 1 and len(taxid) == len(parent) == len(rank)):
            raise ValueError("a taxonomy is three arrays of one length: taxid, parent, rank")
        raw = [g if isinstance(g, bytes) else str(g).encode() for g, _ in genomes]
        ids = (C.c_char_p * max(len(raw), 1))(*raw)
        gtax = np.array([int(t) for _, t in genomes], dtype=np.uint32)
        u32, u8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        cfg = _abi.TaxevalConfig(len(taxid), taxid.ctypes.data_as(u32), parent.ctypes.data_as(u32), rank.ctypes.data_as(u8), len(raw), ids,
                                 gtax.ctypes.data_as(u32))
        self.n_entries = self.n_nodes = 0
        try:
            self._check(self.lib.simmr_taxeval_reset(self._h, C.byref(cfg)))
        finally:
            self._texts = []  # the reset has synchronised
        self.n_nodes = len(taxid)
        self.genome_ids = sorted(raw)  # the genome row is the place in this order

    _text = Mapeval._text

    def lineage(self, taxid: int):
        """(the taxids of the node's ancestor-or-self at the 8 ranks, 0 where it has none; its depth)"""
        out, depth = (C.c_uint32 * _abi.TAXEVAL_RANKS)(), C.c_uint32(0)
        self._check(self.lib.simmr_taxeval_lineage(self._h, int(taxid), out, C.byref(depth)))
        return [int(v) for v in out], int(depth.value)

    def truth_add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_taxeval_truth_add(self._h, p, n))

    def truth_plan(self) -> int:
        n = C.c_uint64(0)
        self.n_entries = 0
        try:
            self._check(self.lib.simmr_taxeval_truth_plan(self._h, C.byref(n)))
        finally:
            self._texts = []  # the plan has synchronised
        self.n_entries = int(n.value)
        return self.n_entries

    def add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_taxeval_add(self._h, p, n))

    def read(self):
        """(counts by the names of struct simmr_taxeval_counts, by_rank as an (8, 5) uint64 array: the records by rank and class,
        reads_by_rank as an (8, 5) uint64 array: the truth entries by rank and best class)"""
        c = _abi.TaxevalCounts()
        by_rank = np.zeros((_abi.TAXEVAL_RANKS, _abi.TAXEVAL_CLASSES), dtype=np.uint64)
        reads_by_rank = np.zeros_like(by_rank)
        try:
            self._check(self.lib.simmr_taxeval_read(self._h, C.byref(c), by_rank.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                    reads_by_rank.ctypes.data_as(C.POINTER(C.c_uint64))))
        finally:
            self._texts = []
        return {n: int(getattr(c, n)) for n in _abi.TAXEVAL_COUNTS}, by_rank, reads_by_rank

    def reads(self):
        """The truth entries ascending by id, as numpy arrays: id (uint64), genome_row, mates, seen, hits (uint32)"""
        torch = _torch()
        n, dev = self.n_entries, self.engine.device
        key = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        narrow = [torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for _ in range(4)]
        self._check(self.lib.simmr_taxeval_emit(self._h, *[C.c_void_p(t.data_ptr()) for t in [key] + narrow], n))
        self._texts = []
        return (key[:n].cpu().numpy().view(np.uint64),) + tuple(t[:n].cpu().numpy().view(np.uint32) for t in narrow)

    def taxa(self):
        """One row per node in taxid order, as numpy arrays: taxid (uint32) and the clade sums true, called, both (uint64)"""
        torch = _torch()
        n, dev = self.n_nodes, self.engine.device
        taxid = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        wide = [torch.zeros(max(n, 1), dtype=torch.int64, device=dev) for _ in range(3)]
        self._check(self.lib.simmr_taxeval_taxa(self._h, *[C.c_void_p(t.data_ptr()) for t in [taxid] + wide], n))
        self._texts = []
        return (taxid[:n].cpu().numpy().view(np.uint32),) + tuple(t[:n].cpu().numpy().view(np.uint64) for t in wide)

    def last_ms(self) -> float:
        return self.engine._ms(self.lib.simmr_last_taxeval_ms, self._h)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.simmr_taxeval_destroy(self._h)  # synchronises the stream before it frees: enqueued adds have read their texts
            self._h = None
            self._texts = []
            if self in getattr(self.engine, "_mapevals", []):
                self.engine._mapevals.remove(self)


class CorrEval:
    """A read error corrector's output scored against the true reads on the device (simmr_correval_*, include/simmr_hip.h states the
    rules).  truth_add() the truth SAM text, truth_plan(), add() the corrected FASTQ (or two-line FASTA) in whole records, then read()
    and entries().  A text is bytes (copied up) or a contiguous CUDA uint8 tensor; the adds only enqueue, so every text is kept until
    a call that synchronises."""

    def __init__(self, engine: "Engine", lines_per_record: int = 4):
        self.engine, self.lib = engine, engine.lib
        self._texts = []
        h = C.c_void_p()
        engine._check(self.lib.simmr_correval_create(engine._h, C.byref(h)))
        self._h = h
        try:
            self.reset(lines_per_record)
        except Exception:
            self.close()
            raise

    def _check(self, rc: int):
        self.engine._check(rc)

    def reset(self, lines_per_record: int = 4):
        cfg = _abi.CorrevalConfig(int(lines_per_record), 0)
        try:
            self._check(self.lib.simmr_correval_reset(self._h, C.byref(cfg)))
        finally:
            self._texts = []  # the reset has synchronised

    _text = Mapeval._text

    def truth_add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_correval_truth_add(self._h, p, n))

    def truth_plan(self) -> int:
        n = C.c_uint64(0)
        try:
            self._check(self.lib.simmr_correval_truth_plan(self._h, C.byref(n)))
        finally:
            self._texts = []  # the plan has synchronised
        self.n_entries = int(n.value)
        return self.n_entries

    def add(self, text):
        p, n = self._text(text)
        self._check(self.lib.simmr_correval_add(self._h, p, n))

    def read(self):
        """(counts by the names of struct simmr_correval_counts, cube (5, 5, 5) [t][o][c], by_qual (95, 5), by_pos (512, 5)), uint64 arrays;
        the five columns are kept, damaged, fixed, left, miscorrected"""
        c = _abi.CorrevalCounts()
        cube = np.zeros((5, 5, 5), dtype=np.uint64)
        by_qual = np.zeros((_abi.CORREVAL_QUALS, 5), dtype=np.uint64)
        by_pos = np.zeros((_abi.CORREVAL_POS, 5), dtype=np.uint64)
        u64 = C.POINTER(C.c_uint64)
        try:
            self._check(self.lib.simmr_correval_read(self._h, C.byref(c), cube.ctypes.data_as(u64), by_qual.ctypes.data_as(u64), by_pos.ctypes.data_as(u64)))
        finally:
            self._texts = []
        return {n: int(getattr(c, n)) for n in _abi.CORREVAL_COUNTS}, cube, by_qual, by_pos

    def entries(self):
        """(key uint64, length, before, residual, hits uint32) of every truth entry, ascending by key, as numpy arrays"""
        torch = _torch()
        n = getattr(self, "n_entries", 0)
        dev = self.engine.device
        key = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        cols = [torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for _ in range(4)]
        self._check(self.lib.simmr_correval_emit(self._h, C.c_void_p(key.data_ptr()), *[C.c_void_p(c.data_ptr()) for c in cols], n))
        self._texts = []
        return (key[:n].cpu().numpy().view(np.uint64),) + tuple(c[:n].cpu().numpy().view(np.uint32) for c in cols)

    def last_ms(self) -> float:
        return self.engine._ms(self.lib.simmr_last_correval_ms, self._h)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.simmr_correval_destroy(self._h)  # synchronises the stream before it frees: enqueued adds have read their texts
            self._h = None
            self._texts = []
            if self in getattr(self.engine, "_mapevals", []):
                self.engine._mapevals.remove(self)


def cut_at_line_ends(text: bytes, pieces: int):
    """`text` in at most `pieces` parts of about one size, each cut behind a newline"""
    out, a = [], 0
    for i in range(1, pieces):
        b = text.find(b"\n", max(a, len(text) * i // pieces - 1)) + 1
        if b <= a:
            break
        out.append(text[a:b])
        a = b
    return out + [text[a:]]


class Engine:
    """One engine == one GPU == one host thread (include/simmr_hip.h)."""

    def __init__(self, device: int = 0):
        self.lib = _abi.load()
        h = C.c_void_p()
        rc = self.lib.simmr_engine_create(int(device), C.byref(h))
        if rc != 0:
            raise SimmrError(rc, (self.lib.simmr_last_error(None) or b"").decode())
        self._h = h
        self._fit_sam_texts = []  # SAM texts of fit_add_sam whose adds may still be enqueued
        self.device_index = int(device)
        self._keep = []

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            for m in list(getattr(self, "_mapevals", [])):  # (their state lives on the engine: they go first)
                m.close()
            if getattr(self, "_bam_sort", None):  # (the sorted-BAM state lives on the engine: it goes first)
                self.lib.simmr_bam_sort_destroy(self._bam_sort)
                self._bam_sort = None
            self.lib.simmr_engine_destroy(self._h)  # synchronises the device before it frees: enqueued adds have read their texts
            self._h = None
            self._fit_sam_texts = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise SimmrError(rc, (self.lib.simmr_last_error(self._h) or b"").decode())

    def _ms(self, fn, handle=None) -> float:
        """what a simmr_last_*_ms call answers (`handle`: the object it is asked of, the engine by default)"""
        ms = C.c_float()
        self._check(fn(self._h if handle is None else handle, C.byref(ms)))
        return ms.value

    @property
    def device(self):
        return _torch().device("cuda", self.device_index)

    def use_current_torch_stream(self):
        s = _torch().cuda.current_stream(self.device)
        self._check(self.lib.simmr_engine_set_stream(self._h, C.c_void_p(s.cuda_stream)))

    def set_read_slots(self, slot_bytes: int):
        """Layout of the reads that plans made from now on emit: 0 compact, 16 = SIMMR_SLOT16 (simmr_engine_set_read_slots).
        The setting is the ENGINE's and it sticks: simmr_amd.simulate's entry points select SIMMR_SLOT16 and leave it
        selected, so direct pe_plan / long_plan calls made on the same engine afterwards also get the slot layout, in which
        seq_off[r + 1] - seq_off[r] is not read r's length (PlanInfo.slot_bytes / Reads.slot_bytes say which layout a plan
        emits; the C ABI's own default is compact)."""
        self._check(self.lib.simmr_engine_set_read_slots(self._h, int(slot_bytes)))

    def set_plan_overlap(self, on: bool):
        """The plan of the next shard beside the emit of this one (simmr_engine_set_plan_overlap): plan calls on a stream
        of the engine's own, into a second set of the plan buffers."""
        self._check(self.lib.simmr_engine_set_plan_overlap(self._h, 1 if on else 0))

    # -- staging ------------------------------------------------------------
    def stage_genome(self, genome_idx: int, contigs: Sequence, sizes: Optional[Sequence[int]] = None):
        """contigs: normalised ASCII sequences (bytes or uint8 arrays), Seq.seq
        of genome.rs:17-23; sizes: Seq.size when it differs (--contiguous)."""
        arrs = [np.ascontiguousarray(np.frombuffer(c, dtype=np.uint8) if isinstance(c, (bytes, bytearray))
                                     else np.asarray(c, dtype=np.uint8)) for c in contigs]
        n = len(arrs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        lens = (C.c_uint64 * n)(*[a.size for a in arrs])
        szs = (C.c_uint64 * n)(*[int(s) for s in sizes]) if sizes is not None else None
        self._check(self.lib.simmr_stage_genome(self._h, genome_idx, n, ptrs, lens, szs))

    def stage_fasta(self, genome_idx: int, bodies: Sequence[bytes], contiguous: bool = False, min_size: int = 0):
        """Raw FASTA record bodies (the bytes between a header line and the next header) -> staged genome;
        normalisation (needletail normalize(false), genome.rs:114) and packing happen on the device.
        Returns (bases per record, number of sequences staged)."""
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) for b in bodies]
        n = len(arrs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data if a.size else None for a in arrs])
        lens = (C.c_uint64 * n)(*[a.size for a in arrs])
        counts = (C.c_uint64 * n)()
        staged = C.c_uint32(0)
        self._check(self.lib.simmr_stage_fasta(self._h, genome_idx, n, ptrs, lens, 1 if contiguous else 0, int(min_size),
                                               counts, C.byref(staged)))
        return [int(x) for x in counts], int(staged.value)

    def stage_synthetic(self, genome_idx: int, contig_lens: Sequence[int], splitmix_seed: int):
        n = len(contig_lens)
        lens = (C.c_uint64 * n)(*[int(x) for x in contig_lens])
        self._check(self.lib.simmr_stage_synthetic(self._h, genome_idx, n, lens, C.c_uint64(splitmix_seed)))

    def unstage(self, genome_idx: int, contig: int, first: int, count: int) -> np.ndarray:
        out = np.empty(count, dtype=np.uint8)
        self._check(self.lib.simmr_unstage_contig(self._h, genome_idx, contig, first, count,
                                                  C.c_void_p(out.ctypes.data)))
        return out

    def genome_info(self, genome_idx: int):
        n = C.c_uint32()
        t = C.c_uint64()
        self._check(self.lib.simmr_genome_info(self._h, genome_idx, C.byref(n), C.byref(t)))
        return n.value, t.value

    # -- paired-end (simulate.rs:165-302) -------------------------------------
    def pe_plan(self, genome_idx: int, profile: ErrorProfilePOD, genome_reads: int,
                seed: Optional[int], first: int = 0, count: int = U64_MAX,
                start: Tuple[int, int] = (0, 0)) -> PlanInfo:
        """`start` = (slot, pair): a known position of the genome's outer stream at or before
        `first` (see simulate.seek_outer_stream); (0, 0) walks the stream from its beginning."""
        info = PlanInfo()
        if start == (0, 0):
            self._check(self.lib.simmr_pe_plan(self._h, genome_idx, C.byref(profile), genome_reads,
                                               0 if seed is None else 1, 0 if seed is None else seed,
                                               Range(first, count), C.byref(info)))
        else:
            if seed is None:
                raise ValueError("seeking needs a seed")
            self._check(self.lib.simmr_pe_plan_at(self._h, genome_idx, C.byref(profile), genome_reads, seed,
                                                  Range(first, count), start[0], start[1], C.byref(info)))
        return info

    def outer_summarize(self, genome_idx: int, seed: int, slot_first: int, slot_count: int):
        """(units0, units1, end0, end1) of slots [slot_first, slot_first + slot_count) of the genome's
        outer stream (simulate.rs:172-184), see include/simmr_hip.h."""
        s = _abi.OuterSummary()
        self._check(self.lib.simmr_outer_summarize(self._h, genome_idx, seed, slot_first, slot_count, C.byref(s)))
        return int(s.units[0]), int(s.units[1]), int(s.end_state[0]), int(s.end_state[1])

    def pe_plan_multi(self, genome_idx: Sequence[int], genome_reads: Sequence[int], profile: ErrorProfilePOD,
                      seed: Optional[int], first: int = 0, count: int = U64_MAX) -> PlanInfo:
        """simulate_pe_reads over several genomes in one plan; [first, first + count) is a range of the
        global pair index (genomes concatenated in order)."""
        n = len(genome_idx)
        gi = (C.c_uint32 * n)(*[int(x) for x in genome_idx])
        gr = (C.c_uint64 * n)(*[int(x) for x in genome_reads])
        info = PlanInfo()
        self._check(self.lib.simmr_pe_plan_multi(self._h, n, gi, gr, C.byref(profile), 0 if seed is None else 1,
                                                 0 if seed is None else seed, Range(first, count), C.byref(info)))
        return info

    def simulate_pe_reads_multi(self, genome_idx, genome_reads, profile, seed, first=0, count=U64_MAX,
                                qual_offset=0) -> Reads:
        info = self.pe_plan_multi(genome_idx, genome_reads, profile, seed, first, count)
        out = Reads.allocate(info.n_reads, info.total_bases, self.device, qual_offset, info.slot_bytes)
        self.pe_emit(0, out)
        return out

    def pe_emit(self, read_id_base: int, out: Reads):
        pod = out.pod()
        self._check(self.lib.simmr_pe_emit(self._h, read_id_base, C.byref(pod)))

    def simulate_pe_reads_from_genome(self, genome_idx: int, profile: ErrorProfilePOD, genome_reads: int,
                                      seed: Optional[int], first: int = 0, count: int = U64_MAX,
                                      read_id_base: int = 0, qual_offset: int = 0,
                                      start: Tuple[int, int] = (0, 0)) -> Reads:
        info = self.pe_plan(genome_idx, profile, genome_reads, seed, first, count, start)
        out = Reads.allocate(info.n_reads, info.total_bases, self.device, qual_offset, info.slot_bytes)
        self.pe_emit(read_id_base, out)
        return out

    # -- long reads (simulate.rs:323-523) --------------------------------------
    def long_plan(self, genome_idx: Sequence[int], genome_reads: Sequence[int], profile: ErrorProfilePOD,
                  seed: Optional[int], first: int = 0, count: int = U64_MAX) -> PlanInfo:
        n = len(genome_idx)
        gi = (C.c_uint32 * n)(*[int(x) for x in genome_idx])
        gr = (C.c_uint64 * n)(*[int(x) for x in genome_reads])
        info = PlanInfo()
        self._check(self.lib.simmr_long_plan(self._h, n, gi, gr, C.byref(profile),
                                             0 if seed is None else 1, 0 if seed is None else seed,
                                             Range(first, count), C.byref(info)))
        return info

    def long_emit(self, read_id_base: int, out: Reads):
        pod = out.pod()
        self._check(self.lib.simmr_long_emit(self._h, read_id_base, C.byref(pod)))

    def simulate_long_reads(self, genome_idx, genome_reads, profile, seed, first=0, count=U64_MAX,
                            read_id_base=0, qual_offset=0) -> Reads:
        info = self.long_plan(genome_idx, genome_reads, profile, seed, first, count)
        out = Reads.allocate(info.n_reads, info.total_bases, self.device, qual_offset, info.slot_bytes)
        self.long_emit(read_id_base, out)
        return out

    # -- FASTQ framing (fastq.rs:14-124) ------------------------------------------
    def fastq(self, reads: Reads, header_format: str, names, paired: bool):
        """FASTQ text of `reads` as a CUDA uint8 tensor.  `names` = [(engine genome slot, genome id,
        [sequence id per contig]), ...]; qualities must have been emitted with qual_offset=33.
        Raises SimmrError(ENOTSUP) for the cases the library leaves to the host writer."""
        torch = _torch()
        fn = self._fastq_names(names)
        pod = reads.pod()
        total = C.c_uint64(0)
        self._check(self.lib.simmr_fastq_plan(self._h, header_format.encode(), C.byref(fn), C.byref(pod),
                                              reads.n_reads, 1 if paired else 0, C.byref(total)))
        out = torch.empty(max(total.value, 1), dtype=torch.uint8, device=self.device)
        self._check(self.lib.simmr_fastq_emit(self._h, C.byref(pod), C.c_void_p(out.data_ptr()), total.value))
        return out[: total.value]

    def _fastq_names(self, names):
        n = len(names)
        gi = (C.c_uint32 * max(n, 1))(*[int(x[0]) for x in names])
        gid = (C.c_char_p * max(n, 1))(*[str(x[1]).encode() for x in names])
        nc = (C.c_uint32 * max(n, 1))(*[len(x[2]) for x in names])
        flat = [str(sid).encode() for x in names for sid in x[2]]
        sids = (C.c_char_p * max(len(flat), 1))(*flat)
        fn = _abi.FastqNames(n, gi, gid, nc, sids)
        fn._keep = (gi, gid, nc, sids)
        return fn

    def fastq_plan_direct(self, header_format: str, names, read_id_base: int = 0) -> int:
        """Sizes the FASTQ text of the CURRENT plan's shard (simmr_fastq_plan_direct); returns its bytes."""
        fn = self._fastq_names(names)
        total = C.c_uint64(0)
        self._check(self.lib.simmr_fastq_plan_direct(self._h, header_format.encode(), C.byref(fn), int(read_id_base),
                                                     C.byref(total)))
        return int(total.value)

    def emit_fastq(self, out):
        """Writes the text planned by fastq_plan_direct into the CUDA uint8 tensor `out` (simmr_emit_fastq)."""
        self._check(self.lib.simmr_emit_fastq(self._h, C.c_void_p(out.data_ptr()), int(out.numel())))

    def fastq_direct(self, header_format: str, names, read_id_base: int = 0):
        """FASTQ text of the current plan's shard without the columns in between, as a CUDA uint8 tensor."""
        torch = _torch()
        total = self.fastq_plan_direct(header_format, names, read_id_base)
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)
        self.emit_fastq(out)
        return out[:total]

    def last_fastq_plan_ms(self) -> float:
        return self._ms(self.lib.simmr_last_fastq_plan_ms)

    # -- ground truth per read ------------------------------------------------------
    def truth_plan(self, reads: Reads) -> int:
        """Counts the edits of `reads` against the staged genomes (simmr_truth_plan); returns their total."""
        pod = reads.pod()
        total = C.c_uint64(0)
        self._check(self.lib.simmr_truth_plan(self._h, C.byref(pod), reads.n_reads, C.byref(total)))
        return int(total.value)

    def truth(self, reads: Reads) -> Truth:
        """Mismatch counts and edit lists of `reads` as CUDA tensors (simmr_truth_plan + simmr_truth_emit)."""
        torch = _torch()
        m = self.truth_plan(reads)
        n = reads.n_reads
        t = Truth(nm=torch.empty(max(n, 1), dtype=torch.int32, device=self.device),
                  edit_off=torch.empty(n + 1, dtype=torch.int64, device=self.device),
                  edit_pos=torch.empty(max(m, 1), dtype=torch.int32, device=self.device),
                  edit_ref=torch.empty(max(m, 1), dtype=torch.uint8, device=self.device),
                  edit_alt=torch.empty(max(m, 1), dtype=torch.uint8, device=self.device),
                  edit_qual=torch.empty(max(m, 1), dtype=torch.uint8, device=self.device),
                  n_reads=n, n_edits=m)
        out = t.pod()
        pod = reads.pod()
        self._check(self.lib.simmr_truth_emit(self._h, C.byref(pod), C.byref(out)))
        return t

    def last_truth_ms(self) -> float:
        return self._ms(self.lib.simmr_last_truth_ms)

    # -- the true alignments as SAM text ---------------------------------------------
    def _sam_names(self, rnames):
        n = len(rnames)
        gi = (C.c_uint32 * max(n, 1))(*[int(x[0]) for x in rnames])
        nc = (C.c_uint32 * max(n, 1))(*[len(x[1]) for x in rnames])
        flat = [str(name).encode() for x in rnames for name in x[1]]
        names = (C.c_char_p * max(len(flat), 1))(*flat)
        sn = _abi.SamNames(n, gi, nc, names)
        sn._keep = (gi, nc, names)
        return sn

    def sam(self, reads: Reads, rnames, paired: bool, truth: Optional[Truth] = None):
        """The alignment lines of `reads` (simmr_sam_plan + simmr_sam_emit) as a CUDA uint8 tensor, without a header
        (simmr_amd.sam.sam_header writes one).  `rnames` = [(engine genome slot, [RNAME per contig]), ...]; the reads
        must have been emitted with qual_offset=33.  `truth`: what Engine.truth(reads) returned; made here if None."""
        torch = _torch()
        t = truth if truth is not None else self.truth(reads)
        out = t.pod()
        sn = self._sam_names(rnames)
        pod = reads.pod()
        total = C.c_uint64(0)
        self._check(self.lib.simmr_sam_plan(self._h, C.byref(sn), C.byref(pod), C.byref(out), reads.n_reads,
                                            1 if paired else 0, C.byref(total)))
        text = torch.empty(max(total.value, 1), dtype=torch.uint8, device=self.device)
        self._check(self.lib.simmr_sam_emit(self._h, C.byref(pod), C.byref(out), C.c_void_p(text.data_ptr()), total.value))
        return text[: total.value]

    def last_sam_ms(self) -> float:
        return self._ms(self.lib.simmr_last_sam_ms)

    def sam_sorted(self, reads: Reads, rnames, paired: bool, truth: Optional[Truth] = None, with_keys: bool = False):
        """The alignment lines of Engine.sam() in coordinate order (simmr_sam_sort_plan + simmr_sam_sort_emit): ascending by
        (index of the contig in `rnames`, leftmost position), ties in read order.  Returns the text tensor; with `with_keys`
        (text, key, line_off): CUDA int64 tensors holding the key (row << 40 | lo) of every line written and the lines'
        offsets (n_reads + 1)."""
        torch = _torch()
        t = truth if truth is not None else self.truth(reads)
        out = t.pod()
        sn = self._sam_names(rnames)
        pod = reads.pod()
        total = C.c_uint64(0)
        self._check(self.lib.simmr_sam_sort_plan(self._h, C.byref(sn), C.byref(pod), C.byref(out), reads.n_reads,
                                                 1 if paired else 0, C.byref(total)))
        text = torch.empty(max(total.value, 1), dtype=torch.uint8, device=self.device)
        key = torch.empty(max(reads.n_reads, 1), dtype=torch.int64, device=self.device) if with_keys else None
        line_off = torch.empty(reads.n_reads + 1, dtype=torch.int64, device=self.device) if with_keys else None
        self._check(self.lib.simmr_sam_sort_emit(self._h, C.byref(pod), C.byref(out), C.c_void_p(text.data_ptr()), total.value,
                                                 C.c_void_p(key.data_ptr()) if with_keys else None,
                                                 C.c_void_p(line_off.data_ptr()) if with_keys else None))
        if with_keys:
            return text[: total.value], key[: reads.n_reads], line_off
        return text[: total.value]

    def last_sam_sort_ms(self) -> float:
        return self._ms(self.lib.simmr_last_sam_sort_ms)

    # -- the true alignments as BAM records, and BGZF framing ------------------------------
    def bam(self, reads: Reads, rnames, paired: bool, truth: Optional[Truth] = None, framed: bool = True):
        """The BAM records of `reads` in read order (simmr_bam_plan + simmr_bam_emit) as a CUDA uint8 tensor: back to back,
        or with `framed` their BGZF blocks (Engine.bgzf).  Arguments as Engine.sam().  A file is Engine.bgzf of
        simmr_amd.sam.bam_header(...), these blocks, and simmr_amd.sam.BGZF_EOF."""
        torch = _torch()
        t = truth if truth is not None else self.truth(reads)
        out = t.pod()
        sn = self._sam_names(rnames)
        pod = reads.pod()
        total = C.c_uint64(0)
        self._check(self.lib.simmr_bam_plan(self._h, C.byref(sn), C.byref(pod), C.byref(out), reads.n_reads,
                                            1 if paired else 0, C.byref(total)))
        rec = torch.empty(max(total.value, 1), dtype=torch.uint8, device=self.device)
        self._check(self.lib.simmr_bam_emit(self._h, C.byref(pod), C.byref(out), C.c_void_p(rec.data_ptr()), total.value))
        return self.bgzf(rec[: total.value]) if framed else rec[: total.value]

    def last_bam_ms(self) -> float:
        return self._ms(self.lib.simmr_last_bam_ms)

    def bgzf(self, data):
        """The bytes of a contiguous CUDA uint8 tensor as BGZF blocks with stored deflate blocks (simmr_bgzf_frame), without the
        end-of-file block (simmr_amd.sam.BGZF_EOF)."""
        torch = _torch()
        if data.dtype != torch.uint8 or not data.is_cuda or not data.is_contiguous():
            raise ValueError("Engine.bgzf takes a contiguous CUDA uint8 tensor")
        n = data.numel()
        bound = self.lib.simmr_bgzf_bound(n)
        dst = torch.empty(max(bound, 1), dtype=torch.uint8, device=self.device)
        written = C.c_uint64(0)
        self._check(self.lib.simmr_bgzf_frame(self._h, C.c_void_p(data.data_ptr()), n, C.c_void_p(dst.data_ptr()), bound, C.byref(written)))
        return dst[: written.value]

    # -- the BAM records in coordinate order, and the BAI index ---------------------------
    def _bam_sort_handle(self):
        """the state object of simmr_bam_sort_* / simmr_bai_*, made on first use and destroyed by close() before the engine"""
        if getattr(self, "_bam_sort", None) is None:
            h = C.c_void_p()
            self._check(self.lib.simmr_bam_sort_create(self._h, C.byref(h)))
            self._bam_sort = h
        return self._bam_sort

    def bam_sorted(self, reads: Reads, rnames, paired: bool, truth: Optional[Truth] = None, index: bool = True):
        """A coordinate-sorted BAM and its BAI index (simmr_bam_sort_plan / _emit, simmr_bgzf_frame, simmr_bai_plan / _emit) as
        two CUDA uint8 tensors (blocks, bai).  `blocks` holds simmr_amd.sam.bam_header(..., "coordinate") and the records of
        Engine.bam() in the order of Engine.sam_sorted(), framed as ONE stream: blocks + simmr_amd.sam.BGZF_EOF is the file,
        `bai` its index (None with index=False).  Arguments as Engine.sam()."""
        from . import sam as _sam_py
        torch = _torch()
        t = truth if truth is not None else self.truth(reads)
        out = t.pod()
        h = self._bam_sort_handle()
        sn = self._sam_names(rnames)
        pod = reads.pod()
        n = reads.n_reads
        total = C.c_uint64(0)
        self._check(self.lib.simmr_bam_sort_plan(h, C.byref(sn), C.byref(pod), C.byref(out), n, 1 if paired else 0, C.byref(total)))
        flat = [str(name) for x in rnames for name in x[1]]
        lens = (C.c_uint64 * max(len(flat), 1))()
        n_rows = C.c_uint64(0)
        self._check(self.lib.simmr_bam_sort_ref_lengths(h, lens, len(flat), C.byref(n_rows)))
        lengths = [int(lens[i]) for i in range(n_rows.value)]
        header = _sam_py.bam_header(flat, lengths, "coordinate")
        base = len(header)
        stream = torch.empty(base + total.value, dtype=torch.uint8, device=self.device)
        stream[:base] = torch.frombuffer(bytearray(header), dtype=torch.uint8).to(self.device)
        key = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        end = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        rec_off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        self._check(self.lib.simmr_bam_sort_emit(h, C.byref(pod), C.byref(out), C.c_void_p(stream.data_ptr() + base), total.value,
                                                 C.c_void_p(key.data_ptr()), C.c_void_p(rec_off.data_ptr()), C.c_void_p(end.data_ptr())))
        blocks = self.bgzf(stream)
        if not index:
            return blocks, None
        return blocks, self.bai(key[:n], end[:n], rec_off, len(flat), base, ref_len=lengths)

    def last_bam_sort_ms(self) -> float:
        if getattr(self, "_bam_sort", None) is None:
            raise SimmrError(_abi.ESTATE, "no simmr_bam_sort_plan yet")
        return self._ms(self.lib.simmr_last_bam_sort_ms, self._bam_sort)

    def bai(self, key, end, rec_off, n_ref: int, base: int, ref_len=None):
        """The BAI index (simmr_bai_plan + simmr_bai_emit) of a coordinate-sorted record stream held as CUDA columns: key (int64,
        row << 40 | lo, ascending), end (int32, exclusive), rec_off (int64, one entry more: the records' offsets behind the
        `base` uncompressed bytes of the header).  The stream must have been framed as one (Engine.bgzf of header + records).
        `ref_len`: the references' lengths if known (one of 2^29 bases or more is refused).  Returns a CUDA uint8 tensor."""
        torch = _torch()
        n = int(key.numel())
        for col, dt, m in ((key, torch.int64, n), (end, torch.int32, n), (rec_off, torch.int64, n + 1)):
            if col.dtype != dt or not col.is_cuda or not col.is_contiguous() or col.numel() != m:
                raise ValueError("Engine.bai takes contiguous CUDA columns: key int64[n], end int32[n], rec_off int64[n + 1]")
        lens = None
        if ref_len is not None:
            if len(ref_len) != n_ref:
                raise ValueError("ref_len has one entry per reference")
            lens = (C.c_uint64 * max(n_ref, 1))(*[int(x) for x in ref_len])
        h = self._bam_sort_handle()
        total = C.c_uint64(0)
        self._check(self.lib.simmr_bai_plan(h, C.c_void_p(key.data_ptr()) if n else None, C.c_void_p(end.data_ptr()) if n else None,
                                            C.c_void_p(rec_off.data_ptr()), n, int(n_ref), lens, int(base), C.byref(total)))
        dst = torch.empty(total.value, dtype=torch.uint8, device=self.device)
        self._check(self.lib.simmr_bai_emit(h, C.c_void_p(dst.data_ptr()), total.value))
        return dst

    # -- the true read-to-read overlaps as PAF ------------------------------------------
    OVERLAP_COLUMNS = (("a", np.uint32), ("b", np.uint32), ("ref_start", np.uint64), ("ref_end", np.uint64), ("row", np.uint32))

    def overlap_reset(self, paired: bool):
        """Drops the reads accumulated for the overlap pass and fixes the rows to the genomes staged now (simmr_overlap_reset);
        `paired`: every add carries interleaved mates, named <read_id>/1 and /2."""
        self._check(self.lib.simmr_overlap_reset(self._h, 1 if paired else 0))

    def overlap_add(self, reads: Reads):
        """Appends the metadata of `reads` (simmr_overlap_add): start, end, contig, genome, read_id and flags; no base is read."""
        pod = reads.pod()
        self._check(self.lib.simmr_overlap_add(self._h, C.byref(pod), reads.n_reads))

    def overlap_plan(self, min_overlap: int):
        """(n_reads, n_pairs, total_bytes) of the reads added since the reset (simmr_overlap_plan)."""
        n, pairs, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.simmr_overlap_plan(self._h, int(min_overlap), C.byref(n), C.byref(pairs), C.byref(total)))
        return int(n.value), int(pairs.value), int(total.value)

    def overlap_window(self, first_place: int, max_bytes: int):
        """(n_places, n_pairs, bytes) of the longest run of places from `first_place` whose records fit `max_bytes`
        (simmr_overlap_window); SimmrError with code ERANGE if the first place alone does not fit."""
        n, pairs, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.simmr_overlap_window(self._h, int(first_place), int(max_bytes), C.byref(n), C.byref(pairs), C.byref(b)))
        return int(n.value), int(pairs.value), int(b.value)

    def overlaps(self, min_overlap: int, text: bool = True, columns: bool = False, max_bytes: Optional[int] = None):
        """The true overlaps of the reads added since overlap_reset (simmr_overlap_plan + simmr_overlap_emit): every pair of reads
        that share at least `min_overlap` reference bases, ordered by (place of the query, place of the target).  text: the PAF
        records as a CUDA uint8 tensor; columns: a dict of CUDA tensors a, b (ordinals, int32), ref_start, ref_end (int64) and
        row (int32), one entry per record.  Returns the text, the columns, or (text, columns).  With `max_bytes` the output is
        drained by windows of at most that many bytes of text (simmr_overlap_window) and concatenated."""
        torch = _torch()
        n, pairs, total = self.overlap_plan(min_overlap)
        dt = {np.uint32: torch.int32, np.uint64: torch.int64}
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device) if text else None
        cols = {name: torch.empty(max(pairs, 1), dtype=dt[t], device=self.device) for name, t in self.OVERLAP_COLUMNS} if columns else None
        place, rec, at = 0, 0, 0
        while True:
            if max_bytes is None:
                n_places, n_rec, n_bytes = n, pairs, total
            else:
                n_places, n_rec, n_bytes = self.overlap_window(place, max_bytes)
            pod = None
            if columns:
                pod = _abi.OverlapCols(*[cols[name].data_ptr() + rec * np.dtype(t).itemsize for name, t in self.OVERLAP_COLUMNS], pairs - rec)
            self._check(self.lib.simmr_overlap_emit(self._h, place, n_places, C.byref(pod) if columns else None,
                                                    C.c_void_p(out.data_ptr() + at) if text else None, total - at))
            place, rec, at = place + n_places, rec + n_rec, at + n_bytes
            if place >= n:
                break
        if columns:
            cols = {name: v[:pairs] for name, v in cols.items()}
        if text and columns:
            return out[:total], cols
        return out[:total] if text else cols

    def last_overlap_ms(self) -> float:
        return self._ms(self.lib.simmr_last_overlap_ms)

    # -- strain divergence ------------------------------------------------------------
    def strain_plan(self, genome_idx: int, identity: float, seed: int) -> int:
        """Counts the sites that `identity` and `seed` give genome slot `genome_idx` (simmr_strain_plan); returns their total."""
        total = C.c_uint64(0)
        self._check(self.lib.simmr_strain_plan(self._h, genome_idx, float(identity), C.c_uint64(seed & (2**64 - 1)), C.byref(total)))
        return int(total.value)

    def strain(self, genome_idx: int, identity: float, seed: int, sites: bool = True):
        """Diverges the staged genome in place to `identity` (0.25 .. 1) of what it was (simmr_strain_plan +
        simmr_strain_apply).  sites=True: the site list as numpy arrays {contig: uint32, pos: uint64, ref: uint8, alt: uint8}
        (ASCII), ordered by contig, then by position; sites=False: their number alone."""
        n = self.strain_plan(genome_idx, identity, seed)
        if not sites:
            self._check(self.lib.simmr_strain_apply(self._h, genome_idx, None))
            return n
        torch = _torch()
        cols = {"contig": torch.empty(max(n, 1), dtype=torch.int32, device=self.device),
                "pos": torch.empty(max(n, 1), dtype=torch.int64, device=self.device),
                "ref": torch.empty(max(n, 1), dtype=torch.uint8, device=self.device),
                "alt": torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)}
        out = _abi.StrainOut(cols["contig"].data_ptr(), cols["pos"].data_ptr(), cols["ref"].data_ptr(), cols["alt"].data_ptr(), n)
        self._check(self.lib.simmr_strain_apply(self._h, genome_idx, C.byref(out)))
        host = {k: v[:n].cpu().numpy() for k, v in cols.items()}
        return {"contig": host["contig"].view(np.uint32), "pos": host["pos"].view(np.uint64), "ref": host["ref"], "alt": host["alt"]}

    def last_strain_ms(self) -> float:
        return self._ms(self.lib.simmr_last_strain_ms)

    # -- run statistics -------------------------------------------------------------
    def stats_reset(self):
        """Zeroes the engine's run-statistics tables and their sticky error (simmr_stats_reset)."""
        self._check(self.lib.simmr_stats_reset(self._h))

    def stats_add(self, reads: Reads, n_sets: int):
        """Adds `reads` to the tables (simmr_stats_add): enqueues only.  n_sets 2: mates 1 / 2 of a paired shard; 1: long reads."""
        pod = reads.pod()
        self._check(self.lib.simmr_stats_add(self._h, C.byref(pod), reads.n_reads, int(n_sets)))

    def stats(self) -> dict:
        """The tables as numpy uint64 arrays with the names and shapes of struct simmr_run_stats (simmr_stats_read)."""
        st = _abi.RunStats()
        self._check(self.lib.simmr_stats_read(self._h, C.byref(st)))
        return {name: np.ctypeslib.as_array(getattr(st, name)).astype(np.uint64) for name, _ in _abi.RunStats._fields_}

    def last_stats_ms(self) -> float:
        return self._ms(self.lib.simmr_last_stats_ms)

    # -- coverage depth ---------------------------------------------------------------
    def depth_reset(self) -> int:
        """Zeroes the engine's difference array over every genome staged now (simmr_depth_reset); returns n_positions."""
        n, rows = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.simmr_depth_reset(self._h, C.byref(n), C.byref(rows)))
        self._depth_positions, self._depth_rows = int(n.value), int(rows.value)
        return self._depth_positions

    def depth_add(self, reads: Reads):
        """Adds the windows of `reads` (simmr_depth_add): enqueues only; reads start, end, contig and genome."""
        pod = reads.pod()
        self._check(self.lib.simmr_depth_add(self._h, C.byref(pod), reads.n_reads))

    def depth(self):
        """depth[] of the reads added since the reset as a CUDA uint32 tensor of n_positions entries (simmr_depth_emit)."""
        torch = _torch()
        n = self._depth_positions
        out = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        self._check(self.lib.simmr_depth_emit(self._h, C.c_void_p(out.data_ptr()), n))
        return out[:n].view(torch.uint32)

    def depth_contig_first(self, genome_idx: int, contig: int) -> int:
        first = C.c_uint64(0)
        self._check(self.lib.simmr_depth_contig_first(self._h, int(genome_idx), int(contig), C.byref(first)))
        return int(first.value)

    def depth_summary(self, window: int = 0, depth=None) -> dict:
        """Contig rows, depth histogram and (window > 0) the window columns of `depth` (default: self.depth()) as numpy
        arrays (simmr_depth_summarize): genome, contig, first, len, covered, depth_sum, depth_max, first_window per
        tracked contig; hist[256]; win_sum, win_covered, win_max per window."""
        torch = _torch()
        if depth is None:
            depth = self.depth()
        n_rows = self._depth_rows
        rows = (_abi.DepthContig * max(n_rows, 1))()
        hist = (C.c_uint64 * _abi.DEPTH_HIST_BINS)()
        win = _abi.DepthWindows(None, None, None, 0, 0)
        cols = None
        for _ in range(2):  # win.capacity too small: size the columns from what the call reports and call again
            rc = self.lib.simmr_depth_summarize(self._h, C.c_void_p(depth.data_ptr()), int(window), rows, len(rows), hist,
                                                C.byref(win) if window else None)
            if not (rc == _abi.ERANGE and window and win.capacity < win.n_windows):
                break
            n = int(win.n_windows)
            cols = (torch.empty(n, dtype=torch.int64, device=self.device), torch.empty(n, dtype=torch.int32, device=self.device),
                    torch.empty(n, dtype=torch.int32, device=self.device))
            win = _abi.DepthWindows(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), n, 0)
        self._check(rc)
        n = n_rows
        out = {name: np.array([getattr(rows[k], name) for k in range(n)], dtype=np.uint32 if name in ("genome", "contig", "depth_max") else np.uint64)
               for name in ("genome", "contig", "first", "len", "covered", "depth_sum", "depth_max", "first_window")}
        out["hist"] = np.array(list(hist), dtype=np.uint64)
        if window:
            m = int(win.n_windows)
            empty = m == 0 or cols is None
            out["win_sum"] = np.zeros(0, np.uint64) if empty else cols[0][:m].cpu().numpy().astype(np.uint64)
            out["win_covered"] = np.zeros(0, np.uint32) if empty else cols[1][:m].cpu().numpy().astype(np.uint32)
            out["win_max"] = np.zeros(0, np.uint32) if empty else cols[2][:m].cpu().numpy().astype(np.uint32)
        return out

    def last_depth_ms(self) -> float:
        return self._ms(self.lib.simmr_last_depth_ms)

    # -- gold-standard assembly ---------------------------------------------------------
    REGION_COLUMNS = (("genome", np.uint32), ("contig", np.uint32), ("start", np.uint64), ("len", np.uint64),
                      ("depth_sum", np.uint64), ("seq_off", np.uint64))

    def regions_plan(self, depth, min_depth: int = 1, min_len: int = 1):
        """Counts the regions of `depth` (a CUDA uint32 tensor in the layout of the last depth_reset) and their bases
        (simmr_regions_plan); returns (n_regions, n_bases)."""
        nr, nb = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.simmr_regions_plan(self._h, C.c_void_p(depth.data_ptr()), int(min_depth), int(min_len), C.byref(nr), C.byref(nb)))
        return int(nr.value), int(nb.value)

    def regions_emit(self, depth, out: "_abi.RegionsOut"):
        """Writes the columns and the base stream that `out` gives of the plan in force (simmr_regions_emit)."""
        self._check(self.lib.simmr_regions_emit(self._h, C.c_void_p(depth.data_ptr()) if depth is not None else None, C.byref(out)))

    def regions(self, min_depth: int = 1, min_len: int = 1, depth=None, seq: bool = True) -> dict:
        """The gold-standard assembly of `depth` (default: self.depth()): every run of at least `min_len` consecutive positions
        of one contig with depth >= `min_depth` (simmr_regions_plan + simmr_regions_emit).  numpy columns genome, contig
        (uint32), start, len, depth_sum (uint64) per region and seq_off (uint64, one more entry), ordered as depth[] is; "seq":
        the regions' bases as staged now, back to back, as a CUDA uint8 tensor of seq_off[-1] bytes (None with seq=False)."""
        torch = _torch()
        if depth is None:
            depth = self.depth()
        n, nb = self.regions_plan(depth, min_depth, min_len)
        dt = {np.uint32: torch.int32, np.uint64: torch.int64}
        cols = {name: torch.empty(n + 1, dtype=dt[t], device=self.device) for name, t in self.REGION_COLUMNS}
        bases = torch.empty((nb + 15) // 16 * 16 + 16, dtype=torch.uint8, device=self.device) if seq else None
        out = _abi.RegionsOut(*[cols[name].data_ptr() for name, _ in self.REGION_COLUMNS], n,
                              bases.data_ptr() if seq else None, bases.numel() if seq else 0)
        self.regions_emit(depth, out)
        res = {name: cols[name][: n + (name == "seq_off")].cpu().numpy().view(t) for name, t in self.REGION_COLUMNS}
        res["seq"] = bases[:nb] if seq else None
        return res

    def last_regions_ms(self) -> float:
        return self._ms(self.lib.simmr_last_regions_ms)

    # -- allele counts at listed sites ----------------------------------------------------
    def pileup_reset(self, genome, contig, pos) -> int:
        """Takes the site list (genome slot, contig, pos), strictly ascending in that order — torch tensors on this device or
        numpy arrays — and zeroes the engine's counts[n][2][5] (simmr_pileup_reset); returns n.  The columns are not kept."""
        torch = _torch()

        def col(a, unsigned, signed, dt):  # (torch holds the unsigned columns in the signed type of their width)
            if isinstance(a, torch.Tensor):
                return a.to(device=self.device, dtype=dt).contiguous()
            return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(unsigned)).view(signed)).to(self.device)
        g, c, p = (col(genome, np.uint32, np.int32, torch.int32), col(contig, np.uint32, np.int32, torch.int32),
                   col(pos, np.uint64, np.int64, torch.int64))
        n = int(p.numel())
        if g.numel() != n or c.numel() != n:
            raise ValueError("pileup_reset: genome, contig and pos differ in length")
        sites = _abi.PileupSites(g.data_ptr() if n else None, c.data_ptr() if n else None, p.data_ptr() if n else None, n)
        self._pileup_sites = None
        self._check(self.lib.simmr_pileup_reset(self._h, C.byref(sites)))
        self._pileup_sites = n
        return n

    def pileup_add(self, reads: Reads):
        """Adds what `reads` show at the sites (simmr_pileup_add): enqueues only; reads every column but qual and read_id."""
        pod = reads.pod()
        self._check(self.lib.simmr_pileup_add(self._h, C.byref(pod), reads.n_reads))

    def pileup(self) -> np.ndarray:
        """counts[site][strand][class] of the reads added since the reset as a numpy uint32[n, 2, 5] (simmr_pileup_read):
        strand 1 = reverse reads; classes A C G T other, observed in genome orientation."""
        torch = _torch()
        n = getattr(self, "_pileup_sites", None) or 0
        out = torch.empty(max(n, 1) * 10, dtype=torch.int32, device=self.device)
        self._check(self.lib.simmr_pileup_read(self._h, C.c_void_p(out.data_ptr()), n))
        return out[: n * 10].cpu().numpy().view(np.uint32).reshape(n, 2, 5)

    def last_pileup_ms(self) -> float:
        return self._ms(self.lib.simmr_last_pileup_ms)

    # -- fitting an error model from a run ------------------------------------------------
    def fit_reset(self, k: int = 7, max_alt_kmers: int = 20, pair_capacity: int = 1 << 20):
        """Zeroes the engine's model-fitting tables (simmr_fit_reset): k-mer size 3..10, the cut per reference k-mer, and how
        many distinct changed (reference, alternate) pairs the run may show."""
        self._check(self.lib.simmr_fit_reset(self._h, int(k), int(max_alt_kmers), int(pair_capacity)))

    def fit_add(self, reads: Reads, n_sets: int):
        """Adds `reads` to the tables (simmr_fit_add): enqueues only.  n_sets 2: a paired shard (insert sizes are taken); 1: long reads."""
        pod = reads.pod()
        self._check(self.lib.simmr_fit_add(self._h, C.byref(pod), reads.n_reads, int(n_sets)))

    def fit_add_sam(self, text, n_sets: int):
        """Adds the records of SAM `text` to the tables (simmr_fit_add_sam): whole lines, as a CUDA uint8 tensor or as bytes
        (copied up).  Enqueues only: every text is kept until a call that synchronises (fit_model, fit_sam_counts) or until
        close(), whose simmr_engine_destroy synchronises the device before anything is dropped."""
        torch = _torch()
        if isinstance(text, (bytes, bytearray, memoryview)):
            host = np.frombuffer(bytes(text), dtype=np.uint8)
            text = torch.from_numpy(host.copy()).to(self.device) if host.size else torch.empty(0, dtype=torch.uint8, device=self.device)
        if text.dtype != torch.uint8 or not text.is_cuda or not text.is_contiguous():
            raise ValueError("fit_add_sam takes bytes or a contiguous CUDA uint8 tensor")
        self._fit_sam_texts.append(text)
        n = int(text.numel())
        self._check(self.lib.simmr_fit_add_sam(self._h, C.c_void_p(text.data_ptr() if n else None), n, int(n_sets)))

    def fit_sam_counts(self) -> dict:
        """What the SAM adds since the last fit_reset took and skipped (simmr_fit_sam_counts_read), by the names of the struct."""
        c = _abi.FitSamCounts()
        self._check(self.lib.simmr_fit_sam_counts_read(self._h, C.byref(c)))
        self._fit_sam_texts = []
        return {n: int(getattr(c, n)) for n in _abi.FIT_SAM_COUNTS}

    def fit_model(self) -> dict:
        """Finishes the model from what was added (simmr_fit_plan / simmr_fit_emit): the columns of struct simmr_fit_out as
        numpy arrays, the scalars of struct simmr_fit_info, and `model_bytes`, the bincode image of the ErrorModelParams
        (model_io.serialize_model), which the custom profiles load unchanged."""
        from . import model_io
        torch = _torch()
        info = _abi.FitInfo()
        try:
            self._check(self.lib.simmr_fit_plan(self._h, C.byref(info)))
        finally:
            self._fit_sam_texts = []  # the plan has synchronised
        nr, npair, npos, nl, ni = (int(info.n_ref_kmers), int(info.n_pairs), int(info.n_positions), int(info.n_length_bins),
                                   int(info.n_insert_bins))
        shapes = {"kmer_ref": (nr, torch.int32, np.uint32), "kmer_first": (nr + 1, torch.int64, np.uint64),
                  "pair_alt": (npair, torch.int32, np.uint32), "pair_count": (npair, torch.int64, np.uint64),
                  "pair_prob": (npair, torch.float32, np.float32),
                  "qual_hist": (npos * _abi.FIT_QUALS, torch.int64, np.uint64), "qual_density": (npos * _abi.FIT_DENSITIES, torch.float64, np.float64),
                  "length_hist": (_abi.FIT_MAX_L + 1, torch.int64, np.uint64), "insert_hist": (_abi.FIT_MAX_INSERT + 1, torch.int64, np.uint64),
                  "length_density": (nl, torch.float64, np.float64), "length_lo": (nl, torch.int32, np.uint32), "length_hi": (nl, torch.int32, np.uint32),
                  "insert_density": (ni, torch.float64, np.float64), "insert_lo": (ni, torch.int32, np.uint32), "insert_hi": (ni, torch.int32, np.uint32)}
        cols = {n: torch.zeros(max(size, 1), dtype=dt, device=self.device) for n, (size, dt, _) in shapes.items()}
        out = _abi.FitOut(*[cols[n].data_ptr() for n in _abi.FIT_COLUMNS], nr, npair, npos, nl, ni)
        self._check(self.lib.simmr_fit_emit(self._h, C.byref(out)))
        m = {n: cols[n][:shapes[n][0]].cpu().numpy().view(shapes[n][2]) for n in _abi.FIT_COLUMNS}
        m["qual_hist"] = m["qual_hist"].reshape(npos, _abi.FIT_QUALS)
        m["qual_density"] = m["qual_density"].reshape(npos, _abi.FIT_DENSITIES)
        for name, _ in _abi.FitInfo._fields_:
            if name != "pad":
                m[name] = getattr(info, name)
        m["model_bytes"] = model_io.serialize_fitted(m)
        return m

    def last_fit_ms(self) -> float:
        return self._ms(self.lib.simmr_last_fit_ms)

    # -- an aligner's SAM against the true alignments ---------------------------------------
    def mapeval(self, names, min_overlap_pct: int = 10) -> "Mapeval":
        """An evaluation object (simmr_mapeval_*): `names` are the reference names of both texts, in any order.  Closed by
        its close(), or by the engine's before the engine goes."""
        m = Mapeval(self, names, min_overlap_pct)
        if not hasattr(self, "_mapevals"):
            self._mapevals = []
        self._mapevals.append(m)
        return m

    # -- an overlapper's PAF against the true overlaps --------------------------------------
    def overlap_eval(self, min_pct: int = 10) -> "OverlapEval":
        """An evaluation object (simmr_ovleval_*).  Closed by its close(), or by the engine's before the engine goes (it is kept
        in the list of the mapeval objects, which the engine closes first)."""
        m = OverlapEval(self, min_pct)
        if not hasattr(self, "_mapevals"):
            self._mapevals = []
        self._mapevals.append(m)
        return m

    # -- a variant caller's VCF against the strain's sites ----------------------------------
    def vcf_eval_open(self, names, use_filtered: bool = False) -> "VcfEval":
        """An evaluation object (simmr_vcfeval_*) over the contig names.  Closed by its close(), or by the engine's before the
        engine goes (it is kept in the list of the mapeval objects, which the engine closes first)."""
        m = VcfEval(self, names, use_filtered)
        if not hasattr(self, "_mapevals"):
            self._mapevals = []
        self._mapevals.append(m)
        return m

    def vcf_eval(self, truth, calls, names, use_filtered: bool = False, pieces=None):
        """Scores the VCF text `calls` against the truth VCF `truth` (each bytes, a CUDA uint8 tensor, or a list of those: an add
        each; with `pieces`, a bytes text goes up in that many adds cut at line ends).  Returns (counts as a dict, by_qual
        (256, 2), by_ad (33, 2), (key, alleles, ad, best, hits) of the truth entries in key order)."""
        def adds(text):
            texts = list(text) if isinstance(text, (list, tuple)) else [text]
            if pieces:
                texts = [part for t in texts for part in (cut_at_line_ends(bytes(t), int(pieces)) if isinstance(t, (bytes, bytearray, memoryview)) else [t])]
            return texts
        ev = self.vcf_eval_open(names, use_filtered)
        try:
            for t in adds(truth):
                ev.truth_add(t)
            ev.truth_plan()
            for t in adds(calls):
                ev.add(t)
            counts, by_qual, by_ad = ev.read()
            return counts, by_qual, by_ad, ev.sites()
        finally:
            ev.close()

    # -- a read classifier's calls against each read's true genome ---------------------------
    def classify_eval_open(self, taxonomy, genomes) -> "TaxEval":
        """An evaluation object (simmr_taxeval_*) over a taxonomy, a triple of arrays (taxid, parent, rank), and the genomes, a list
        of (genome_id, taxid).  Closed by its close(), or by the engine's before the engine goes (it is kept in the list of the
        mapeval objects, which the engine closes first)."""
        m = TaxEval(self, taxonomy, genomes)
        if not hasattr(self, "_mapevals"):
            self._mapevals = []
        self._mapevals.append(m)
        return m

    def classify_eval(self, truth, calls, taxonomy, genomes, pieces=1):
        """Scores the classifier's per-read text `calls` against the truth TSV `truth` (each bytes, a CUDA uint8 tensor, or a list
        of those: an add each; a bytes text goes up in `pieces` adds cut at line ends).  Returns (counts as a dict, by_rank (8, 5),
        reads_by_rank (8, 5), (id, genome_row, mates, seen, hits) of the truth entries in id order, (taxid, true, called, both)
        of the nodes in taxid order)."""
        def adds(text):
            texts = list(text) if isinstance(text, (list, tuple)) else [text]
            return [part for t in texts for part in (cut_at_line_ends(bytes(t), max(int(pieces), 1)) if isinstance(t, (bytes, bytearray, memoryview)) else [t])]
        ev = self.classify_eval_open(taxonomy, genomes)
        try:
            for t in adds(truth):
                ev.truth_add(t)
            ev.truth_plan()
            for t in adds(calls):
                ev.add(t)
            counts, by_rank, reads_by_rank = ev.read()
            return counts, by_rank, reads_by_rank, ev.reads(), ev.taxa()
        finally:
            ev.close()

    # -- an assembler's contigs against the gold-standard assembly ---------------------------
    def assembly_eval_open(self, genomes, k: int = 31, plain_search: bool = False) -> "AsmEval":
        """An evaluation object (simmr_asmeval_*) over the genome names.  Closed by its close(), or by the engine's before the
        engine goes (it is kept in the list of the mapeval objects, which the engine closes first)."""
        m = AsmEval(self, genomes, k, plain_search)
        if not hasattr(self, "_mapevals"):
            self._mapevals = []
        self._mapevals.append(m)
        return m

    def assembly_eval(self, truth_bytes, contigs_bytes, genomes, k: int = 31):
        """Scores the FASTA `contigs_bytes` against the gold-standard FASTA `truth_bytes` (each bytes, a CUDA uint8 tensor, or a
        list of those: an add each, of whole records).  Returns (counts as a dict, by_genome (n_genomes + 1, 5), (key, genome,
        mult, hits) of the entries in key order, (length, kmers, found, shared, top_genome, top_kmers) of the contigs)."""
        def adds(text):
            return list(text) if isinstance(text, (list, tuple)) else [text]
        ev = self.assembly_eval_open(genomes, k)
        try:
            for t in adds(truth_bytes):
                ev.truth_add(t)
            ev.truth_plan()
            for t in adds(contigs_bytes):
                ev.add(t)
            counts, by_genome = ev.read()
            return counts, by_genome, ev.entries(), ev.contigs()
        finally:
            ev.close()

    # -- an assembler's contigs placed on the gold-standard assembly -------------------------
    def assembly_map_open(self, genomes, k: int = 31, band: int = 64, relocation: int = 1000, min_anchors: int = 16) -> "AsmMap":
        """A placement object (simmr_asmmap_*) over the genome names.  Closed by its close(), or by the engine's before the
        engine goes (it is kept in the list of the mapeval objects, which the engine closes first)."""
        m = AsmMap(self, genomes, k, band, relocation, min_anchors)
        if not hasattr(self, "_mapevals"):
            self._mapevals = []
        self._mapevals.append(m)
        return m

    def assembly_map(self, truth_bytes, contigs_bytes, genomes, k: int = 31, band: int = 64, relocation: int = 1000, min_anchors: int = 16):
        """Places the FASTA `contigs_bytes` on the gold-standard FASTA `truth_bytes` (each bytes, a CUDA uint8 tensor, or a list
        of those: an add each, of whole records).  Returns (counts as a dict, by_genome (n_genomes, 5), (length, hits, blocks,
        first_block, block_bases, worst_join) of the contigs, the nine block columns)."""
        def adds(text):
            return list(text) if isinstance(text, (list, tuple)) else [text]
        ev = self.assembly_map_open(genomes, k, band, relocation, min_anchors)
        try:
            for t in adds(truth_bytes):
                ev.truth_add(t)
            ev.truth_plan()
            for t in adds(contigs_bytes):
                ev.add(t)
            counts, by_genome = ev.read()
            return counts, by_genome, ev.contigs(), ev.blocks()
        finally:
            ev.close()

    # -- a binner's bins against each contig's true genome ------------------------------------
    def binning_eval_open(self, genomes, hash_bits: int = 64) -> "BinEval":
        """An evaluation object (simmr_bineval_*) over the genome names.  Closed by its close(), or by the engine's before the
        engine goes (it is kept in the list of the mapeval objects, which the engine closes first)."""
        m = BinEval(self, genomes, hash_bits)
        if not hasattr(self, "_mapevals"):
            self._mapevals = []
        self._mapevals.append(m)
        return m

    def binning_eval(self, truth_bytes, bins_bytes, genomes, hash_bits: int = 64):
        """Scores the binner's assignment `bins_bytes` against the contig truth `truth_bytes` (each bytes, a CUDA uint8 tensor, or a
        list of those: an add each, cut behind a line end).  Returns (counts as a dict, by_genome (n_genomes + 1, 7), the six bin
        columns, the four cell columns, the four contig columns)."""
        def adds(text):
            return list(text) if isinstance(text, (list, tuple)) else [text]
        ev = self.binning_eval_open(genomes, hash_bits)
        try:
            for t in adds(truth_bytes):
                ev.truth_add(t)
            ev.truth_plan()
            for t in adds(bins_bytes):
                ev.add(t)
            counts, by_genome = ev.read()
            return counts, by_genome, ev.bins(), ev.cells(), ev.contigs()
        finally:
            ev.close()

    # -- a read error corrector's output against the true reads -------------------------------
    def correction_eval_open(self, lines_per_record: int = 4) -> "CorrEval":
        """An evaluation object (simmr_correval_*).  Closed by its close(), or by the engine's before the engine goes (it is kept in
        the list of the mapeval objects, which the engine closes first)."""
        m = CorrEval(self, lines_per_record)
        if not hasattr(self, "_mapevals"):
            self._mapevals = []
        self._mapevals.append(m)
        return m

    def correction_eval(self, truth_sam_bytes, corrected_bytes, lines_per_record: int = 4):
        """Scores the corrected reads `corrected_bytes` (FASTQ, or two-line FASTA with lines_per_record=2) against the truth SAM
        `truth_sam_bytes` (each bytes, a CUDA uint8 tensor, or a list of those: an add each, cut at a line's end for the truth and at
        a record's end for the reads).  Returns (counts as a dict, cube (5, 5, 5), by_qual (95, 5), by_pos (512, 5), (key, length,
        before, residual, hits) of the truth entries in key order)."""
        def adds(text):
            return list(text) if isinstance(text, (list, tuple)) else [text]
        ev = self.correction_eval_open(lines_per_record)
        try:
            for t in adds(truth_sam_bytes):
                ev.truth_add(t)
            ev.truth_plan()
            for t in adds(corrected_bytes):
                ev.add(t)
            counts, cube, by_qual, by_pos = ev.read()
            return counts, cube, by_qual, by_pos, ev.entries()
        finally:
            ev.close()

    # -- counters / timing --------------------------------------------------------
    def counters(self) -> np.ndarray:
        host = (C.c_uint64 * _abi.N_COUNTERS)()
        self._check(self.lib.simmr_counters(self._h, None, host))
        return np.array(list(host), dtype=np.uint64)

    def counters_to(self, tensor):
        """Copy the counters into a CUDA int64 tensor (for one all-reduce)."""
        self._check(self.lib.simmr_counters(self._h, C.c_void_p(tensor.data_ptr()), None))

    def counters_reset(self):
        self._check(self.lib.simmr_counters_reset(self._h))

    # -- the counters across GPUs without torch.distributed: RCCL through the C ABI ------
    def comm_unique_id(self) -> bytes:
        """rank 0: an id to hand to the other ranks (ncclGetUniqueId)"""
        buf = C.create_string_buffer(_abi.COMM_ID_BYTES)
        rc = self.lib.simmr_comm_unique_id(buf)
        if rc != 0:
            raise SimmrError(rc, "simmr_comm_unique_id failed (is librccl loadable?)")
        return buf.raw

    def comm_init(self, comm_id: bytes, rank: int, world: int):
        buf = C.create_string_buffer(bytes(comm_id), _abi.COMM_ID_BYTES)
        self._check(self.lib.simmr_comm_init(self._h, buf, int(rank), int(world)))

    def allreduce_counts(self, tensor):
        """in-place sum over the ranks of a CUDA int64 tensor (a no-op without a communicator)"""
        self._check(self.lib.simmr_allreduce_counts(self._h, C.c_void_p(tensor.data_ptr()), int(tensor.numel())))

    def last_emit_kernel_ms(self) -> float:
        return self._ms(self.lib.simmr_last_emit_kernel_ms)

    def emit_kernel_ms_mean(self, last_n: int) -> float:
        """Mean HIP-event time of the last `last_n` emits (one synchronisation; simmr_emit_kernel_ms_mean)."""
        ms = C.c_float()
        self._check(self.lib.simmr_emit_kernel_ms_mean(self._h, int(last_n), C.byref(ms)))
        return ms.value

    def last_plan_ms(self) -> float:
        return self._ms(self.lib.simmr_last_plan_ms)
