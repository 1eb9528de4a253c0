// record_stream.hpp — the bodies the four record writers share on the device: the SAM text and the BAM records, in read order
// (sam_kernels.hip, bam_kernels.hip) and in coordinate order (sam_sort_kernels.hip, bam_index_kernels.hip).  Routines only, no
// kernel: included by sam_kernels.hip behind its record routine, so every unit that includes that file gets its own copy, as
// with sam_scan_chunks.  The sixteen kernels k_{sam,bam,samsort,bamsort}_* are wrappers over these bodies and the two scans'
// bodies of sam_kernels.hip; each declares its own LDS and hands it in.
//
// A record policy `Rec` says what a record is: SamRec (sam_kernels.hip, over sam_record<>) or BamRec (bam_kernels.hip, over
// bam_record<>).  It gives
//   Rec::SLOT_BYTES                 LDS bytes the writer needs per row of 16 lanes (SAM: the head and tail slots; BAM: 0);
//   Rec::size(rd, ed, nm, r, ...)   the bytes of read r's record (0 for a refused read), in every lane of the row;
//   Rec::write(rd, ed, nm, r, at, ..., slot, off, dst, err)   the record of read r into bytes off[at] .. off[at + 1] of dst.
// Both are one routine underneath, so a record's length and its bytes cannot disagree.
// Not self-standing: it is written in the terms sam_kernels.hip has defined above its include (SIMMR_DEV, SamReads / SamEdits /
// SamNames, the SAM_* constants, sam_wg_scan) and is meant to be included from there alone.
#pragma once
#if !defined(SAM_LANES) || !defined(SAM_CHUNK) || !defined(SIMMR_DEV)
#error "record_stream.hpp is included by sam_kernels.hip, behind its record routine"
#endif

namespace simmr {

#define REC_KEY_POS_BITS 40u /* the canonical key of a place: row << 40 | lo */

// ---- sizes in read order: the body of k_sam_size / k_bam_size -----------------------------------------------------------
// A workgroup takes chunks of SAM_CHUNK consecutive reads, 16 at a time, and leaves every chunk's sum: the scan's first level.
// part: SAM_WG_READS words of LDS.
template <class Rec>
SIMMR_DEV void rec_size_chunks(const SamReads& rd, const SamEdits& ed, const SamNames& nm, uint64_t n_reads, uint32_t paired,
                               uint32_t* __restrict__ len, uint64_t* __restrict__ chunk_sum, uint32_t* __restrict__ err, uint32_t* part) {
  const uint32_t sub = threadIdx.x & (SAM_LANES - 1u), row = threadIdx.x / SAM_LANES;
  const uint64_t n_chunks = (n_reads + SAM_CHUNK - 1u) / SAM_CHUNK;
  for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    uint32_t acc = 0;  // (a record is below 2^20 bytes: 64 of them fit)
    for (uint32_t it = 0; it < SAM_CHUNK / SAM_WG_READS; it++) {
      const uint64_t r = chunk * SAM_CHUNK + it * SAM_WG_READS + row;
      const uint32_t bytes = Rec::size(rd, ed, nm, r, n_reads, paired, sub, err);
      if (sub == 0u && r < n_reads) len[r] = bytes;
      acc += bytes;
    }
    if (sub == 0u) part[row] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t s = 0;
      for (uint32_t i = 0; i < SAM_WG_READS; i++) s += part[i];
      chunk_sum[chunk] = s;
    }
    __syncthreads();
  }
}

// ---- sizes and keys: the body of k_samsort_size / k_bamsort_size --------------------------------------------------------
// A row of 16 lanes per read.  The bound check that gives the key its width: max(start, end) <= the staged length of the
// read's contig.  A read outside its contig (or without a named contig) sets bit 2 of the error word and has nothing else
// loaded or stored for it but zeros.  WITH_END: end[r] is the exclusive end of the interval the BAM record gives its bin
// (lo + L, or lo + 1 for a read without bases).
template <class Rec, bool WITH_END>
SIMMR_DEV void rec_size_keyed(const SamReads& rd, const SamEdits& ed, const SamNames& nm, const uint64_t* __restrict__ c_bases, uint64_t n_reads,
                              uint32_t paired, uint32_t pos_bits, uint32_t* __restrict__ len, uint64_t* __restrict__ key, uint32_t* __restrict__ end,
                              uint32_t* __restrict__ err) {
  const uint32_t sub = threadIdx.x & (SAM_LANES - 1u), row = threadIdx.x / SAM_LANES;
  const uint64_t n_chunks = (n_reads + SAM_CHUNK - 1u) / SAM_CHUNK;
  for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    for (uint32_t it = 0; it < SAM_CHUNK / SAM_WG_READS; it++) {
      const uint64_t r = chunk * SAM_CHUNK + it * SAM_WG_READS + row;
      if (r >= n_reads) continue;  // (uniform over the row)
      const uint64_t a = rd.start[r], b = rd.end[r];
      const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
      const uint32_t g = rd.genome[r], c = rd.contig[r];
      bool ok = g < nm.n_slots;
      if (ok) ok = c < nm.g_ncontig[g];
      uint64_t crow = 0;
      if (ok) {
        crow = (uint64_t)nm.g_cbase[g] + c;
        ok = hi <= c_bases[crow];
      }
      uint32_t bytes = 0, e = 0;
      uint64_t k = 0;
      if (ok) {
        bytes = Rec::size(rd, ed, nm, r, n_reads, paired, sub, err);
        k = (crow << pos_bits) | lo;  // (lo <= hi <= the contig's length < 2^pos_bits)
        if (WITH_END) e = bytes ? (uint32_t)(hi > lo ? hi : lo + 1u) : 0u;  // (a record was sized: hi < 2^31)
      } else if (sub == 0u) {
        atomicOr(err, 2u);
      }
      if (sub == 0u) {
        len[r] = bytes;
        key[r] = k;
        if (WITH_END) end[r] = e;
      }
    }
  }
}

// ---- the sorted lengths: the body of k_samsort_gather / k_bamsort_gather ------------------------------------------------
// A workgroup per chunk, four consecutive places per thread; perm == nullptr: place i holds read i (a key without bits).
// Leaves the lengths (and with WITH_END the ends) in sorted order, the sum of every chunk of SAM_CHUNK lengths, and the
// canonical key of every place.  lds: 256 words.
template <bool WITH_END>
SIMMR_DEV void rec_gather(const uint32_t* __restrict__ len, const uint32_t* __restrict__ end, const uint64_t* __restrict__ key,
                          const uint32_t* __restrict__ perm, uint64_t n, uint32_t pos_bits, uint32_t* __restrict__ slen, uint32_t* __restrict__ send,
                          uint64_t* __restrict__ ckey, uint64_t* __restrict__ chunk_sum, uint32_t* lds) {
  const uint64_t n_chunks = (n + SAM_CHUNK - 1u) / SAM_CHUNK;
  const uint64_t lo_mask = (1ull << pos_bits) - 1ull;  // (pos_bits <= 40)
  for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // (uniform over the workgroup)
    const uint64_t i0 = chunk * SAM_CHUNK + 4u * threadIdx.x;
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
      const uint64_t i = i0 + q;
      if (i >= n) continue;
      const uint64_t r = perm ? perm[i] : i;
      const uint32_t v = r < n ? len[r] : 0u;
      const uint64_t k = key[i];
      slen[i] = v;
      if (WITH_END) send[i] = r < n ? end[r] : 0u;
      ckey[i] = ((k >> pos_bits) << REC_KEY_POS_BITS) | (k & lo_mask);
      sum += v;
    }
    uint32_t total;  // (a chunk is below 2^30 bytes)
    (void)sam_wg_scan<uint32_t>(sum, lds, &total);
    if (threadIdx.x == 0) chunk_sum[chunk] = total;
  }
}

// ---- the records: the body of the four write kernels ------------------------------------------------------------------------
// One row of 16 lanes writes the record of place i at entry i of off[].  SORTED == false: place i holds read i and perm is
// not looked at (the kernels in read order pay neither a load nor a branch for it).  SORTED: the read is perm[i], or i when
// perm == nullptr; a place past the end, like a read past it, has no record.  slots: SAM_WG_READS x Rec::SLOT_BYTES of LDS.
template <class Rec, bool SORTED>
SIMMR_DEV void rec_write_places(const SamReads& rd, const SamEdits& ed, const SamNames& nm, uint64_t n_reads, uint32_t paired,
                                const uint32_t* __restrict__ perm, const uint64_t* __restrict__ off, uint8_t* __restrict__ dst,
                                uint32_t* __restrict__ err, uint8_t* slots) {
  const uint32_t sub = threadIdx.x & (SAM_LANES - 1u), row = threadIdx.x / SAM_LANES;
  const uint64_t n_batches = (n_reads + SAM_WG_READS - 1u) / SAM_WG_READS;
  uint8_t* slot = Rec::SLOT_BYTES ? slots + row * Rec::SLOT_BYTES : nullptr;
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t i = batch * SAM_WG_READS + row;
    uint64_t r = i;
    if (SORTED) r = i < n_reads ? (perm ? (uint64_t)perm[i] : i) : n_reads;
    Rec::write(rd, ed, nm, r, i, n_reads, paired, sub, slot, off, dst, err);
  }
}

}  // namespace simmr
