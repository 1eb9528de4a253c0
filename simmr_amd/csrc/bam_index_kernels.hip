// bam_index_kernels.hip — the BAM records in coordinate order and the BAI index of a coordinate-sorted record stream
// (include/simmr_hip.h: simmr_bam_sort_*, simmr_bai_*) on gfx950.  Included by bam_index.hip alone, a translation unit of
// libsimmr_hip.so of its own.  The record policy (BamRec) is bam_kernels.hip's (included without its kernels), the scans' bodies are
// sam_kernels.hip's, the sort is sam_sort.hip's (samsort_sort_pairs, engine_internal.hpp): a record's bytes cannot differ from
// simmr_bam_emit's, only its place does.
//
// No place comes from the order in which atomics land.  The atomics are the error word, the largest end of a reference
// (atomicMax) and the smallest virtual offset of a window (atomicMin): values, which do not depend on the order.
//
// The sorted records, five kernels:
//   k_bamsort_size     every record's length (BamRec::size), its sort key row << P | lo after the bound check of the
//                      sorted SAM (max(start, end) <= the staged length of the read's contig), and end[r]: the exclusive end
//                      of the interval the record gives bam_reg2bin (lo + L, or lo + 1 for a read without bases);
//   k_bamsort_gather   lengths and ends in sorted order, the sum of every chunk of SAM_CHUNK lengths, the canonical keys;
//   k_bamsort_scan, k_bamsort_offsets   the chunked scan of sam_kernels.hip: rec_off[0 .. n];
//   k_bamsort_write    BamRec::write for place i with r = perm[i]: every store bounded by rec_off[i + 1] - rec_off[i].
// The bodies of the size, gather and write kernels are rec_size_keyed, rec_gather and rec_write_places of record_stream.hpp,
// shared with the sorted SAM; the record policy is bam_kernels.hip's BamRec, so this file holds no record routine.
//
// The index, nine kernels.  Input: key[i] = row << 40 | lo, end[i], rec_off[0 .. n] of n records in file order, and `base`,
// the uncompressed bytes in front of record 0.  The virtual offset of uncompressed position p is
// ((p / 65280) * 65311) << 16 | (p % 65280): every block but the last holds BGZF_BLOCK source bytes.
//   k_bai_check        per record: the key ascends, rec_off does not decrease, row < n_ref, lo < end <= 2^29 (else the error
//                      word); rb[i] = row << 16 | reg2bin(lo, end); the largest end of every reference;
//   k_bai_count        per chunk of SAM_CHUNK entries of a[]: how many differ from the entry before (entry 0 does);
//   k_bai_scan         ONE workgroup: the exclusive scan of those counts;
//   k_bai_compact      the entries that differ, compacted: their value and their index (and n behind the last).
//                      Run over rb[] these are the RUNS: maximal stretches of consecutive records of one bin — the chunks.
//                      The runs are then sorted by (row, bin) (stable: file order survives inside a bin) and the same three
//                      kernels run over the sorted run keys give the BINS: their value and their first sorted run;
//   k_bai_refs         per reference: its first bin and its first record (binary searches);
//   k_bai_layout       ONE workgroup: per reference n_intv = 1 + ((largest end - 1) >> 14) and the bytes of its part of the
//                      file, both scanned: where every reference's part and its windows begin;
//   k_bai_windows      per record: atomicMin of its start's virtual offset into every 16 Kbase window it overlaps;
//   k_bai_write_chunks per sorted run: its chunk (virtual offsets of its first record's start and its last record's end) at
//                      its computed place; the first run of a bin also writes the bin's number and n_chunk;
//   k_bai_write_refs   a workgroup per reference: n_bin, the metadata bin 37450, n_intv, and the linear index — an empty
//                      window takes the value of the window before it (0 at the front), by a scan of "last window that has
//                      a record"; workgroup 0 also writes the magic, n_ref and the trailing n_no_coor.
// LDS per workgroup: k_bamsort_size none, gather 1 KiB, scan 2 KiB, offsets 1 KiB, write none; k_bai_check 1 KiB (the
// workgroup's largest end), count 1 KiB, scan 2 KiB, compact 1 KiB, refs none, layout 2 KiB, windows none, write_chunks none,
// write_refs 1 KiB.
#pragma once
#define BAM_ROUTINES_ONLY
#include "bam_kernels.hip"

namespace simmr {

#define BAI_KEY_POS_BITS 40u      /* the canonical key: row << 40 | lo (REC_KEY_POS_BITS, record_stream.hpp) */
#define BAI_BIN_BITS 16u          /* a run's key: row << 16 | bin */
#define BAI_MAX_END 0x20000000u   /* 2^29: what the six bin levels cover */
#define BAI_WINDOW_BITS 14u       /* the linear index: windows of 16384 bases */
#define BAI_META_BIN 37450u
#define BAI_BLOCK_FRAMED (BGZF_BLOCK + BGZF_OVERHEAD)
#define BAI_ERR_ORDER 1u          /* keys descend, rec_off decreases, a row outside n_ref, an empty interval */
#define BAI_ERR_RANGE 2u          /* a record ends beyond 2^29 */

static_assert(BAI_KEY_POS_BITS == REC_KEY_POS_BITS, "one canonical key for the sorted SAM, the sorted BAM and the index");

// ---- the sorted records -------------------------------------------------------------------------------------------------
// A workgroup takes chunks of SAM_CHUNK consecutive reads, 16 at a time, a row of 16 lanes per read.  A read outside its
// contig (or without a named contig) sets the error word and has nothing else loaded or stored for it but zeros.
extern "C" __global__ void __launch_bounds__(256)
k_bamsort_size(const SamReads rd, const SamEdits ed, const SamNames nm, const uint64_t* __restrict__ c_bases, uint64_t n_reads, uint32_t paired,
               uint32_t pos_bits, uint32_t* __restrict__ len, uint64_t* __restrict__ key, uint32_t* __restrict__ end, uint32_t* __restrict__ err) {
  rec_size_keyed<BamRec, true>(rd, ed, nm, c_bases, n_reads, paired, pos_bits, len, key, end, err);
}

// a workgroup per chunk, four consecutive places per thread; perm == nullptr: place i holds read i (a key without bits)
extern "C" __global__ void __launch_bounds__(256)
k_bamsort_gather(const uint32_t* __restrict__ len, const uint32_t* __restrict__ end, const uint64_t* __restrict__ key,
                 const uint32_t* __restrict__ perm, uint64_t n, uint32_t pos_bits, uint32_t* __restrict__ slen, uint32_t* __restrict__ send,
                 uint64_t* __restrict__ ckey, uint64_t* __restrict__ chunk_sum) {
  __shared__ uint32_t lds[256];
  rec_gather<true>(len, end, key, perm, n, pos_bits, slen, send, ckey, chunk_sum, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_bamsort_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_bamsort_offsets(const uint32_t* __restrict__ slen, const uint64_t* __restrict__ prefix, uint64_t n, uint64_t* __restrict__ rec_off) {
  __shared__ uint32_t lds[256];
  sam_chunk_offsets(slen, prefix, n, rec_off, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_bamsort_write(const SamReads rd, const SamEdits ed, const SamNames nm, uint64_t n_reads, uint32_t paired, const uint32_t* __restrict__ perm,
                const uint64_t* __restrict__ rec_off, uint8_t* __restrict__ dst, uint32_t* __restrict__ err) {
  rec_write_places<BamRec, true>(rd, ed, nm, n_reads, paired, perm, rec_off, dst, err, nullptr);
}

// ---- the index ------------------------------------------------------------------------------------------------------------
// SAM spec 4.1.1 under the caller's contract: every block in front of position p is full
SIMMR_DEV uint64_t bai_voff(uint64_t p) {
  const uint64_t blk = p / BGZF_BLOCK;
  return ((blk * BAI_BLOCK_FRAMED) << 16) | (p - blk * BGZF_BLOCK);
}
SIMMR_DEV void bai_store32(uint8_t* dst, uint64_t at, uint64_t cap, uint32_t v) {
  if (at <= cap && cap - at >= 4u) *reinterpret_cast<u32_unaligned*>(dst + at) = v;
}
SIMMR_DEV void bai_store64(uint8_t* dst, uint64_t at, uint64_t cap, uint64_t v) {
  bai_store32(dst, at, cap, (uint32_t)v);
  bai_store32(dst, at + 4u, cap, (uint32_t)(v >> 32));
}
// the first index in [0, n) whose entry is >= v (n: none)
SIMMR_DEV uint64_t bai_lower_bound(const uint64_t* __restrict__ a, uint64_t n, uint64_t v) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// a workgroup per chunk of SAM_CHUNK records, four consecutive records per thread.  A refused record gets the run key of the
// record before it in the thread (or ~0): nothing downstream indexes with it, and the plan ends with the error.
extern "C" __global__ void __launch_bounds__(256)
k_bai_check(const uint64_t* __restrict__ key, const uint32_t* __restrict__ end, const uint64_t* __restrict__ rec_off, uint64_t n, uint64_t n_ref,
            uint64_t* __restrict__ rb, uint32_t* __restrict__ ref_max_end, uint32_t* __restrict__ err) {
  __shared__ uint32_t lds[256];
  const uint64_t n_chunks = (n + SAM_CHUNK - 1u) / SAM_CHUNK;
  const uint64_t lo_mask = (1ull << BAI_KEY_POS_BITS) - 1ull;
  for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // (uniform over the workgroup)
    const uint64_t c0 = chunk * SAM_CHUNK, c1 = c0 + SAM_CHUNK < n ? c0 + SAM_CHUNK : n;
    const bool one_row = (key[c0] >> BAI_KEY_POS_BITS) == (key[c1 - 1u] >> BAI_KEY_POS_BITS);  // (sorted: every record between them too)
    uint32_t wg_max = 0, bad = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
      const uint64_t i = c0 + 4u * threadIdx.x + q;
      if (i >= n) continue;
      const uint64_t k = key[i], row = k >> BAI_KEY_POS_BITS, lo = k & lo_mask;
      const uint32_t e = end[i];
      uint32_t mine = 0;
      if (i > 0u && key[i - 1u] > k) mine |= BAI_ERR_ORDER;
      if (rec_off[i + 1u] < rec_off[i]) mine |= BAI_ERR_ORDER;
      if (row >= n_ref || lo >= (uint64_t)e) mine |= BAI_ERR_ORDER;
      if (e > BAI_MAX_END) mine |= BAI_ERR_RANGE;
      bad |= mine;
      if (mine) { rb[i] = ~0ull; continue; }
      rb[i] = (row << BAI_BIN_BITS) | bam_reg2bin((uint32_t)lo, e);
      if (one_row) wg_max = e > wg_max ? e : wg_max;
      else atomicMax(&ref_max_end[row], e);
    }
    if (bad) atomicOr(err, bad);
    // one atomic for a chunk of one reference (nearly every chunk): the largest end over the workgroup
    lds[threadIdx.x] = wg_max;
    __syncthreads();
    for (uint32_t d = 128u; d > 0u; d >>= 1) {
      if (threadIdx.x < d) lds[threadIdx.x] = lds[threadIdx.x] > lds[threadIdx.x + d] ? lds[threadIdx.x] : lds[threadIdx.x + d];
      __syncthreads();
    }
    if (threadIdx.x == 0 && one_row && lds[0] > 0u) {
      const uint64_t row = key[c0] >> BAI_KEY_POS_BITS;
      if (row < n_ref) atomicMax(&ref_max_end[row], lds[0]);
    }
    __syncthreads();  // lds[] is the next chunk's
  }
}

SIMMR_DEV bool bai_differs(const uint64_t* __restrict__ a, uint64_t i) { return i == 0u || a[i] != a[i - 1u]; }

extern "C" __global__ void __launch_bounds__(256)
k_bai_count(const uint64_t* __restrict__ a, uint64_t n, uint64_t* __restrict__ chunk_sum) {
  __shared__ uint32_t lds[256];
  const uint64_t n_chunks = (n + SAM_CHUNK - 1u) / SAM_CHUNK;
  for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // (uniform over the workgroup)
    const uint64_t i0 = chunk * SAM_CHUNK + 4u * threadIdx.x;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++)
      if (i0 + q < n && bai_differs(a, i0 + q)) c++;
    uint32_t total;
    (void)sam_wg_scan<uint32_t>(c, lds, &total);
    if (threadIdx.x == 0) chunk_sum[chunk] = total;
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_bai_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

// out_val[j] / out_first[j]: the j-th entry of a[] that differs from the one before, and its index; out_first[n_out] = n
extern "C" __global__ void __launch_bounds__(256)
k_bai_compact(const uint64_t* __restrict__ a, uint64_t n, const uint64_t* __restrict__ prefix, uint64_t n_out, uint64_t* __restrict__ out_val,
              uint32_t* __restrict__ out_first) {
  __shared__ uint32_t lds[256];
  const uint64_t n_chunks = (n + SAM_CHUNK - 1u) / SAM_CHUNK;
  if (blockIdx.x == 0 && threadIdx.x == 0) out_first[n_out] = (uint32_t)n;  // (fewer than 2^31 entries)
  for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // (uniform over the workgroup)
    const uint64_t i0 = chunk * SAM_CHUNK + 4u * threadIdx.x;
    bool f[4];
    uint32_t c = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
      f[q] = i0 + q < n && bai_differs(a, i0 + q);
      c += f[q] ? 1u : 0u;
    }
    uint32_t total;
    uint64_t j = prefix[chunk] + sam_wg_scan<uint32_t>(c, lds, &total);
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
      if (!f[q]) continue;
      if (j < n_out) {  // (it is: the counts are those of these entries)
        out_val[j] = a[i0 + q];
        out_first[j] = (uint32_t)(i0 + q);
      }
      j++;
    }
  }
}

// reference r of 0 .. n_ref (one past the last, for the differences): its first bin and its first record
extern "C" __global__ void __launch_bounds__(256)
k_bai_refs(const uint64_t* __restrict__ bin_key, uint64_t n_bins, const uint64_t* __restrict__ key, uint64_t n, uint64_t n_ref,
           uint32_t* __restrict__ ref_bin0, uint32_t* __restrict__ ref_rec0) {
  for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r <= n_ref; r += (uint64_t)gridDim.x * 256u) {
    // (entry n_ref is the end outright: with 2^24 references its key would be 2^64)
    ref_bin0[r] = r == n_ref ? (uint32_t)n_bins : (uint32_t)bai_lower_bound(bin_key, n_bins, r << BAI_BIN_BITS);
    ref_rec0[r] = r == n_ref ? (uint32_t)n : (uint32_t)bai_lower_bound(key, n, r << BAI_KEY_POS_BITS);
  }
}

// ONE workgroup.  A reference with records: n_bin, its bins (8 bytes and 16 per chunk), the metadata bin (40), n_intv and the
// windows; one without: n_bin = 0 and n_intv = 0.  ref_off[r]: where its part begins in the file (the magic and n_ref in
// front); win_off[r]: where its windows begin among all windows.  Entry n_ref of both: the totals (the file's without n_no_coor).
extern "C" __global__ void __launch_bounds__(256)
k_bai_layout(const uint32_t* __restrict__ ref_bin0, const uint32_t* __restrict__ bin_first, const uint32_t* __restrict__ ref_max_end, uint64_t n_ref,
             uint32_t* __restrict__ ref_intv, uint64_t* __restrict__ ref_off, uint64_t* __restrict__ win_off) {
  __shared__ uint64_t lds[256];
  uint64_t carry_b = 8u, carry_w = 0u;
  for (uint64_t base = 0; base < n_ref; base += 256u) {  // (uniform over the workgroup)
    const uint64_t r = base + threadIdx.x;
    uint64_t bytes = 0;
    uint32_t n_intv = 0;
    if (r < n_ref) {
      const uint32_t b0 = ref_bin0[r], b1 = ref_bin0[r + 1u];
      bytes = 8u;
      if (b1 > b0) {
        const uint32_t me = ref_max_end[r];
        n_intv = 1u + ((me ? me - 1u : 0u) >> BAI_WINDOW_BITS);
        bytes = 4u + 8ull * (b1 - b0) + 16ull * (bin_first[b1] - bin_first[b0]) + 40u + 4u + 8ull * n_intv;
      }
      ref_intv[r] = n_intv;
    }
    uint64_t total_b, total_w;
    const uint64_t ex_b = sam_wg_scan<uint64_t>(bytes, lds, &total_b);
    const uint64_t ex_w = sam_wg_scan<uint64_t>((uint64_t)n_intv, lds, &total_w);
    if (r < n_ref) { ref_off[r] = carry_b + ex_b; win_off[r] = carry_w + ex_w; }
    carry_b += total_b;
    carry_w += total_w;
  }
  if (threadIdx.x == 0) { ref_off[n_ref] = carry_b; win_off[n_ref] = carry_w; }
}

// win[] starts as all ones.  A record from simmr_bam_sort_emit spans at most five windows (a read has at most 65 535 bases); a
// caller's own columns may hold a record over up to 32 768 of them, which one thread then walks alone: right, and slow.  Every
// index is checked against the plan's layout, so columns changed since the plan cannot carry a store out of win[].
extern "C" __global__ void __launch_bounds__(256)
k_bai_windows(const uint64_t* __restrict__ key, const uint32_t* __restrict__ end, const uint64_t* __restrict__ rec_off, uint64_t n, uint64_t n_ref,
              uint64_t base, const uint32_t* __restrict__ ref_intv, const uint64_t* __restrict__ win_off, unsigned long long* __restrict__ win) {
  const uint64_t lo_mask = (1ull << BAI_KEY_POS_BITS) - 1ull;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t k = key[i], row = k >> BAI_KEY_POS_BITS, lo = k & lo_mask;
    const uint32_t e = end[i];
    if (row >= n_ref || lo >= (uint64_t)e) continue;
    const uint32_t n_intv = ref_intv[row];
    const uint64_t w0 = lo >> BAI_WINDOW_BITS, w1 = (uint64_t)(e - 1u) >> BAI_WINDOW_BITS;
    const unsigned long long v = bai_voff(base + rec_off[i]);
    for (uint64_t w = w0; w <= w1 && w < n_intv; w++) atomicMin(&win[win_off[row] + w], v);
  }
}

// sorted run j: chunk (j - the first sorted run of its bin) of bin b = the bin of j
extern "C" __global__ void __launch_bounds__(256)
k_bai_write_chunks(const uint64_t* __restrict__ bin_key, const uint32_t* __restrict__ bin_first, uint64_t n_bins, const uint32_t* __restrict__ run_perm,
                   const uint32_t* __restrict__ run_first, uint64_t n_runs, const uint64_t* __restrict__ rec_off, uint64_t n, uint64_t n_ref,
                   uint64_t base, const uint32_t* __restrict__ ref_bin0, const uint64_t* __restrict__ ref_off, uint8_t* __restrict__ dst, uint64_t cap) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n_runs; j += (uint64_t)gridDim.x * 256u) {
    uint64_t lo = 0, hi = n_bins;  // the last bin whose first run is <= j
    while (hi - lo > 1u) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (bin_first[mid] <= j) lo = mid; else hi = mid;
    }
    const uint64_t b = lo, bk = bin_key[b], row = bk >> BAI_BIN_BITS;
    const uint32_t q = run_perm[j];
    if (row >= n_ref || q >= n_runs) continue;
    const uint32_t rb0 = ref_bin0[row], f = bin_first[b];
    const uint64_t at = ref_off[row] + 4u + 8ull * (b - rb0) + 16ull * (f - bin_first[rb0]);  // the bin's head
    if (j == f) {
      bai_store32(dst, at, cap, (uint32_t)(bk & 0xffffu));
      bai_store32(dst, at + 4u, cap, bin_first[b + 1u] - f);
    }
    const uint64_t i0 = run_first[q], i1 = run_first[q + 1u];
    if (i0 > n || i1 > n) continue;
    const uint64_t c = at + 8u + 16ull * (j - f);
    bai_store64(dst, c, cap, bai_voff(base + rec_off[i0]));
    bai_store64(dst, c + 8u, cap, bai_voff(base + rec_off[i1]));
  }
}

// inclusive scan of the maximum over the 256-thread workgroup through LDS
SIMMR_DEV uint32_t bai_wg_scan_max(uint32_t v, uint32_t* lds) {
  const uint32_t t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < 256u; d <<= 1) {
    const uint32_t o = t >= d ? lds[t - d] : 0u;
    __syncthreads();
    lds[t] = lds[t] > o ? lds[t] : o;
    __syncthreads();
  }
  const uint32_t inc = lds[t];
  __syncthreads();
  return inc;
}

extern "C" __global__ void __launch_bounds__(256)
k_bai_write_refs(const uint32_t* __restrict__ ref_bin0, const uint32_t* __restrict__ ref_rec0, const uint32_t* __restrict__ bin_first,
                 const uint32_t* __restrict__ ref_intv, const uint64_t* __restrict__ ref_off, const uint64_t* __restrict__ win_off,
                 const uint64_t* __restrict__ win, const uint64_t* __restrict__ rec_off, uint64_t n, uint64_t n_ref, uint64_t base,
                 uint8_t* __restrict__ dst, uint64_t cap) {
  __shared__ uint32_t lds[256];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    bai_store32(dst, 0u, cap, 0x01494142u);  // "BAI\1"
    bai_store32(dst, 4u, cap, (uint32_t)n_ref);
    bai_store64(dst, ref_off[n_ref], cap, 0ull);  // n_no_coor
  }
  for (uint64_t r = blockIdx.x; r < n_ref; r += gridDim.x) {  // (uniform over the workgroup)
    const uint32_t b0 = ref_bin0[r], b1 = ref_bin0[r + 1u], n_intv = ref_intv[r];
    const uint64_t at = ref_off[r];
    if (b1 == b0) {
      if (threadIdx.x == 0) { bai_store32(dst, at, cap, 0u); bai_store32(dst, at + 4u, cap, 0u); }
      continue;
    }
    const uint64_t meta = at + 4u + 8ull * (b1 - b0) + 16ull * (bin_first[b1] - bin_first[b0]);
    if (threadIdx.x == 0) {
      const uint64_t i0 = ref_rec0[r], i1 = ref_rec0[r + 1u];
      bai_store32(dst, at, cap, b1 - b0 + 1u);
      bai_store32(dst, meta, cap, BAI_META_BIN);
      bai_store32(dst, meta + 4u, cap, 2u);
      bai_store64(dst, meta + 8u, cap, i0 <= n ? bai_voff(base + rec_off[i0]) : 0ull);
      bai_store64(dst, meta + 16u, cap, i1 <= n ? bai_voff(base + rec_off[i1]) : 0ull);
      bai_store64(dst, meta + 24u, cap, i1 - i0);  // n_mapped
      bai_store64(dst, meta + 32u, cap, 0ull);     // n_unmapped
      bai_store32(dst, meta + 40u, cap, n_intv);
    }
    // the linear index: window w shows the value of the last window <= w that a record overlaps (0: none yet)
    const uint64_t* mine = win + win_off[r];
    uint64_t carry = 0;  // the value behind the tile before
    for (uint32_t w0 = 0; w0 < n_intv; w0 += 256u) {
      const uint32_t w = w0 + threadIdx.x;
      const uint64_t v = w < n_intv ? mine[w] : ~0ull;
      const uint32_t last = bai_wg_scan_max(v != ~0ull ? threadIdx.x + 1u : 0u, lds);  // 1 + the tile's thread whose window shows here
      // (another thread's value is read from win[], which nobody writes in this kernel)
      const uint64_t shown = last ? mine[w0 + last - 1u] : carry;
      if (w < n_intv) bai_store64(dst, meta + 44u + 8ull * w, cap, shown);
      // the carry: what the tile's last thread shows, as two words
      if (threadIdx.x == 255u) { lds[0] = (uint32_t)shown; lds[1] = (uint32_t)(shown >> 32); }
      __syncthreads();
      carry = (uint64_t)lds[0] | ((uint64_t)lds[1] << 32);
      __syncthreads();
    }
  }
}

}  // namespace simmr
