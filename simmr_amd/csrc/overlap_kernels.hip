// overlap_kernels.hip — the true read-to-read overlaps as PAF text on the device (include/simmr_hip.h: simmr_overlap_*).
// Included by overlap.hip alone, the library's eighth translation unit.  Nothing of the reads' bytes is touched: the pass
// works on three engine-held columns per read — the key row << 40 | lo, a word L | rev << 40 | mate << 41, and the read id —
// which simmr_overlap_add appends range by range.  The sort is sam_sort.hip's (samsort_sort_pairs, engine_internal.hpp); the
// scans' bodies, the decimal pieces and the aligned LDS writer are those of sam_kernels.hip and fastq_format.hpp (included
// without their kernels).
//
// Eight kernels.  No place comes from an atomic (the only one is the error word): partners are counted, scanned, sized,
// scanned again, and every record is written at its offset, so launch geometry never changes a byte.
//   k_ovl_add       the three columns of a call's reads behind those already held, after the bound check
//                   (slot and contig staged, max(start, end) <= the contig's staged length);
//   k_ovl_keys      the sort key of every read: row << P | lo over the significant bits, or, for a read with L < min_overlap,
//                   n_rows << P — behind every row, so that such reads sort last and are partners of nothing;
//   k_ovl_partners  per place p (four consecutive places per thread): the read's word and id in sorted order, and
//                   cnt[p] = ub(p) - p - 1, ub(p) the first place whose key exceeds row_p << P | (hi_p - min_overlap), by a
//                   binary search on the sorted keys: the partners of p are exactly the places (p, ub(p)); the sum of every
//                   chunk of SAM_CHUNK counts;
//   k_ovl_scan      ONE workgroup: the exclusive scan of chunk sums (of the counts, then of the record bytes);
//   k_ovl_offsets   rec_off[p]: the index of the first record of place p, rec_off[n] = n_pairs (64 bits);
//   k_ovl_size      per chunk of OVL_CHUNK records: the sum of the records' bytes.  A record's size is recomputed wherever
//                   it is needed, never stored;
//   k_ovl_window    ONE workgroup: for a first place and a byte budget (or a number of places) the run of places, its records
//                   [j0, j1) and their bytes [b0, b1) — byte_at(j) is the chunk's prefix plus the recomputed sizes of the
//                   chunk's records before j;
//   k_ovl_write     a workgroup per chunk of records, 256 records a pass, one per thread: record j is (p, q) with
//                   p = the place whose records hold j (binary search in rec_off) and q = p + 1 + (j - rec_off[p]) — a pile
//                   of a thousand partners on one place is a thousand threads' work, not one's.  The pass's sizes are
//                   scanned, every thread formats its line into an LDS slot through aligned 32-bit stores, and four lanes
//                   a record copy the slots out in 16-byte windows (k_sam_write's copy), every store inside the record;
//                   the columns a, b, ref_start, ref_end, row of the same records, one entry per thread.
// LDS per workgroup: write 39 936 bytes (256 slots of OVL_PITCH: four workgroups a CU; the pass's scan uses the first KiB before
// the slots are written), window 1040 bytes, size 1 KiB, partners and offsets 2 KiB, scan 2 KiB, add and keys none.
#pragma once
#define SAM_ROUTINES_ONLY
#include "sam_kernels.hip"

namespace simmr {

#define OVL_CHUNK 1024u      /* records per chunk of the size pass and of the writer: four passes of 256 */
#define OVL_PITCH 156u       /* LDS bytes of a record's slot: 144 (two names of 12, eight numbers of 13, "255", the strand, twelve
                                separators) and the aligned writer's two words of slack; an odd number of words */
#define OVL_POS_BITS 40u     /* the canonical key: row << 40 | lo */
#define OVL_L_MASK ((1ull << 40) - 1ull)
#define OVL_REV_BIT (1ull << 40)
#define OVL_MATE_BIT (1ull << 41)
#define OVL_WGS_PER_CU 8u

struct OvlRows {  // the rows the reset fixed (device pointers)
  const uint32_t* g_cbase;    // per engine genome slot: the row of its first contig
  const uint32_t* g_ncontig;  // 0: the slot is not staged
  const uint64_t* c_bases;    // per row: the contig's staged length
  uint32_t n_slots;
};
struct OvlSorted {  // what the plan keeps, in place order (device pointers)
  const uint64_t* key;      // the sort keys, ascending: row << pos_bits | lo
  const uint64_t* meta;     // L | rev << 40 | mate << 41
  const uint32_t* rid;
  const uint32_t* perm;     // place -> ordinal
  const uint64_t* rec_off;  // n + 1
  uint64_t n, n_pairs;
  uint32_t pos_bits, paired;
};
struct OvlCols {  // simmr_overlap_cols, any of them NULL
  uint32_t* a;
  uint32_t* b;
  uint64_t* ref_start;
  uint64_t* ref_end;
  uint32_t* row;
};

// ---- the columns of a call ------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
k_ovl_add(const uint64_t* __restrict__ start, const uint64_t* __restrict__ end, const uint32_t* __restrict__ contig,
          const uint32_t* __restrict__ genome, const uint32_t* __restrict__ read_id, const uint8_t* __restrict__ flags, uint64_t n_reads,
          const OvlRows rows, uint32_t paired, uint64_t* __restrict__ key, uint64_t* __restrict__ meta, uint32_t* __restrict__ rid,
          uint32_t* __restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_reads) return;
  const uint64_t a = start[i], b = end[i];
  const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
  const uint32_t g = genome[i], c = contig[i];
  bool ok = g < rows.n_slots;
  if (ok) ok = c < rows.g_ncontig[g];
  uint64_t row = 0;
  if (ok) {
    row = (uint64_t)rows.g_cbase[g] + c;
    ok = hi <= rows.c_bases[row];  // (below 2^40: the reset refused longer contigs)
  }
  if (!ok) {
    atomicOr(err, 1u);
    return;
  }
  key[i] = (row << OVL_POS_BITS) | lo;
  meta[i] = (hi - lo) | ((flags[i] & SIMMR_FLAG_REVCOMP) ? OVL_REV_BIT : 0ull) | ((paired && (i & 1u)) ? OVL_MATE_BIT : 0ull);
  rid[i] = read_id[i];
}

extern "C" __global__ void __launch_bounds__(256)
k_ovl_keys(const uint64_t* __restrict__ key, const uint64_t* __restrict__ meta, uint64_t n, uint64_t min_overlap, uint32_t pos_bits,
           uint64_t n_rows, uint64_t* __restrict__ skey) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = key[i];
  const bool in = (meta[i] & OVL_L_MASK) >= min_overlap;
  skey[i] = in ? (((k >> OVL_POS_BITS) << pos_bits) | (k & OVL_L_MASK)) : (n_rows << pos_bits);
}

// ---- partners ---------------------------------------------------------------------------------------------------------------
// the first place in (p, n) whose key exceeds `bound` (keys ascend)
SIMMR_DEV uint64_t ovl_upper(const uint64_t* __restrict__ key, uint64_t p, uint64_t n, uint64_t bound) {
  uint64_t lo = p + 1u, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (key[mid] <= bound) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

extern "C" __global__ void __launch_bounds__(256)
k_ovl_partners(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ perm, const uint64_t* __restrict__ meta,
               const uint32_t* __restrict__ rid, uint64_t n, uint64_t min_overlap, uint32_t pos_bits, uint64_t n_rows,
               uint64_t* __restrict__ smeta, uint32_t* __restrict__ srid, uint32_t* __restrict__ cnt, uint64_t* __restrict__ chunk_sum) {
  __shared__ uint64_t lds[256];
  const uint64_t n_chunks = (n + SAM_CHUNK - 1u) / SAM_CHUNK;
  const uint64_t lo_mask = (1ull << pos_bits) - 1ull;  // (pos_bits <= 40)
  for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // (uniform over the workgroup)
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
      const uint64_t p = chunk * SAM_CHUNK + 4u * threadIdx.x + q;
      if (p >= n) continue;
      const uint64_t r = perm ? perm[p] : p;
      const uint64_t m = r < n ? meta[r] : 0ull, k = skey[p];
      smeta[p] = m;
      srid[p] = r < n ? rid[r] : 0u;
      uint32_t c = 0;
      if ((k >> pos_bits) < n_rows) {  // (a read with L >= min_overlap: hi - min_overlap >= lo stays inside the position bits)
        const uint64_t bound = (k & ~lo_mask) | ((k & lo_mask) + (m & OVL_L_MASK) - min_overlap);
        c = (uint32_t)(ovl_upper(skey, p, n, bound) - p - 1u);  // (fewer than 2^31 reads)
      }
      cnt[p] = c;
      sum += c;
    }
    uint64_t total;
    (void)sam_wg_scan<uint64_t>(sum, lds, &total);
    if (threadIdx.x == 0) chunk_sum[chunk] = total;
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_ovl_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

// sam_chunk_offsets with a 64-bit scan inside the chunk: 1024 places may hold more than 2^32 records
extern "C" __global__ void __launch_bounds__(256)
k_ovl_offsets(const uint32_t* __restrict__ cnt, const uint64_t* __restrict__ prefix, uint64_t n, uint64_t* __restrict__ rec_off) {
  __shared__ uint64_t lds[256];
  const uint64_t n_chunks = (n + SAM_CHUNK - 1u) / SAM_CHUNK;
  if (blockIdx.x == 0 && threadIdx.x == 0) rec_off[n] = prefix[n_chunks];
  for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // (uniform over the workgroup)
    const uint64_t p0 = chunk * SAM_CHUNK + 4u * threadIdx.x;
    uint32_t v[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) v[k] = p0 + k < n ? cnt[p0 + k] : 0u;
    uint64_t total;
    uint64_t ex = sam_wg_scan<uint64_t>((uint64_t)v[0] + v[1] + v[2] + v[3], lds, &total);
    const uint64_t base = prefix[chunk];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
      if (p0 + k < n) rec_off[p0 + k] = base + ex;
      ex += v[k];
    }
  }
}

// ---- a record -----------------------------------------------------------------------------------------------------------------
struct OvlRec {
  uint64_t Lq, qs, qe, Lt, ts, te, ov, s, e;
  uint32_t idq, idt, mq, mt, same, row, p, q;
};
// record j < n_pairs: the place p with rec_off[p] <= j < rec_off[p + 1] and its partner j - rec_off[p] places behind it
SIMMR_DEV OvlRec ovl_open(const OvlSorted& S, uint64_t j) {
  uint64_t lo = 0, hi = S.n;  // the first place whose rec_off exceeds j, in (0, n]
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (S.rec_off[mid] <= j) lo = mid + 1u; else hi = mid;
  }
  const uint64_t p = lo - 1u;
  uint64_t q = p + 1u + (j - S.rec_off[p]);
  if (q >= S.n) q = S.n - 1u;  // (it is not: the counts are those of these keys)
  const uint64_t lo_mask = (1ull << S.pos_bits) - 1ull;
  const uint64_t kp = S.key[p], kq = S.key[q], mp = S.meta[p], mq = S.meta[q];
  const uint64_t lo_p = kp & lo_mask, lo_q = kq & lo_mask, hi_p = lo_p + (mp & OVL_L_MASK), hi_q = lo_q + (mq & OVL_L_MASK);
  OvlRec R;
  R.s = lo_q > lo_p ? lo_q : lo_p;
  R.e = hi_p < hi_q ? hi_p : hi_q;
  if (R.e < R.s) R.e = R.s;
  R.ov = R.e - R.s;
  R.Lq = mp & OVL_L_MASK;
  R.Lt = mq & OVL_L_MASK;
  const bool rp = (mp & OVL_REV_BIT) != 0, rq = (mq & OVL_REV_BIT) != 0;
  R.qs = rp ? hi_p - R.e : R.s - lo_p;
  R.qe = R.qs + R.ov;
  R.ts = rq ? hi_q - R.e : R.s - lo_q;
  R.te = R.ts + R.ov;
  R.same = rp == rq ? 1u : 0u;
  R.idq = S.rid[p];
  R.idt = S.rid[q];
  R.mq = (mp & OVL_MATE_BIT) ? 1u : 0u;
  R.mt = (mq & OVL_MATE_BIT) ? 1u : 0u;
  R.row = (uint32_t)(kp >> S.pos_bits);
  R.p = (uint32_t)p;
  R.q = (uint32_t)q;
  return R;
}
SIMMR_DEV uint32_t ovl_len(const OvlRec& R, uint32_t paired) {
  return dec_digits(R.idq) + dec_digits(R.idt) + (paired ? 4u : 0u) + dec_digits(R.Lq) + dec_digits(R.qs) + dec_digits(R.qe) +
         dec_digits(R.Lt) + dec_digits(R.ts) + dec_digits(R.te) + 2u * dec_digits(R.ov) + 16u;  // the strand, "255", twelve separators
}
SIMMR_DEV uint32_t ovl_size(const OvlSorted& S, uint64_t j) {
  if (j >= S.n_pairs) return 0u;
  const OvlRec R = ovl_open(S, j);
  return ovl_len(R, S.paired);
}
// The line into an LDS slot.  Ten pieces — a literal of up to three bytes, then a number — in ONE loop, so that the decimal
// writer exists once in the kernel: the query's id, L, start, end; the strand and the target's id, L, start, end; ov twice.
SIMMR_DEV uint32_t ovl_format(uint8_t* slot, const OvlRec& R, uint32_t paired) {
  FqW o = fq_begin(slot);
#pragma clang loop unroll(disable)
  for (uint32_t i = 0; i < 10u; i++) {
    uint64_t lit = sam_lit("\t"), v = R.ov;
    uint32_t ln = 1u;
    if (i == 0u) { v = R.idq; ln = 0u; }
    else if (i == 1u || i == 5u) {  // behind a name: the mate, if the run is paired
      v = i == 1u ? R.Lq : R.Lt;
      if (paired) { lit = (i == 1u ? R.mq : R.mt) ? sam_lit("/2\t") : sam_lit("/1\t"); ln = 3u; }
    }
    else if (i == 2u) v = R.qs;
    else if (i == 3u) v = R.qe;
    else if (i == 4u) { lit = R.same ? sam_lit("\t+\t") : sam_lit("\t-\t"); ln = 3u; v = R.idt; }
    else if (i == 6u) v = R.ts;
    else if (i == 7u) v = R.te;
    if (ln) fq_put8(o, lit, ln);
    fq_put_dec(o, v);
  }
  fq_put8(o, sam_lit("\t255\n"), 5u);
  return o.at;
}

// the sum of one value per thread over the workgroup (lds: 256 words)
SIMMR_DEV uint32_t ovl_wg_sum(uint32_t v, uint32_t* lds) {
  uint32_t total;
  (void)sam_wg_scan<uint32_t>(v, lds, &total);
  return total;
}

extern "C" __global__ void __launch_bounds__(256)
k_ovl_size(const OvlSorted S, uint64_t* __restrict__ chunk_sum) {
  __shared__ uint32_t lds[256];
  const uint64_t n_chunks = (S.n_pairs + OVL_CHUNK - 1u) / OVL_CHUNK;
  for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // (uniform over the workgroup)
    uint32_t acc = 0;  // (a record is at most 144 bytes)
    for (uint32_t it = 0; it < OVL_CHUNK / 256u; it++) acc += ovl_size(S, chunk * OVL_CHUNK + it * 256u + threadIdx.x);
    const uint32_t total = ovl_wg_sum(acc, lds);
    if (threadIdx.x == 0) chunk_sum[chunk] = total;
  }
}

// the bytes before record j (j <= n_pairs), by the whole workgroup
SIMMR_DEV uint64_t ovl_byte_at(const OvlSorted& S, const uint64_t* __restrict__ prefix, uint64_t j, uint32_t* lds) {
  const uint64_t c = j / OVL_CHUNK;
  uint32_t acc = 0;
  for (uint32_t it = 0; it < OVL_CHUNK / 256u; it++) {
    const uint64_t k = c * OVL_CHUNK + it * 256u + threadIdx.x;
    if (k < j) acc += ovl_size(S, k);
  }
  return prefix[c] + ovl_wg_sum(acc, lds);
}

// out[0] = n_places, out[1] = j0, out[2] = j1, out[3] = b0, out[4] = b1, out[5] = the bytes of place `first` alone.
// fixed_places != ~0: the run is that many places; else the longest run whose bytes fit max_bytes.  first <= n.
extern "C" __global__ void __launch_bounds__(256)
k_ovl_window(const OvlSorted S, const uint64_t* __restrict__ prefix, uint64_t first, uint64_t max_bytes, uint64_t fixed_places,
             uint64_t* __restrict__ out) {
  __shared__ uint32_t lds[256];
  __shared__ uint64_t bc[2];
  const uint64_t n_chunks = (S.n_pairs + OVL_CHUNK - 1u) / OVL_CHUNK;
  const uint64_t j0 = S.rec_off[first];
  const uint64_t b0 = ovl_byte_at(S, prefix, j0, lds);
  const uint64_t jn = first < S.n ? S.rec_off[first + 1u] : j0;
  const uint64_t need = ovl_byte_at(S, prefix, jn, lds) - b0;
  uint64_t last;
  if (fixed_places != ~0ull) {
    last = first + fixed_places;  // (the host has checked it against n)
  } else {
    const uint64_t limit = b0 + max_bytes < b0 ? ~0ull : b0 + max_bytes;
    if (threadIdx.x == 0) {  // the last chunk whose prefix is within the limit (prefix[0] = 0 is)
      uint64_t lo = 0, hi = n_chunks;
      while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo + 1u) >> 1);
        if (prefix[mid] <= limit) lo = mid; else hi = mid - 1u;
      }
      bc[0] = lo;
    }
    __syncthreads();
    const uint64_t c = bc[0];
    uint64_t J = S.n_pairs;
    if (c < n_chunks) {  // the records of chunk c that end within the limit (uniform over the workgroup)
      uint64_t run = prefix[c];
      uint32_t fit = 0;
      for (uint32_t it = 0; it < OVL_CHUNK / 256u; it++) {
        const uint64_t k = c * OVL_CHUNK + it * 256u + threadIdx.x;
        const uint32_t sz = ovl_size(S, k);
        uint32_t total;
        const uint32_t ex = sam_wg_scan<uint32_t>(sz, lds, &total);
        if (k < S.n_pairs && run + ex + sz <= limit) fit++;
        run += total;
      }
      J = c * OVL_CHUNK + ovl_wg_sum(fit, lds);
    }
    if (threadIdx.x == 0) {  // the last place whose first record is at or before J, in [first, n]
      uint64_t lo = first, hi = S.n;
      while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo + 1u) >> 1);
        if (S.rec_off[mid] <= J) lo = mid; else hi = mid - 1u;
      }
      bc[1] = lo;
    }
    __syncthreads();
    last = bc[1];
  }
  const uint64_t j1 = S.rec_off[last];
  const uint64_t b1 = ovl_byte_at(S, prefix, j1, lds);
  if (threadIdx.x == 0) {
    out[0] = last - first; out[1] = j0; out[2] = j1; out[3] = b0; out[4] = b1; out[5] = need;
  }
}

// ---- the records --------------------------------------------------------------------------------------------------------------
// records [j0, j1) at dst[byte_at(j) - b0]; `bytes` = byte_at(j1) - b0 bounds every store
extern "C" __global__ void __launch_bounds__(256)
k_ovl_write(const OvlSorted S, const uint64_t* __restrict__ prefix, uint64_t j0, uint64_t j1, uint64_t b0, uint64_t bytes,
            uint8_t* __restrict__ dst, const OvlCols cols) {
  // a slot: the line (at most 144 bytes; the aligned writer and the window reads touch words 0 .. 36), then its length and its
  // offset in the pass in words 37 and 38
  __shared__ __attribute__((aligned(16))) uint8_t slots[256u * OVL_PITCH];
  uint32_t* scan = reinterpret_cast<uint32_t*>(slots);
  const uint32_t t = threadIdx.x;
  const uint64_t c_first = j0 / OVL_CHUNK, c_end = (j1 + OVL_CHUNK - 1u) / OVL_CHUNK;
  for (uint64_t chunk = c_first + blockIdx.x; chunk < c_end; chunk += gridDim.x) {  // (uniform over the workgroup)
    uint64_t run = prefix[chunk];
    for (uint32_t it = 0; it < OVL_CHUNK / 256u; it++) {
      const uint64_t j = chunk * OVL_CHUNK + it * 256u + t;
      const bool have = j < S.n_pairs;
      OvlRec R{};
      if (have) R = ovl_open(S, j);
      const uint32_t sz = have ? ovl_len(R, S.paired) : 0u;
      uint32_t total;
      const uint32_t ex = sam_wg_scan<uint32_t>(sz, scan, &total);  // (ends with a barrier: the slots are free for the lines)
      const bool mine = have && j >= j0 && j < j1;
      const uint64_t pass_at = run - b0;  // (wraps for a pass before the run's first record: no record of it is `mine`)
      const uint64_t at = pass_at + ex;
      run += total;
      if (mine) {
        const uint64_t k = j - j0;
        const uint32_t a = S.perm ? S.perm[R.p] : R.p, b = S.perm ? S.perm[R.q] : R.q;
        if (cols.a) cols.a[k] = a;
        if (cols.b) cols.b[k] = b;
        if (cols.ref_start) cols.ref_start[k] = R.s;
        if (cols.ref_end) cols.ref_end[k] = R.e;
        if (cols.row) cols.row[k] = R.row;
      }
      if (dst) {  // (uniform)
        uint32_t wrote = 0;
        if (mine) wrote = ovl_format(slots + t * OVL_PITCH, R, S.paired);
        // a line whose bytes differ from its size, or that would leave dst[0, bytes), is not copied
        uint32_t* tail = reinterpret_cast<uint32_t*>(slots + t * OVL_PITCH) + 37;
        tail[0] = (mine && wrote == sz && at <= bytes && bytes - at >= sz) ? sz : 0u;
        tail[1] = ex;
        __syncthreads();
        // four lanes a record, 64 records a round: window g of a line starts at byte 16 g, the last one ends at the line's end
        for (uint32_t round = 0; round < 4u; round++) {
          const uint32_t rec = round * 64u + (t >> 2);
          const uint8_t* slot = slots + rec * OVL_PITCH;
          const uint32_t n = reinterpret_cast<const uint32_t*>(slot)[37];
          if (n == 0u) continue;
          uint8_t* line = dst + (pass_at + reinterpret_cast<const uint32_t*>(slot)[38]);
          const uint32_t nw = (n + 15u) >> 4;  // (a line is at least 26 bytes)
          for (uint32_t g = t & 3u; g < nw; g += 4u) {
            const uint32_t k = 16u * g + 16u <= n ? 16u * g : n - 16u;
            sam_store16(line, k, n, fq_read16(slot, k));
          }
        }
        __syncthreads();  // the next pass scans in the slots
      }
    }
  }
}

}  // namespace simmr
