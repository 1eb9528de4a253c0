// sam_sort_kernels.hip — the true alignments in coordinate order (include/simmr_hip.h: simmr_sam_sort_*): a stable radix sort
// of (key, read) pairs on the device, the record sizes scanned in sorted order, and the records of sam_kernels.hip written
// at their sorted places.  Included by sam_sort.hip alone, the library's seventh translation unit.  The record routine, the
// scans' bodies and the constants are those of sam_kernels.hip (included without its kernels): a line's bytes cannot differ
// from simmr_sam_emit's, only its place does.
//
// Eight kernels.  No place comes from the order in which atomics land: the only atomics are the counts of a histogram
// (a sum does not depend on its order) and the error word.
//   k_samsort_size        every record's length, as k_sam_size finds it, and its sort key row << P | lo, after the bound
//                         check that gives the key its width: max(start, end) <= the staged length of the read's contig;
//   k_samsort_hist        per pass, per tile of SAMSORT_TILE pairs: the counts of the pass's digit, stored digit-major
//                         (hist[d * n_tiles + tile]);
//   k_samsort_digit_scan  per pass, a workgroup per digit: the exclusive scan of that digit's counts over the tiles and
//                         the digit's total — with the 256 totals scanned in the scatter, one scan over digits x tiles;
//   k_samsort_scatter     per pass, per tile: pair i goes to (pairs of smaller digits) + (pairs of its digit in earlier
//                         tiles) + (pairs of its digit earlier in the tile): stable;
//   k_samsort_gather      the lengths in sorted order (len[perm[i]]), the sum of every chunk of SAM_CHUNK of them, and the
//                         canonical key row << 40 | lo of every place;
//   k_samsort_scan, k_samsort_offsets   the chunked scan of sam_kernels.hip over the sorted lengths: line_off[0 .. n];
//   k_samsort_write       SamRec::write for place i with r = perm[i]: every store bounded by line_off[i + 1] - line_off[i].
// The bodies of the size, gather and write kernels are rec_size_keyed, rec_gather and rec_write_places of record_stream.hpp,
// shared with the sorted BAM (bam_index_kernels.hip); the radix passes are this file's own.
//
// A tile is a fixed 2048 pairs whatever the grid, so the histogram's layout is a function of n alone.  Wave w of the four
// owns pairs 512 w .. 512 w + 511 of the tile, 64 at a time (eight rounds): a pair's rank inside the tile is
//   (pairs of its digit in the waves before) + (pairs of its digit in the wave's earlier rounds) + (lanes below it in the
//   round with the same digit),
// the last from eight ballots (one per bit of the digit), the middle from a running count per wave and digit in LDS that
// only the wave itself reads and writes, the first from those counts once every wave is done.
//
// Digits are 8 bits: 256 counters per wave fit LDS four times over (4 KiB), a pass's histogram is n / 8 words, and the
// widths that occur — 23 bits for one bacterial contig, 27 to 33 for a hundred genomes — take three to five passes; 11-bit
// digits would save one pass of those at eight times the counters and a scan eight times as long.
// LDS per workgroup: scatter 6 KiB (counts 4 KiB, digit bases 1 KiB, scan 1 KiB), hist 1 KiB, digit_scan 1 KiB, gather
// 1 KiB, scan 2 KiB, offsets 1 KiB, write 6400 bytes (the head and tail slots of k_sam_write), size none.
#pragma once
#define SAM_ROUTINES_ONLY
#include "sam_kernels.hip"

namespace simmr {

#define SAMSORT_DIGIT_BITS 8u   /* bits per pass */
#define SAMSORT_TILE 2048u      /* pairs per workgroup and pass: four waves x eight rounds x 64 lanes */
#define SAMSORT_ROUNDS 8u
#define SAMSORT_DIGITS (1u << SAMSORT_DIGIT_BITS)
#define SAMSORT_KEY_POS_BITS 40u /* the canonical key: row << 40 | lo (REC_KEY_POS_BITS, record_stream.hpp) */

static_assert(SAMSORT_TILE == 4u * SAMSORT_ROUNDS * 64u, "a tile is four waves of eight rounds");
static_assert(SAMSORT_DIGITS == 256u, "one digit per thread of the workgroup");
static_assert(SAMSORT_KEY_POS_BITS == REC_KEY_POS_BITS, "one canonical key for the sorted SAM, the sorted BAM and the index");

// ---- sizes and keys ---------------------------------------------------------------------------------------------------
// A workgroup takes chunks of SAM_CHUNK consecutive reads, 16 at a time, a row of 16 lanes per read.  A read outside its
// contig (or without a named contig) sets the error word and has nothing else loaded or stored for it but a zero length and key.
extern "C" __global__ void __launch_bounds__(256)
k_samsort_size(const SamReads rd, const SamEdits ed, const SamNames nm, const uint64_t* __restrict__ c_bases, uint64_t n_reads, uint32_t paired,
               uint32_t pos_bits, uint32_t* __restrict__ len, uint64_t* __restrict__ key, uint32_t* __restrict__ err) {
  rec_size_keyed<SamRec, false>(rd, ed, nm, c_bases, n_reads, paired, pos_bits, len, key, nullptr, err);
}

// ---- a pass of the sort -------------------------------------------------------------------------------------------------
SIMMR_DEV uint32_t samsort_digit(uint64_t k, uint32_t shift) { return (uint32_t)(k >> shift) & (SAMSORT_DIGITS - 1u); }

extern "C" __global__ void __launch_bounds__(256)
k_samsort_hist(const uint64_t* __restrict__ key, uint64_t n, uint32_t shift, uint32_t* __restrict__ hist, uint32_t n_tiles) {
  __shared__ uint32_t h[SAMSORT_DIGITS];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * SAMSORT_TILE;
#pragma unroll
  for (uint32_t j = 0; j < SAMSORT_ROUNDS; j++) {
    const uint64_t i = base + j * 256u + threadIdx.x;
    if (i < n) atomicAdd(&h[samsort_digit(key[i], shift)], 1u);
  }
  __syncthreads();
  hist[(uint64_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// workgroup d: hist[d][0 .. n_tiles) becomes its exclusive scan, digit_total[d] the sum
extern "C" __global__ void __launch_bounds__(256)
k_samsort_digit_scan(uint32_t* __restrict__ hist, uint32_t n_tiles, uint32_t* __restrict__ digit_total) {
  __shared__ uint32_t lds[256];
  uint32_t* rowp = hist + (uint64_t)blockIdx.x * n_tiles;
  uint32_t carry = 0;  // (fewer than 2^31 pairs)
  for (uint32_t base = 0; base < n_tiles; base += 256u) {  // (uniform over the workgroup)
    const uint32_t i = base + threadIdx.x;
    uint32_t total;
    const uint32_t ex = sam_wg_scan<uint32_t>(i < n_tiles ? rowp[i] : 0u, lds, &total);
    if (i < n_tiles) rowp[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) digit_total[blockIdx.x] = carry;
}

// idx_in == nullptr: the first pass, pair i is read i
extern "C" __global__ void __launch_bounds__(256)
k_samsort_scatter(const uint64_t* __restrict__ key_in, const uint32_t* __restrict__ idx_in, uint64_t* __restrict__ key_out,
                  uint32_t* __restrict__ idx_out, uint64_t n, uint32_t shift, const uint32_t* __restrict__ hist,
                  const uint32_t* __restrict__ digit_total, uint32_t n_tiles) {
  __shared__ uint32_t cnt[4][SAMSORT_DIGITS];  // per wave and digit: the running count, then the wave's base
  __shared__ uint32_t gbase[SAMSORT_DIGITS];   // where the tile's pairs of a digit begin
  __shared__ uint32_t lds[256];
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) cnt[k][t] = 0u;
  uint32_t all;
  const uint32_t before = sam_wg_scan<uint32_t>(digit_total[t], lds, &all);  // pairs of smaller digits
  gbase[t] = before + hist[(uint64_t)t * n_tiles + blockIdx.x];
  __syncthreads();
  volatile uint32_t* mine = cnt[w];
  const uint64_t base = (uint64_t)blockIdx.x * SAMSORT_TILE + w * (SAMSORT_ROUNDS * 64u) + lane;
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t k[SAMSORT_ROUNDS];
  uint32_t rank[SAMSORT_ROUNDS];
#pragma unroll
  for (uint32_t j = 0; j < SAMSORT_ROUNDS; j++) {
    const uint64_t i = base + j * 64u;
    const bool valid = i < n;
    k[j] = valid ? key_in[i] : 0ull;
    const uint32_t d = samsort_digit(k[j], shift);
    uint64_t same = __ballot(valid);  // the lanes of the round with this lane's digit
#pragma unroll
    for (uint32_t b = 0; b < SAMSORT_DIGIT_BITS; b++) {
      const bool bit = (d >> b) & 1u;
      const uint64_t bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const uint32_t lower = (uint32_t)__popcll(same & below);
    uint32_t prev = 0;
    if (valid) prev = mine[d];
    __builtin_amdgcn_wave_barrier();  // (every lane has read the count before the first lane of a digit moves it on)
    if (valid && lower == 0u) mine[d] = prev + (uint32_t)__popcll(same);
    __builtin_amdgcn_wave_barrier();
    rank[j] = prev + lower;
  }
  __syncthreads();
  {
    uint32_t at = gbase[t];
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
      const uint32_t c = cnt[q][t];
      cnt[q][t] = at;
      at += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < SAMSORT_ROUNDS; j++) {
    const uint64_t i = base + j * 64u;
    if (i >= n) continue;
    const uint64_t to = (uint64_t)cnt[w][samsort_digit(k[j], shift)] + rank[j];
    if (to < n) {  // (it is: the counts are those of these pairs)
      key_out[to] = k[j];
      idx_out[to] = idx_in ? idx_in[i] : (uint32_t)i;
    }
  }
}

// ---- the sorted lengths ---------------------------------------------------------------------------------------------------
// a workgroup per chunk, four consecutive places per thread; perm == nullptr: place i holds read i (a key without bits)
extern "C" __global__ void __launch_bounds__(256)
k_samsort_gather(const uint32_t* __restrict__ len, const uint64_t* __restrict__ key, const uint32_t* __restrict__ perm, uint64_t n,
                 uint32_t pos_bits, uint32_t* __restrict__ slen, uint64_t* __restrict__ ckey, uint64_t* __restrict__ chunk_sum) {
  __shared__ uint32_t lds[256];
  rec_gather<false>(len, nullptr, key, perm, n, pos_bits, slen, nullptr, ckey, chunk_sum, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_samsort_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_samsort_offsets(const uint32_t* __restrict__ slen, const uint64_t* __restrict__ prefix, uint64_t n, uint64_t* __restrict__ line_off) {
  __shared__ uint32_t lds[256];
  sam_chunk_offsets(slen, prefix, n, line_off, lds);
}

// ---- the records, in order -------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
k_samsort_write(const SamReads rd, const SamEdits ed, const SamNames nm, uint64_t n_reads, uint32_t paired, const uint32_t* __restrict__ perm,
                const uint64_t* __restrict__ line_off, uint8_t* __restrict__ dst, uint32_t* __restrict__ err) {
  __shared__ __attribute__((aligned(16))) uint8_t slots[SAM_WG_READS][SamRec::SLOT_BYTES];
  rec_write_places<SamRec, true>(rd, ed, nm, n_reads, paired, perm, line_off, dst, err, &slots[0][0]);
}

}  // namespace simmr
