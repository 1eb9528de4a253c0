// stats_kernels.hip — run statistics on the device (gfx950): quality, base and mismatch tables of the emitted reads,
// as integer sums in a simmr_run_stats (include/simmr_hip.h states every table).  Included by stats.hip behind
// truth_host.hpp; entry points simmr_stats_reset / simmr_stats_add / simmr_stats_read.
//
// One kernel, k_read_stats, one pass over the columns.  It walks the reads with the walker of truth_kernels.hip
// (walk_open / walk_window, shared with k_truth) — STATS_LANES = 16 lanes (one DPP row) share a read, a lane takes 16
// bases per round, the expected bytes come from gather_piece / expand4, a read's last 16-byte window of seq[] AND of
// qual[] ends at the read's end with the overlapped bits masked, reads under 16 bases are loaded bytewise, one bounds
// check keeps every load inside the read — and turns each base into adds on 32-bit tables in LDS.  The workgroup adds its LDS tables to the engine's 64-bit tables in HBM (the struct itself, word
// for word) and zeroes them; there is no second kernel.
//
// LDS, 36 616 bytes per workgroup (four workgroups of 256 per CU: 4 waves per SIMD):
//   words 0..705       reads, bases, qual_n, qual_mismatch, pair, nm_hist, gc_hist at the struct's own word offsets;
//   words 706..9153    the per-cycle tables, packed: four words per (block, offset j < 512)
//                        w0 = cycle_n | cycle_mismatch << 16      w1 = #A | #C << 16      w2 = #G | #T << 16      w3 = cycle_qsum
//                      (class "other" = n - A - C - G - T at the flush), so a base costs three adds, not five.
//                      A block is a row of the wave (row & 3): the four reads a wave-instruction serves never add to
//                      one address.  Read r is of set r % n_sets and r = 16 batch + row, so block b holds set b & 1
//                      (n_sets 2) or set 0 (n_sets 1), and the flush sums the blocks of a set.
//                      Inside a block offset j lies at (j & 256) + 16 (j & 15) + (j >> 4 & 15): the sixteen lanes of a
//                      row, at offsets 16 apart, add to sixteen consecutive words, and blocks are 528 = 16 mod 32 words
//                      apart, so the two rows of a 32-lane half use different halves of the banks.
// Tried: this form only (plain LDS adds on the conflict-free packed image).  Lanes that keep a cycle group in registers
// across reads (32 packed registers per lane and a shifted last window) and a wave-level pre-reduction over the four
// rows were weighed and not built; DESIGN.md §4 has the measured time and what bounds it.
//
// What bounds a 32-bit partial (for ANY n_reads): a workgroup flushes after every STATS_FLUSH_BATCHES = 4096 batches of
// 16 reads, and a read longer than STATS_MAX_L = 65 535 bases (the longest the simulator writes, a u16) is refused by
// the bounds check.  Between flushes a block sees 4 reads per batch: a 16-bit half is at most 16 384, cycle_qsum at
// most 255 * 16 384; a word of the small tables is at most the bases of the period, 4096 * 16 * 65 535 = 4 294 901 760
// < 2^32.  Per-lane class counts (two per register) are at most 16 * 256 rounds, per-row sums at most 65 535.
//
// Global adds: the grid is persistent, at most STATS_WGS_PER_CU = 4 workgroups per CU (1024 on 256 CUs), each looping
// over batches; zero entries are skipped.  A 150 bp paired shard has about 2 600 live entries (2 * 150 * 8 cycle words,
// ~80 quality, ~16 pair, ~10 nm, ~60 GC bins), so 100 M reads — 6 104 batches per workgroup, two flushes — queue about
// 1024 * 2 * 2 600 = 5.3 M 64-bit atomics per launch, against 1.5e10 bases read.
#pragma once

#include <cstddef>

namespace simmr {

#define STATS_LANES 16u            /* lanes per read: one DPP row */
#define STATS_WG_READS 16u         /* reads per 256-thread workgroup and batch */
#define STATS_WGS_PER_CU 4u        /* the grid is capped at this many workgroups per CU; beyond it workgroups loop */
#define STATS_FLUSH_BATCHES 4096u  /* a workgroup adds its LDS tables to HBM after this many batches */
#define STATS_MAX_L 65535u         /* longest read taken */
#define STATS_CYC_STRIDE 528u      /* words of one block of one packed cycle word: 512 offsets + 16 (bank skew) */

#define STATS_WORD(field) ((uint32_t)(offsetof(simmr_run_stats, field) / 8u))
#define STATS_SMALL_WORDS STATS_WORD(cycle_n)                    /* everything before the per-cycle tables */
#define STATS_TABLE_WORDS ((uint32_t)(sizeof(simmr_run_stats) / 8u))
#define STATS_LDS_WORDS (STATS_SMALL_WORDS + 4u * 4u * STATS_CYC_STRIDE)
static_assert(STATS_WORD(reads) == 0 && STATS_SMALL_WORDS == 706, "the LDS image mirrors the head of simmr_run_stats");
static_assert(STATS_LDS_WORDS * 4u <= 40960u, "four workgroups per CU");
static_assert((uint64_t)STATS_FLUSH_BATCHES * STATS_WG_READS * STATS_MAX_L < (1ull << 32), "a 32-bit partial must not wrap");
static_assert(STATS_FLUSH_BATCHES * 4u < 65536u, "a 16-bit half of a packed cycle word must not wrap");
static_assert(SIMMR_STATS_CYCLES == 512u && STATS_LANES * STATS_WG_READS == 256u, "the slot permutation is written for 512 offsets");

// A C G T -> 0 1 2 3, every other byte -> 4
SIMMR_DEV uint32_t stats_class(uint32_t x) {
  const uint32_t d = x - 0x41u, c = (x >> 1) & 3u;  // (x >> 1) & 3: A 0, C 1, T 2, G 3
  return (d < 20u && ((0x80045u >> d) & 1u)) ? (c ^ (c >> 1)) : 4u;
}
// byte B (a constant) of four words
#define STATS_BYTE(v, B) (((v)[(B) >> 2] >> (((B) & 3u) * 8u)) & 0xffu)

// tab: the engine's simmr_run_stats in HBM (STATS_TABLE_WORDS words); err: its sticky error word
__global__ void __launch_bounds__(256)
k_read_stats(const GenomeDev* __restrict__ genomes, uint32_t n_genomes, TruthReads rd, uint64_t n_reads, uint32_t n_sets,
             uint32_t qual_offset, unsigned long long* __restrict__ tab, uint32_t* __restrict__ err) {
  __shared__ uint32_t lds[STATS_LDS_WORDS];
  const uint32_t tid = threadIdx.x, sub = tid & (STATS_LANES - 1u), row = tid / STATS_LANES;
  const uint32_t set = n_sets == 2u ? (row & 1u) : 0u;
  uint32_t* const cyc = lds + STATS_SMALL_WORDS + (row & 3u) * STATS_CYC_STRIDE;  // this row's block of w0
  const uint32_t CW = 4u * STATS_CYC_STRIDE;                                     // from w0 to w1, w1 to w2, ...
  for (uint32_t i = tid; i < STATS_LDS_WORDS; i += 256u) lds[i] = 0u;
  __syncthreads();

  const uint64_t n_batches = (n_reads + STATS_WG_READS - 1u) / STATS_WG_READS;
  uint32_t since_flush = 0;
  for (uint64_t batch = blockIdx.x;; batch += gridDim.x) {  // (uniform over the workgroup)
    const bool more = batch < n_batches;
    if (!more || since_flush == STATS_FLUSH_BATCHES) {
      // add the workgroup's tables to HBM, zero entries skipped, and zero them
      __syncthreads();
      for (uint32_t i = tid; i < STATS_SMALL_WORDS; i += 256u) {
        const uint32_t v = lds[i];
        if (v) { atomicAdd(tab + i, (unsigned long long)v); lds[i] = 0u; }
      }
      for (uint32_t i = tid; i < n_sets * SIMMR_STATS_CYCLES; i += 256u) {
        const uint32_t m = i >> 9, j = i & 511u;
        uint32_t* const at = lds + STATS_SMALL_WORDS + (j & 256u) + ((j & 15u) << 4) + ((j >> 4) & 15u);
        uint32_t n = 0, mm = 0, a = 0, c = 0, g = 0, t = 0, qs = 0;
        for (uint32_t b = m; b < 4u; b += n_sets) {  // the blocks of set m
          uint32_t* const w = at + b * STATS_CYC_STRIDE;
          const uint32_t w0 = w[0], w1 = w[CW], w2 = w[2u * CW];
          if (w0) {
            n += w0 & 0xffffu; mm += w0 >> 16; a += w1 & 0xffffu; c += w1 >> 16; g += w2 & 0xffffu; t += w2 >> 16;
            qs += w[3u * CW];
            w[0] = 0u; w[CW] = 0u; w[2u * CW] = 0u; w[3u * CW] = 0u;
          }
        }
        if (n) {
          atomicAdd(tab + STATS_WORD(cycle_n) + i, (unsigned long long)n);
          if (qs) atomicAdd(tab + STATS_WORD(cycle_qsum) + i, (unsigned long long)qs);
          if (mm) atomicAdd(tab + STATS_WORD(cycle_mismatch) + i, (unsigned long long)mm);
          unsigned long long* const cb = tab + STATS_WORD(cycle_base) + i * 5u;
          const uint32_t other = n - a - c - g - t;
          if (a) atomicAdd(cb + 0, (unsigned long long)a);
          if (c) atomicAdd(cb + 1, (unsigned long long)c);
          if (g) atomicAdd(cb + 2, (unsigned long long)g);
          if (t) atomicAdd(cb + 3, (unsigned long long)t);
          if (other) atomicAdd(cb + 4, (unsigned long long)other);
        }
      }
      __syncthreads();
      since_flush = 0;
      if (!more) break;
    }
    since_flush++;

    const uint64_t r = batch * STATS_WG_READS + row;
    const ReadWalk w = walk_open<STATS_MAX_L>(genomes, n_genomes, rd, r, n_reads, err, 1u, sub == 0);
    const uint32_t L = w.L;
    const bool good = w.good;
    const uint8_t* seq = rd.seq + w.so;
    const uint8_t* qual = rd.qual + (rd.slot16 ? (w.so & ~15ull) : w.so);
    const uint32_t n_groups = (L + 15u) >> 4;
    uint32_t nm = 0, gc = 0, same01 = 0, same23 = 0;  // edits; 'G' + 'C' written; unedited A | C << 16 and G | T << 16
    for (uint32_t g0 = 0; g0 < n_groups; g0 += STATS_LANES) {  // (uniform over the row)
      const uint32_t grp = g0 + sub;
      if (grp >= n_groups) continue;
      const ReadWindow x = walk_window<true>(w, grp, seq, qual);
      const uint32_t k = x.k, keep = x.keep, diff = x.diff;
      const v4u32 have = x.have, qv = x.qv, want = x.want;
      nm += __builtin_popcount(diff);
#pragma unroll
      for (uint32_t b = 0; b < 16u; b++) {
        if (!((keep >> b) & 1u)) continue;
        const uint32_t c = stats_class(STATS_BYTE(have, b)), q = (STATS_BYTE(qv, b) - qual_offset) & 255u;
        const uint32_t d = (diff >> b) & 1u, j = k + b;
        const uint32_t half = 1u << ((c & 1u) * 16u);
        atomicAdd(&lds[STATS_WORD(qual_n) + q], 1u);
        if (d) {
          atomicAdd(&lds[STATS_WORD(qual_mismatch) + q], 1u);
          atomicAdd(&lds[STATS_WORD(pair) + stats_class(STATS_BYTE(want, b)) * 5u + c], 1u);
        } else {
          same01 += c < 2u ? half : 0u;
          same23 += (c & 6u) == 2u ? half : 0u;
        }
        gc += (c == 1u || c == 2u) ? 1u : 0u;
        if (j < SIMMR_STATS_CYCLES) {
          uint32_t* const w = cyc + (j & 256u) + ((j & 15u) << 4) + ((j >> 4) & 15u);
          atomicAdd(w, 1u + (d << 16));
          if (c < 4u) atomicAdd(w + (1u + (c >> 1)) * CW, half);
          atomicAdd(w + 3u * CW, q);
        }
      }
    }
    nm = row_inclusive_scan_u32(nm);
    gc = row_inclusive_scan_u32(gc);
    same01 = row_inclusive_scan_u32(same01);
    same23 = row_inclusive_scan_u32(same23);
    if (sub == STATS_LANES - 1u && good) {
      atomicAdd(&lds[STATS_WORD(reads) + set], 1u);
      atomicAdd(&lds[STATS_WORD(nm_hist) + (nm < SIMMR_STATS_NM_BINS ? nm : SIMMR_STATS_NM_BINS - 1u)], 1u);
      if (L) {
        atomicAdd(&lds[STATS_WORD(bases) + set], L);
        atomicAdd(&lds[STATS_WORD(gc_hist) + 100u * gc / L], 1u);
        // the diagonal of pair: the unedited bases by class; "other" is the rest
        const uint32_t sa = same01 & 0xffffu, sc = same01 >> 16, sg = same23 & 0xffffu, st = same23 >> 16;
        const uint32_t sx = L - nm - sa - sc - sg - st;
        if (sa) atomicAdd(&lds[STATS_WORD(pair) + 0u], sa);
        if (sc) atomicAdd(&lds[STATS_WORD(pair) + 6u], sc);
        if (sg) atomicAdd(&lds[STATS_WORD(pair) + 12u], sg);
        if (st) atomicAdd(&lds[STATS_WORD(pair) + 18u], st);
        if (sx) atomicAdd(&lds[STATS_WORD(pair) + 24u], sx);
      }
    }
  }
}

}  // namespace simmr
