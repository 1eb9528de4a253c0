// asmmap_kernels.hip — an assembler's contigs PLACED on the gold-standard assembly by unique canonical k-mers (gfx950): anchor
// hits, collinear runs, blocks and the breakpoints between them (include/simmr_hip.h states every rule).  Included by asmmap.hip
// alone, a translation unit of its own.  The text, the planes, the roll and the lookup are asmeval's, taken and not restated:
// asm_roll_at, asm_find, asm_upper_bound, AsmPlane and AsmEntries of asmeval_kernels.hip through ASM_ROUTINES_ONLY (which brings
// MEV_ROUTINES_ONLY and FSAM_ROUTINES_ONLY with it); the text-to-planes kernels through asmeval_front.hpp.
//
// Truth add:  front -> genomes -> k_amap_truth_records -> k_amap_roll_truth.
//   k_amap_truth_records  a record a thread: the row t = records before the add + r, its genome and its length.
//   k_amap_roll_truth     asm_roll_at twice, as k_asm_roll_truth: the count, a wave scan and ONE atomic a wave, then the stores of
//                         (key, t << 1 | o, p); p = the k-mer's first base in its record.
// Plan:  samsort_sort_pairs -> k_amap_marks -> two scans -> k_amap_index -> k_amap_table (twice) -> k_amap_reduce_truth.
//   k_amap_marks          a sorted occurrence a thread: anchor = its key differs from both neighbours; repeat = the head of a run
//                         of two or more.
//   k_amap_index          the compaction behind the scans: the anchor index (key, t, p, o) and the distinct repeat keys.
//   k_amap_table          THE PREFIX TABLE, asmeval's rule (min(24, bit length of the entries) bits): a thread a bucket.
//   k_amap_reduce_truth   by_genome's truth_bases (over the truth records) and truth_anchors (over the anchors), through LDS.
// Add:  front -> k_amap_contig_len -> k_amap_roll_count -> scan -> k_amap_roll_write -> k_amap_run_heads -> scan -> k_amap_runs ->
//       k_amap_kept -> scan -> k_amap_kept_runs -> k_amap_block_heads -> scan -> k_amap_blocks -> k_amap_block_span -> k_amap_joins.
//   k_amap_roll_count     a lane takes the 32 k-mer ends of one validity word: every key is looked up among the anchors and, on
//                         a miss, among the repeats; the lane's anchor hits go to lane_hits[word] (the input of the scan), its hits
//                         per contig to the contig's column, and the sums of k-mers, hits and repeat hits to ONE atomic a wave each.
//   k_amap_roll_write     the same walk behind the scan: hit (contig, q, t << 1 | s, d) at the lane's offset, so the hits stand in
//                         (contig, q) order without an atomic.
//   k_amap_run_heads      1 where a hit starts a run (the contig, t or s changes, or |d - d_prev| > band).
//   k_amap_runs           behind the scan: a run's first and last hit.
//   k_amap_kept           1 where a run has min_anchors hits or more; the others are counted (runs_dropped, stray_hits).
//   k_amap_kept_runs      the compaction of the kept runs (first and last hit).
//   k_amap_block_heads    1 where a kept run starts a block (the rule of the runs, between the previous kept run's last hit and
//                         this one's first).
//   k_amap_blocks         a kept run a thread: the block's contig, truth record, strand, q_start, q_end, hits (an atomic add a run)
//                         and the d of its first and last hit.
//   k_amap_block_span     a hit a thread: p_start and p_end by atomic minimum and maximum, ONE pair a wave where the wave's hits
//                         are all of one block.
//   k_amap_joins          a block a thread: the class of the step from the block before it; the contig's blocks, block bases,
//                         first block and worst join.
// Read:  k_amap_reduce_blocks (counts and by_genome over the blocks), k_amap_reduce_contigs (the contig classes),
//        k_amap_contig_cols (first_block and worst_join as the header states them).
// Bounds.  Occurrences are stored below a capacity the host derived from the bytes of the truth adds, truth rows below the one it
// derived from their lines; hits below the total of the scan (at most a base each), for which the host made room after it had read
// it; runs, kept runs and blocks below the totals of their scans likewise; contig columns below c0 + the add's records.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#define ASM_ROUTINES_ONLY
#include "asmeval_kernels.hip"  // asm_roll_at, asm_find, AsmPlane, AsmEntries; through it mapeval's and the reader's routines

namespace simmr {

#define AMAP_WG 256u
#define AMAP_LDS_ROWS 1024u  /* rows of the per-genome table that are combined in LDS */
#define AMAP_JOIN_NONE 0u    /* a contig's first block; the classes are the header's SIMMR_ASMMAP_INTER_GENOME (1) .. SIMMR_ASMMAP_LOCAL (5) */
/* a contig's worst join is kept as AMAP_WORST_BASE - class, so that the smallest class is an atomicMax over a zeroed column; 0: none */
#define AMAP_WORST_BASE (SIMMR_ASMMAP_LOCAL + 1u)
static_assert(SIMMR_ASMMAP_INTER_GENOME == 1u && SIMMR_ASMMAP_INTER_RECORD == 2u && SIMMR_ASMMAP_INVERSION == 3u && SIMMR_ASMMAP_RELOCATION == 4u &&
              SIMMR_ASMMAP_LOCAL == 5u, "the five break counts follow each other in the header's order of the classes");

enum { AM_T_RECORDS = 0, AM_T_BASES, AM_T_INVALID, AM_T_KMERS, AM_T_ANCHORS, AM_T_REPEATS, AM_RECORDS, AM_BASES, AM_INVALID, AM_KMERS, AM_HITS,
       AM_STRAY_HITS, AM_REPEAT_HITS, AM_RUNS, AM_RUNS_DROPPED, AM_BLOCKS, AM_BLOCK_BASES, AM_BR_INTER_GENOME, AM_BR_INTER_RECORD, AM_BR_INVERSION,
       AM_BR_RELOCATION, AM_BR_LOCAL, AM_C_UNPLACED, AM_C_CLEAN, AM_C_LOCAL_ONLY, AM_C_MISASSEMBLED, AM_MIS_BASES, AM_COUNT };
static_assert(sizeof(simmr_asmmap_counts) == AM_COUNT * 8u, "the counts in the header's order");
#define AMAP_GENOME_COLS 5u  /* truth_bases, truth_anchors, blocks, block_bases, longest_block */
static_assert(SIMMR_ASMMAP_GENOME_COLS == AMAP_GENOME_COLS, "the header's table");

struct AmapAnchors {  // the anchor index behind its table, and the distinct repeat keys behind theirs
  AsmEntries A, R;
  const uint32_t* t;
  const uint32_t* p;
  const uint32_t* o;
};

struct AmapHits {  // the anchor hits of one add in (contig, q) order
  uint32_t* c;   // the contig's ordinal in the add
  uint32_t* q;
  uint32_t* ts;  // t << 1 | s
  long long* d;
};

struct AmapBlocks {  // the block columns since the plan
  uint32_t *contig, *truth, *strand, *q_start, *q_end, *p_start, *p_end, *hits, *join;
  long long *d_first, *d_last;
};

struct AmapContigs {  // the contig columns since the plan
  uint64_t* length;
  uint32_t* hits;
  uint32_t* blocks;
  uint32_t* first;   // the first block's row + 1; 0: none
  unsigned long long* block_bases;
  uint32_t* worst;   // AMAP_WORST_BASE - the smallest join class; 0: none
};

SIMMR_DEV uint64_t amap_dist(long long a, long long b) { return a < b ? (uint64_t)(b - a) : (uint64_t)(a - b); }

// the sum of v over the wave, in every lane
SIMMR_DEV uint32_t amap_wave_sum(uint32_t v) {
  for (uint32_t d = 32u; d > 0u; d >>= 1) v += (uint32_t)__shfl_xor((int)v, (int)d, 64);
  return v;
}

// ---- the truth --------------------------------------------------------------------------------------------------------------------
// counts[AM_T_RECORDS] holds the add's records already (the front's chunks kernel ran before)
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_truth_records(const uint32_t* __restrict__ rec_start, const uint32_t* __restrict__ tot, const uint32_t* __restrict__ rec_row,
                     const unsigned long long* __restrict__ counts, uint64_t capacity, uint32_t* __restrict__ t_genome, uint32_t* __restrict__ t_len) {
  const uint32_t n_rec = tot[2];
  const uint64_t t0 = counts[AM_T_RECORDS] - n_rec;
  for (uint32_t r = blockIdx.x * AMAP_WG + threadIdx.x; r < n_rec; r += gridDim.x * AMAP_WG) {
    const uint64_t t = t0 + r;
    if (t >= capacity) continue;
    t_genome[t] = rec_row[r];
    t_len[t] = rec_start[r + 1u] - rec_start[r];
  }
}

extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_roll_truth(AsmPlane P, uint32_t k, const unsigned long long* __restrict__ counts, uint64_t* __restrict__ occ_key, uint32_t* __restrict__ occ_to,
                  uint32_t* __restrict__ occ_p, uint64_t capacity, unsigned long long* __restrict__ cursor) {
  const uint32_t n_bases = P.tot[1], n_rec = P.tot[2];
  const uint32_t n_words = n_bases / ASM_WORD + (n_bases % ASM_WORD ? 1u : 0u);
  const uint64_t t0 = counts[AM_T_RECORDS] - n_rec;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t w0 = (uint64_t)blockIdx.x * AMAP_WG + (threadIdx.x & ~63u); w0 < n_words; w0 += (uint64_t)gridDim.x * AMAP_WG) {  // (uniform over the wave)
    const uint64_t w = w0 + lane;
    uint32_t cnt = 0;
    if (w < n_words) asm_roll_at(P, (uint32_t)w, n_bases, n_rec, k, [&](uint32_t, uint64_t, uint32_t, uint32_t) { cnt++; });
    uint32_t inc = cnt;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
      if (lane >= d) inc += o;
    }
    const uint32_t total = (uint32_t)__shfl((int)inc, 63, 64);
    unsigned long long base = 0;
    if (lane == 0u && total) base = atomicAdd(cursor, (unsigned long long)total);
    base = __shfl(base, 0, 64);
    uint64_t at = base + inc - cnt;
    if (w < n_words && cnt)
      asm_roll_at(P, (uint32_t)w, n_bases, n_rec, k, [&](uint32_t rec, uint64_t key, uint32_t last, uint32_t o) {
        if (at < capacity) {
          occ_key[at] = key;
          occ_to[at] = (uint32_t)(t0 + rec) << 1 | o;
          occ_p[at] = last + 1u - k - P.rec_start[rec];
        }
        at++;
      });
  }
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_marks(const uint64_t* __restrict__ skey, uint64_t n, uint32_t* __restrict__ anchor, uint32_t* __restrict__ repeat) {
  for (uint64_t j = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; j < n; j += (uint64_t)gridDim.x * AMAP_WG) {
    const uint64_t key = skey[j];
    const bool head = j == 0u || skey[j - 1u] != key, last = j + 1u == n || skey[j + 1u] != key;
    anchor[j] = head && last ? 1u : 0u;
    repeat[j] = head && !last ? 1u : 0u;
  }
}

extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_index(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ anchor, const uint32_t* __restrict__ repeat,
             const uint64_t* __restrict__ a_before, const uint64_t* __restrict__ r_before, const uint32_t* __restrict__ occ_to, const uint32_t* __restrict__ occ_p,
             uint64_t n, uint64_t n_anchors, uint64_t n_repeats, uint64_t* __restrict__ a_key, uint32_t* __restrict__ a_t, uint32_t* __restrict__ a_p,
             uint32_t* __restrict__ a_o, uint64_t* __restrict__ r_key) {
  for (uint64_t j = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; j < n; j += (uint64_t)gridDim.x * AMAP_WG) {
    if (anchor[j]) {
      const uint64_t a = a_before[j];
      if (a >= n_anchors) continue;
      const uint32_t i = idx[j], to = occ_to[i];
      a_key[a] = skey[j];
      a_t[a] = to >> 1;
      a_o[a] = to & 1u;
      a_p[a] = occ_p[i];
    } else if (repeat[j]) {
      const uint64_t r = r_before[j];
      if (r < n_repeats) r_key[r] = skey[j];
    }
  }
}

// THE PREFIX TABLE (the rule of k_asm_table: bits = min(24, bit length of the number of entries)): table[b] = the first entry whose
// key >> shift is not below b, for b = 0 .. 2^bits
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_table(const uint64_t* __restrict__ e_key, uint32_t n_entries, uint32_t bits, uint32_t shift, uint32_t* __restrict__ table) {
  const uint64_t n_buckets = (1ull << bits) + 1ull;
  for (uint64_t b = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; b < n_buckets; b += (uint64_t)gridDim.x * AMAP_WG) {
    const uint64_t want = b << shift;
    uint32_t lo = 0, hi = n_entries;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if (e_key[mid] < want) lo = mid + 1u;
      else hi = mid;
    }
    table[b] = lo;
  }
}

// g_truth[row][2] = truth_bases, truth_anchors; rows below AMAP_LDS_ROWS through LDS.  One grid-stride loop over the truth records
// and one over the anchors.
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_reduce_truth(const uint32_t* __restrict__ t_genome, const uint32_t* __restrict__ t_len, uint64_t n_truth, const uint32_t* __restrict__ a_t,
                    uint64_t n_anchors, uint32_t n_genomes, unsigned long long* __restrict__ g_truth) {
  __shared__ unsigned long long l_g[AMAP_LDS_ROWS * 2u];
  for (uint32_t i = threadIdx.x; i < AMAP_LDS_ROWS * 2u; i += AMAP_WG) l_g[i] = 0ull;
  __syncthreads();
  for (uint64_t t = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; t < n_truth; t += (uint64_t)gridDim.x * AMAP_WG) {
    const uint32_t g = t_genome[t];
    if (g >= n_genomes) continue;
    if (g < AMAP_LDS_ROWS) atomicAdd(&l_g[g * 2u], (unsigned long long)t_len[t]);
    else atomicAdd(g_truth + (uint64_t)g * 2u, (unsigned long long)t_len[t]);
  }
  for (uint64_t a = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; a < n_anchors; a += (uint64_t)gridDim.x * AMAP_WG) {
    const uint32_t t = a_t[a];
    if (t >= n_truth) continue;
    const uint32_t g = t_genome[t];
    if (g >= n_genomes) continue;
    if (g < AMAP_LDS_ROWS) atomicAdd(&l_g[g * 2u + 1u], 1ull);
    else atomicAdd(g_truth + (uint64_t)g * 2u + 1u, 1ull);
  }
  __syncthreads();
  const uint32_t lds_rows = n_genomes < AMAP_LDS_ROWS ? n_genomes : AMAP_LDS_ROWS;
  for (uint32_t i = threadIdx.x; i < lds_rows * 2u; i += AMAP_WG)
    if (l_g[i]) atomicAdd(g_truth + i, l_g[i]);
}

// ---- the candidates: the roll in two passes -----------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_contig_len(const uint32_t* __restrict__ rec_start, uint32_t n_rec, uint64_t c0, uint64_t* __restrict__ length) {
  for (uint32_t r = blockIdx.x * AMAP_WG + threadIdx.x; r < n_rec; r += gridDim.x * AMAP_WG) length[c0 + r] = rec_start[r + 1u] - rec_start[r];
}

struct AmapLaneSums {  // what a lane holds of the word it is in: the contig of its last hit and that contig's hits, then the word's sums
  uint32_t rec, of_rec, kmers, hits, repeats;
};

extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_roll_count(AsmPlane P, uint32_t k, AmapAnchors X, uint64_t c0, uint32_t* __restrict__ c_hits, uint32_t* __restrict__ lane_hits,
                  unsigned long long* __restrict__ counts) {
  const uint32_t n_bases = P.tot[1], n_rec = P.tot[2];
  const uint32_t n_words = n_bases / ASM_WORD + (n_bases % ASM_WORD ? 1u : 0u);
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t kmers = 0, hits = 0, repeats = 0;
  for (uint64_t w0 = (uint64_t)blockIdx.x * AMAP_WG + (threadIdx.x & ~63u); w0 < n_words; w0 += (uint64_t)gridDim.x * AMAP_WG) {  // (uniform over the wave)
    const uint64_t w = w0 + lane;
    if (w >= n_words) continue;
    AmapLaneSums S{ASM_NONE, 0u, 0u, 0u, 0u};
    asm_roll_at(P, (uint32_t)w, n_bases, n_rec, k, [&](uint32_t rec, uint64_t key, uint32_t, uint32_t) {
      S.kmers++;
      if (asm_find(X.A, key) != ASM_NONE) {
        if (rec != S.rec) {
          if (S.of_rec) atomicAdd(c_hits + c0 + S.rec, S.of_rec);
          S.rec = rec;
          S.of_rec = 0u;
        }
        S.hits++;
        S.of_rec++;
      } else if (X.R.n && asm_find(X.R, key) != ASM_NONE) {
        S.repeats++;
      }
    });
    if (S.of_rec) atomicAdd(c_hits + c0 + S.rec, S.of_rec);
    lane_hits[w] = S.hits;
    kmers += S.kmers;
    hits += S.hits;
    repeats += S.repeats;
  }
  kmers = amap_wave_sum(kmers);
  hits = amap_wave_sum(hits);
  repeats = amap_wave_sum(repeats);
  if (lane == 0u) {
    if (kmers) atomicAdd(counts + AM_KMERS, (unsigned long long)kmers);
    if (hits) atomicAdd(counts + AM_HITS, (unsigned long long)hits);
    if (repeats) atomicAdd(counts + AM_REPEAT_HITS, (unsigned long long)repeats);
  }
}

// lane_off[w] = the hits in front of word w; n_hits = lane_off[n_words]
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_roll_write(AsmPlane P, uint32_t k, AmapAnchors X, const uint32_t* __restrict__ lane_hits, const uint64_t* __restrict__ lane_off, uint64_t n_hits, AmapHits H) {
  const uint32_t n_bases = P.tot[1], n_rec = P.tot[2];
  const uint32_t n_words = n_bases / ASM_WORD + (n_bases % ASM_WORD ? 1u : 0u);
  for (uint64_t w = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * AMAP_WG) {
    if (lane_hits[w] == 0u) continue;
    uint64_t at = lane_off[w];
    asm_roll_at(P, (uint32_t)w, n_bases, n_rec, k, [&](uint32_t rec, uint64_t key, uint32_t last, uint32_t oc) {
      const uint32_t a = asm_find(X.A, key);
      if (a == ASM_NONE) return;
      if (at < n_hits) {
        const uint32_t q = last + 1u - k - P.rec_start[rec], s = oc ^ X.o[a];
        const long long p = (long long)X.p[a];
        H.c[at] = rec;
        H.q[at] = q;
        H.ts[at] = X.t[a] << 1 | s;
        H.d[at] = s ? p + (long long)q : p - (long long)q;
      }
      at++;
    });
  }
}

// ---- runs ---------------------------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_run_heads(AmapHits H, uint64_t n_hits, uint64_t band, uint32_t* __restrict__ head) {
  for (uint64_t i = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; i < n_hits; i += (uint64_t)gridDim.x * AMAP_WG)
    head[i] = i == 0u || H.c[i] != H.c[i - 1u] || H.ts[i] != H.ts[i - 1u] || amap_dist(H.d[i], H.d[i - 1u]) > band ? 1u : 0u;
}

// before[i] = the heads in front of hit i: the run of hit i is before[i] + head[i] - 1
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_runs(const uint32_t* __restrict__ head, const uint64_t* __restrict__ before, uint64_t n_hits, uint64_t n_runs, uint32_t* __restrict__ r_first,
            uint32_t* __restrict__ r_last) {
  for (uint64_t i = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; i < n_hits; i += (uint64_t)gridDim.x * AMAP_WG) {
    const uint64_t r = before[i] + head[i] - 1u;
    if (r >= n_runs) continue;
    if (head[i]) r_first[r] = (uint32_t)i;
    if (i + 1u == n_hits || head[i + 1u]) r_last[r] = (uint32_t)i;
  }
}

extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_kept(const uint32_t* __restrict__ r_first, const uint32_t* __restrict__ r_last, uint64_t n_runs, uint32_t min_anchors, uint32_t* __restrict__ kept,
            unsigned long long* __restrict__ counts) {
  uint32_t dropped = 0, stray = 0;
  for (uint64_t r0 = (uint64_t)blockIdx.x * AMAP_WG + (threadIdx.x & ~63u); r0 < n_runs; r0 += (uint64_t)gridDim.x * AMAP_WG) {  // (uniform over the wave)
    const uint64_t r = r0 + (threadIdx.x & 63u);
    if (r >= n_runs) continue;
    const uint32_t n = r_last[r] - r_first[r] + 1u;
    kept[r] = n >= min_anchors ? 1u : 0u;
    if (n < min_anchors) {
      dropped++;
      stray += n;
    }
  }
  // (a wave's stray hits are below 2^32: a hit a base, an add below 2^31 bytes)
  dropped = amap_wave_sum(dropped);
  stray = amap_wave_sum(stray);
  if ((threadIdx.x & 63u) == 0u && dropped) {
    atomicAdd(counts + AM_RUNS_DROPPED, (unsigned long long)dropped);
    atomicAdd(counts + AM_STRAY_HITS, (unsigned long long)stray);
  }
}

extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_kept_runs(const uint32_t* __restrict__ kept, const uint64_t* __restrict__ before, const uint32_t* __restrict__ r_first, const uint32_t* __restrict__ r_last,
                 uint64_t n_runs, uint64_t n_kept, uint32_t* __restrict__ k_first, uint32_t* __restrict__ k_last) {
  for (uint64_t r = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; r < n_runs; r += (uint64_t)gridDim.x * AMAP_WG) {
    if (!kept[r]) continue;
    const uint64_t j = before[r];
    if (j >= n_kept) continue;
    k_first[j] = r_first[r];
    k_last[j] = r_last[r];
  }
}

// ---- blocks -------------------------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_block_heads(AmapHits H, const uint32_t* __restrict__ k_first, const uint32_t* __restrict__ k_last, uint64_t n_kept, uint64_t band,
                   uint32_t* __restrict__ head) {
  for (uint64_t j = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; j < n_kept; j += (uint64_t)gridDim.x * AMAP_WG) {
    bool h = j == 0u;
    if (!h) {
      const uint32_t a = k_last[j - 1u], b = k_first[j];
      h = H.c[a] != H.c[b] || H.ts[a] != H.ts[b] || amap_dist(H.d[a], H.d[b]) > band;
    }
    head[j] = h ? 1u : 0u;
  }
}

// before[j] = the heads in front of kept run j; b0 = the blocks of the earlier adds.  hits is zeroed, p_start all ones and p_end
// zero before.
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_blocks(AmapHits H, const uint32_t* __restrict__ k_first, const uint32_t* __restrict__ k_last, const uint32_t* __restrict__ head,
              const uint64_t* __restrict__ before, uint64_t n_kept, uint64_t n_blocks, uint64_t b0, uint64_t c0, uint32_t k, AmapBlocks B) {
  for (uint64_t j = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; j < n_kept; j += (uint64_t)gridDim.x * AMAP_WG) {
    const uint64_t bl = before[j] + head[j] - 1u;
    if (bl >= n_blocks) continue;
    const uint64_t b = b0 + bl;
    const uint32_t first = k_first[j], last = k_last[j];
    if (head[j]) {
      const uint32_t ts = H.ts[first];
      B.contig[b] = (uint32_t)(c0 + H.c[first]);
      B.truth[b] = ts >> 1;
      B.strand[b] = ts & 1u;
      B.q_start[b] = H.q[first];
      B.d_first[b] = H.d[first];
    }
    if (j + 1u == n_kept || head[j + 1u]) {
      B.q_end[b] = H.q[last] + k;
      B.d_last[b] = H.d[last];
    }
    atomicAdd(B.hits + b, last - first + 1u);
  }
}

// a hit a thread: its run, whether that is kept, its block; p by the hit's d, q and strand
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_block_span(AmapHits H, const uint32_t* __restrict__ run_head, const uint64_t* __restrict__ run_before, const uint32_t* __restrict__ kept,
                  const uint64_t* __restrict__ kept_before, const uint32_t* __restrict__ blk_head, const uint64_t* __restrict__ blk_before, uint64_t n_hits,
                  uint64_t n_blocks, uint64_t b0, uint32_t k, AmapBlocks B) {
  for (uint64_t i0 = (uint64_t)blockIdx.x * AMAP_WG + (threadIdx.x & ~63u); i0 < n_hits; i0 += (uint64_t)gridDim.x * AMAP_WG) {  // (uniform over the wave)
    const uint64_t i = i0 + (threadIdx.x & 63u);
    unsigned long long bl = ~0ull;
    uint32_t lo = 0xffffffffu, hi = 0u;
    if (i < n_hits) {
      const uint64_t r = run_before[i] + run_head[i] - 1u;
      if (kept[r]) {
        const uint64_t j = kept_before[r];
        bl = blk_before[j] + blk_head[j] - 1u;
        if (bl >= n_blocks) bl = ~0ull;
        const long long d = H.d[i], q = (long long)H.q[i];
        lo = hi = (uint32_t)((H.ts[i] & 1u) ? d - q : d + q);
      }
    }
    const unsigned long long of_first = __shfl(bl, 0, 64);
    if (__all(bl == of_first)) {  // one block (or none) in the whole wave: one pair of atomics
      for (uint32_t d = 32u; d > 0u; d >>= 1) {
        const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, (int)d, 64), h2 = (uint32_t)__shfl_xor((int)hi, (int)d, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
      }
      if ((threadIdx.x & 63u) != 0u) bl = ~0ull;
    }
    if (bl != ~0ull) {
      atomicMin(B.p_start + b0 + bl, lo);
      atomicMax(B.p_end + b0 + bl, hi + k);
    }
  }
}

// the class of the step into every block of the add, and the contig's columns
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_joins(AmapBlocks B, uint64_t b0, uint64_t n_blocks, const uint32_t* __restrict__ t_genome, uint64_t band, uint64_t relocation, AmapContigs C) {
  for (uint64_t bl = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; bl < n_blocks; bl += (uint64_t)gridDim.x * AMAP_WG) {
    const uint64_t b = b0 + bl;
    const uint32_t c = B.contig[b];
    uint32_t join = AMAP_JOIN_NONE;
    if (bl > 0u && B.contig[b - 1u] == c) {
      const uint32_t t = B.truth[b], tp = B.truth[b - 1u];
      if (t_genome[t] != t_genome[tp]) join = SIMMR_ASMMAP_INTER_GENOME;
      else if (t != tp) join = SIMMR_ASMMAP_INTER_RECORD;
      else if (B.strand[b] != B.strand[b - 1u]) join = SIMMR_ASMMAP_INVERSION;
      else join = amap_dist(B.d_first[b], B.d_last[b - 1u]) > relocation ? SIMMR_ASMMAP_RELOCATION : SIMMR_ASMMAP_LOCAL;
    }
    B.join[b] = join;
    atomicAdd(C.blocks + c, 1u);
    atomicAdd(C.block_bases + c, (unsigned long long)(B.q_end[b] - B.q_start[b]));
    if (join == AMAP_JOIN_NONE) C.first[c] = (uint32_t)b + 1u;
    else atomicMax(C.worst + c, AMAP_WORST_BASE - join);
  }
}

// ---- simmr_asmmap_read --------------------------------------------------------------------------------------------------------------
// g_blocks[row][3] = blocks, block_bases, longest_block.  The blocks are few (a block has min_anchors hits or more): HBM atomics.
extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_reduce_blocks(AmapBlocks B, uint64_t n_blocks, const uint32_t* __restrict__ t_genome, uint32_t n_genomes, unsigned long long* __restrict__ g_blocks,
                     unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long l_c[7];  // blocks, block_bases, then the five classes
  if (threadIdx.x < 7u) l_c[threadIdx.x] = 0ull;
  __syncthreads();
  for (uint64_t b = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; b < n_blocks; b += (uint64_t)gridDim.x * AMAP_WG) {
    const unsigned long long len = B.q_end[b] - B.q_start[b];
    const uint32_t join = B.join[b], g = t_genome[B.truth[b]];
    atomicAdd(&l_c[0], 1ull);
    atomicAdd(&l_c[1], len);
    if (join != AMAP_JOIN_NONE && join <= SIMMR_ASMMAP_LOCAL) atomicAdd(&l_c[1u + join], 1ull);
    if (g < n_genomes) {
      atomicAdd(g_blocks + (uint64_t)g * 3u, 1ull);
      atomicAdd(g_blocks + (uint64_t)g * 3u + 1u, len);
      atomicMax(g_blocks + (uint64_t)g * 3u + 2u, len);
    }
  }
  __syncthreads();
  if (threadIdx.x < 7u && l_c[threadIdx.x]) atomicAdd(counts + AM_BLOCKS + threadIdx.x, l_c[threadIdx.x]);
}

extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_reduce_contigs(AmapContigs C, uint64_t n_contigs, unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long l_c[5];  // unplaced, clean, local only, misassembled, misassembled bases
  if (threadIdx.x < 5u) l_c[threadIdx.x] = 0ull;
  __syncthreads();
  for (uint64_t c = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; c < n_contigs; c += (uint64_t)gridDim.x * AMAP_WG) {
    const uint32_t blocks = C.blocks[c], worst = C.worst[c];
    const uint32_t cls = blocks == 0u ? 0u : blocks == 1u ? 1u : worst == AMAP_WORST_BASE - SIMMR_ASMMAP_LOCAL ? 2u : 3u;
    atomicAdd(&l_c[cls], 1ull);
    if (cls == 3u) atomicAdd(&l_c[4], (unsigned long long)C.length[c]);
  }
  __syncthreads();
  if (threadIdx.x < 5u && l_c[threadIdx.x]) atomicAdd(counts + AM_C_UNPLACED + threadIdx.x, l_c[threadIdx.x]);
}

extern "C" __global__ void __launch_bounds__(AMAP_WG)
k_amap_contig_cols(const uint32_t* __restrict__ first, const uint32_t* __restrict__ worst, uint64_t n_contigs, uint32_t* __restrict__ first_block,
                   uint32_t* __restrict__ worst_join) {
  for (uint64_t c = (uint64_t)blockIdx.x * AMAP_WG + threadIdx.x; c < n_contigs; c += (uint64_t)gridDim.x * AMAP_WG) {
    if (first_block) first_block[c] = first[c] ? first[c] - 1u : ASM_NONE;
    if (worst_join) worst_join[c] = worst[c] ? AMAP_WORST_BASE - worst[c] : 0u;
  }
}

}  // namespace simmr
