// fit_kernels.hip — the counting and the density estimation behind a simmrd-format error model (gfx950): k-mer to
// alternate-k-mer counts, a quality histogram per read offset, read-length and insert-size histograms, and the Gaussian
// kernel densities over them (include/simmr_hip.h states every table and rule).  Included by fit.hip alone, a translation
// unit of its own: nothing here is seen by the other units, whose kernel budgets stay what they were, and of kernels.hip
// and truth_kernels.hip it sees the plain routines of read_walk.hpp only.
//
// Seven kernels.
//   k_fit_add      one pass over the columns with the read walker (walk_open / walk_window, shared with k_truth and
//                  k_read_stats): FIT_LANES = 16 lanes (one DPP row) share a read, a lane takes 16 bases per round.  A lane
//                  turns its 16 expected and 16 written bytes into 3-bit classes packed into two 64-bit registers; the
//                  windows that END in its group need the k - 1 bytes before it, which are its left neighbour's packs
//                  (a row shuffle; lane 0 takes lane 15's of the round before).  From there the lane ROLLS: per byte one
//                  shift of the 2-bit and the 3-bit reference code, of the 3-bit written code and of three k-bit masks
//                  (reference byte not ACGT, written byte N or '-', written byte outside ACGTN-), so no window re-reads k
//                  bytes.  A window whose written k-mer holds an N is compacted from the register (rare).
//                  Unchanged windows and the reference's own count go to a dense table indexed by the 2-bit code:
//                  dense[ref] += 1 + (written == ref).  For k <= FIT_LDS_K = 7 the table (4^k <= 16 384 words) is
//                  privatised in LDS; above that it is 2^16 .. 2^20 entries in HBM, where same-address traffic is thin, and
//                  takes 64-bit atomics directly.  Changed windows go to an open-addressing table in HBM: key =
//                  ref << 32 | alt, claimed with a 64-bit compare-and-swap, counted with an atomic add, linear probing
//                  bounded by FIT_MAX_PROBE — a full table sets the sticky FIT_ERR_FULL and never spins.
//                  Quality, length and insert histograms are per-workgroup partial counts in LDS for the entries a
//                  short-read run hammers (offsets below FIT_LDS_POS, lengths and inserts below FIT_LDS_LEN) and 64-bit
//                  atomics in HBM beyond (long reads spread over thousands of offsets).  The workgroup adds its LDS
//                  tables to HBM, zero entries skipped, at the end and after every FIT_FLUSH_BATCHES batches.
//   k_fit_compact  the live entries of the dense table and of the pair table as (key, count) records, places from one atomic
//                  counter: the order is arbitrary and the sort behind it removes it (keys are unique, so the sorted list is a
//                  function of the inputs alone).  Launched twice: to count, then to write into a list of that size.
//   k_fit_sort_key, k_fit_segments, k_fit_ref_scan, k_fit_pairs   the finish: three stable runs of the shared radix sort
//                  (alt, ~count, ref: 30 + 64 + 30 key bits against its 64), per reference k-mer the run's start, length and
//                  total by atomics on integer tables indexed by the 2-bit code, one workgroup's scan for the offsets, and the
//                  kept pairs with their f32 probabilities.
//   k_fit_density  one workgroup per (column, chunk of points): n, mean, population standard deviation and the bandwidth
//                  1.06 sd n^(-1/5) from the column's histogram, then sum_v count[v] exp(-((x - v) / bw)^2 / 2) /
//                  (sqrt(2 pi) n bw) per point x, all in f64, summed over histogram entries in a fixed tree (the result does
//                  not depend on the grid).  bw == 0 is the point mass.
//
// LDS of k_fit_add, 135 168 bytes per workgroup: one workgroup of 512 threads per CU, two waves per SIMD (at 1024 threads the
// compiler's 128 registers a lane spill to scratch; the privatised tables are worth more than the waves).
//   words 0 .. 16383       dense[code]                       (k <= 7; unused above)
//   words 16384 .. 31743   quality[offset < 160][q < 96]     (q <= 93 is checked before the add)
//   words 31744 .. 32767   lengths below 1024
//   words 32768 .. 33791   inserts below 1024
// What bounds a 32-bit partial: a workgroup flushes after FIT_FLUSH_BATCHES = 512 batches of 32 reads; a read longer than
// FIT_MAX_L = 65 535 is refused by the bounds check and a window adds at most 2 to one dense word, so a word gains at most
// 2 * 65 535 * 32 * 512 = 2 147 450 880 < 2^32 between flushes; the other tables gain at most 1 per read and entry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#include "fit_device.hpp"  // the tables, the class codes and the pair insert: shared with fit_sam_kernels.hip
#include "read_walk.hpp"

namespace simmr {

extern "C" __global__ void __launch_bounds__(FIT_WG)
k_fit_add(const GenomeDev* __restrict__ genomes, uint32_t n_genomes, TruthReads rd, uint64_t n_reads, uint32_t n_sets,
          uint32_t qual_offset, FitTables T) {
  __shared__ uint32_t lds[FIT_LDS_WORDS];
  uint32_t* const l_dense = lds;
  uint32_t* const l_q = lds + FIT_DENSE_LDS;
  uint32_t* const l_len = l_q + FIT_LDS_POS * FIT_Q_STRIDE;
  uint32_t* const l_ins = l_len + FIT_LDS_LEN;
  const uint32_t tid = threadIdx.x, sub = tid & (FIT_LANES - 1u), row = tid / FIT_LANES;
  const uint32_t k = T.k, kmask = (1u << k) - 1u, top2 = 2u * (k - 1u), top3 = 3u * (k - 1u);
  const bool dense_lds = k <= FIT_LDS_K;
  const uint32_t n_dense_lds = dense_lds ? 1u << (2u * k) : 0u;
  for (uint32_t i = tid; i < FIT_LDS_WORDS; i += FIT_WG) lds[i] = 0u;
  __syncthreads();

  const uint64_t n_batches = (n_reads + FIT_WG_READS - 1u) / FIT_WG_READS;
  uint32_t since_flush = 0;
  for (uint64_t batch = blockIdx.x;; batch += gridDim.x) {  // (uniform over the workgroup)
    const bool more = batch < n_batches;
    if (!more || since_flush == FIT_FLUSH_BATCHES) {
      // add the workgroup's tables to HBM, zero entries skipped, and zero them
      __syncthreads();
      for (uint32_t i = tid; i < n_dense_lds; i += FIT_WG) {
        const uint32_t v = l_dense[i];
        if (v) { atomicAdd(T.dense + i, (unsigned long long)v); l_dense[i] = 0u; }
      }
      for (uint32_t i = tid; i < FIT_LDS_POS * FIT_Q_STRIDE; i += FIT_WG) {
        const uint32_t v = l_q[i];
        if (v) { atomicAdd(T.qhist + (uint64_t)(i / FIT_Q_STRIDE) * SIMMR_FIT_QUALS + i % FIT_Q_STRIDE, (unsigned long long)v); l_q[i] = 0u; }
      }
      for (uint32_t i = tid; i < FIT_LDS_LEN; i += FIT_WG) {
        const uint32_t v = l_len[i], u = l_ins[i];
        if (v) { atomicAdd(T.lhist + i, (unsigned long long)v); l_len[i] = 0u; }
        if (u) { atomicAdd(T.ihist + i, (unsigned long long)u); l_ins[i] = 0u; }
      }
      __syncthreads();
      since_flush = 0;
      if (!more) break;
    }
    since_flush++;

    const uint64_t r = batch * FIT_WG_READS + row;
    const ReadWalk w = walk_open<FIT_MAX_L>(genomes, n_genomes, rd, r, n_reads, T.err, FIT_ERR_READ, sub == 0);
    const uint32_t L = w.L;
    const uint8_t* seq = rd.seq + w.so;
    const uint8_t* qual = rd.qual + (rd.slot16 ? (w.so & ~15ull) : w.so);
    const uint32_t n_groups = (L + 15u) >> 4;
    uint64_t carry_w = 0, carry_h = 0;  // lane 15's packs of the round before
    uint32_t bad_q = 0;
    for (uint32_t g0 = 0; g0 < n_groups; g0 += FIT_LANES) {  // (uniform over the row: every lane of it takes the shuffles)
      const uint32_t grp = g0 + sub;
      const bool mine = grp < n_groups;
      // the classes of bases 16 grp .. 16 grp + 15, three bits each, base 16 grp lowest
      uint64_t pw = 0, ph = 0;
      if (mine) {
        const ReadWindow x = walk_window<true>(w, grp, seq, qual);
        const v4u32 have = x.have, qv = x.qv, want = x.want;
#pragma unroll
        for (uint32_t b = 0; b < 16u; b++) {
          pw |= (uint64_t)fit_class(FIT_BYTE(want, b), 4u, 4u) << (3u * b);
          ph |= (uint64_t)fit_class(FIT_BYTE(have, b), 4u, 5u) << (3u * b);
          if (!((x.keep >> b) & 1u)) continue;
          const uint32_t q = (FIT_BYTE(qv, b) - qual_offset) & 255u, j = x.k + b;
          if (q > SIMMR_FIT_MAX_Q) bad_q = 1u;
          else if (j < FIT_LDS_POS) atomicAdd(&l_q[j * FIT_Q_STRIDE + q], 1u);
          else atomicAdd(T.qhist + (uint64_t)j * SIMMR_FIT_QUALS + q, 1ull);
        }
        const uint32_t sh = 3u * (grp * 16u - x.k);  // the last window starts before its group: drop the neighbour's bases
        pw >>= sh;
        ph >>= sh;
      }
      uint64_t left_w = __shfl_up((unsigned long long)pw, 1u, (int)FIT_LANES), left_h = __shfl_up((unsigned long long)ph, 1u, (int)FIT_LANES);
      if (sub == 0u) { left_w = carry_w; left_h = carry_h; }
      carry_w = __shfl((unsigned long long)pw, (int)FIT_LANES - 1, (int)FIT_LANES);
      carry_h = __shfl((unsigned long long)ph, (int)FIT_LANES - 1, (int)FIT_LANES);
      if (!mine) continue;
      // roll: ref2 / ref3 / alt3 hold the last k bases, the masks one bit per base of them (all ones: not k bases yet)
      uint32_t ref2 = 0, ref3 = 0, alt3 = 0, ref_bad = kmask, alt_gap = 0, alt_bad = 0;
      const uint32_t e0 = grp * 16u, n_own = L - e0 < 16u ? L - e0 : 16u;
      for (uint32_t i = grp ? 17u - k : 16u; i < 16u + n_own; i++) {  // the k - 1 bases before the group, then its own
        const uint64_t sw = i < 16u ? left_w : pw, sh = i < 16u ? left_h : ph;
        const uint32_t at = 3u * (i & 15u), wc = (uint32_t)(sw >> at) & 7u, hc = (uint32_t)(sh >> at) & 7u;
        ref2 = (ref2 >> 2) | ((wc & 3u) << top2);
        ref3 = (ref3 >> 3) | (wc << top3);
        alt3 = (alt3 >> 3) | ((hc > 4u ? 4u : hc) << top3);
        ref_bad = ((ref_bad << 1) | (wc > 3u ? 1u : 0u)) & kmask;
        alt_gap = ((alt_gap << 1) | (hc == 4u ? 1u : 0u)) & kmask;
        alt_bad = ((alt_bad << 1) | (hc == 5u ? 1u : 0u)) & kmask;
        // the window that ends at base e = e0 + i - 16 starts at ndx = e + 1 - k; it counts when ndx + k < L
        if (i < 16u || e0 + (i - 16u) + 1u >= L || ref_bad || alt_bad) continue;
        uint32_t alt = alt3;
        if (alt_gap) {  // N and '-' leave the written k-mer, N fills it up again; nothing left: no window
          uint32_t m = 0;
          alt = 0;
          for (uint32_t f = 0; f < k; f++) {
            const uint32_t c = (alt3 >> (3u * f)) & 7u;
            if (c < 4u) alt |= c << (3u * m++);
          }
          if (m == 0u) continue;
          for (; m < k; m++) alt |= 4u << (3u * m);
        }
        const uint32_t same = alt == ref3 ? 1u : 0u;
        if (dense_lds) atomicAdd(&l_dense[ref2], 1u + same);
        else atomicAdd(T.dense + ref2, (unsigned long long)(1u + same));
        if (!same) fit_pair_add(T, (uint64_t)ref3 << 32 | alt);
      }
    }
    if (bad_q) atomicOr(T.err, FIT_ERR_QUAL);
    if (sub == 0u && w.good) {
      if (L < FIT_LDS_LEN) atomicAdd(&l_len[L], 1u);
      else atomicAdd(T.lhist + L, 1ull);
      if (n_sets == 2u) {  // |TLEN| of the pair as sam_kernels.hip has it: the span of the two mates (n_reads is even)
        const uint64_t a = rd.start[r], b = rd.end[r], ma = rd.start[r ^ 1ull], mb = rd.end[r ^ 1ull];
        const uint64_t lo = a < b ? a : b, hi = a < b ? b : a, mlo = ma < mb ? ma : mb, mhi = ma < mb ? mb : ma;
        const uint64_t span = (hi > mhi ? hi : mhi) - (lo < mlo ? lo : mlo);
        if (span < FIT_LDS_LEN) atomicAdd(&l_ins[(uint32_t)span], 1u);
        else if (span <= SIMMR_FIT_MAX_INSERT) atomicAdd(T.ihist + span, 1ull);
      }
    }
  }
}

// the 3-bit code of the ACGT k-mer with 2-bit code c
SIMMR_DEV uint32_t fit_code3(uint32_t c, uint32_t k) {
  uint32_t o = 0;
  for (uint32_t f = 0; f < k; f++) o |= ((c >> (2u * f)) & 3u) << (3u * f);
  return o;
}

// the 2-bit code of the ACGT k-mer with 3-bit code c
SIMMR_DEV uint32_t fit_code2(uint32_t c, uint32_t k) {
  uint32_t o = 0;
  for (uint32_t f = 0; f < k; f++) o |= ((c >> (3u * f)) & 3u) << (2u * f);
  return o;
}

// Two launches: with out_key == nullptr it only counts the live entries (the caller sizes the list from the count), with
// the columns it writes them; `room` entries are there, and a place is taken only inside them.
extern "C" __global__ void __launch_bounds__(256)
k_fit_compact(FitTables T, uint64_t n_dense, uint64_t n_slots, unsigned long long* __restrict__ out_key,
              unsigned long long* __restrict__ out_cnt, uint64_t room, unsigned long long* __restrict__ n_out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_dense + n_slots) return;
  unsigned long long key, cnt;
  if (i < n_dense) {
    cnt = T.dense[i];
    const uint32_t c3 = fit_code3((uint32_t)i, T.k);
    key = (unsigned long long)c3 << 32 | c3;
  } else {
    key = T.hkey[i - n_dense];
    cnt = key == FIT_EMPTY_KEY ? 0ull : T.hcnt[i - n_dense];
  }
  if (!cnt) return;
  const unsigned long long at = atomicAdd(n_out, 1ull);
  if (out_key && at < room) { out_key[at] = key; out_cnt[at] = cnt; }
}

// ---- the finish: order, totals, cut, probabilities --------------------------------------------------------------------
// The order (ref ascending, count descending, alt ascending) is 30 + 64 + 30 key bits; the shared radix sort takes 64-bit keys
// and is stable, so it runs three times, least significant key first: alt, then ~count, then ref.  Between two runs this kernel
// composes the permutation — perm_out[i] = the entry that stands at place i after the run before (idx: that run's answer over
// the order perm_prev; both null: the list's own order) — and writes that entry's key of the next run: which 0 alt, 1 ~count,
// 2 ref, 3 none (the last composition).
extern "C" __global__ void __launch_bounds__(256)
k_fit_sort_key(uint32_t which, const unsigned long long* __restrict__ in_key, const unsigned long long* __restrict__ in_cnt,
               const uint32_t* __restrict__ perm_prev, const uint32_t* __restrict__ idx, uint64_t n, uint32_t* __restrict__ perm_out,
               unsigned long long* __restrict__ key_out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t p = (uint32_t)i;
  if (idx) {
    p = idx[i];
    if (p >= n) return;  // (never: idx is the sort's permutation)
    if (perm_prev) p = perm_prev[p];
  }
  if (p >= n) return;
  perm_out[i] = p;
  if (which == 0u) key_out[i] = in_key[p] & 0xffffffffull;
  else if (which == 1u) key_out[i] = ~in_cnt[p];
  else if (which == 2u) key_out[i] = in_key[p] >> 32;
}

// per reference k-mer, by its 2-bit code: where its run starts in the sorted list, how many alternates it has, their total
struct FitRefs {
  uint32_t* start;            // [4^k], ~0 = absent
  uint32_t* n_alt;            // [4^k]
  unsigned long long* total;  // [4^k]
  unsigned long long* first;  // [4^k]: the reference k-mer's first kept pair (k_fit_ref_scan)
};

extern "C" __global__ void __launch_bounds__(256)
k_fit_segments(const unsigned long long* __restrict__ in_key, const unsigned long long* __restrict__ in_cnt, const uint32_t* __restrict__ perm,
               uint64_t n, uint32_t k, FitRefs R) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = perm[i];
  if (p >= n) return;
  const uint32_t r2 = fit_code2((uint32_t)(in_key[p] >> 32), k);
  atomicMin(R.start + r2, (uint32_t)i);
  atomicAdd(R.n_alt + r2, 1u);
  atomicAdd(R.total + r2, in_cnt[p]);
}

// ONE workgroup of 1024: the reference k-mers present, ascending (the 2-bit and the 3-bit code order alike), and the first kept
// pair of each: two exclusive scans over the 4^k entries, a thread taking a contiguous share.  sizes[0] = reference k-mers,
// sizes[1] = pairs kept; kmer_first gets its closing entry.
extern "C" __global__ void __launch_bounds__(1024)
k_fit_ref_scan(FitRefs R, uint32_t n_dense, uint32_t k, uint32_t max_alt, uint32_t* __restrict__ kmer_ref,
               unsigned long long* __restrict__ kmer_first, unsigned long long* __restrict__ sizes) {
  __shared__ unsigned long long s_ref[1024], s_pair[1024];
  const uint32_t t = threadIdx.x, share = (n_dense + 1023u) / 1024u;
  const uint32_t lo = t * share < n_dense ? t * share : n_dense, hi = lo + share < n_dense ? lo + share : n_dense;
  unsigned long long refs = 0, pairs = 0;
  for (uint32_t c = lo; c < hi; c++) {
    const uint32_t a = R.n_alt[c];
    refs += a ? 1u : 0u;
    pairs += a < max_alt ? a : max_alt;
  }
  s_ref[t] = refs;
  s_pair[t] = pairs;
  __syncthreads();
  for (uint32_t d = 1; d < 1024u; d <<= 1) {
    const unsigned long long a = t >= d ? s_ref[t - d] : 0ull, b = t >= d ? s_pair[t - d] : 0ull;
    __syncthreads();
    s_ref[t] += a;
    s_pair[t] += b;
    __syncthreads();
  }
  unsigned long long ri = s_ref[t] - refs, pi = s_pair[t] - pairs;
  for (uint32_t c = lo; c < hi; c++) {
    const uint32_t a = R.n_alt[c];
    if (!a) continue;
    kmer_ref[ri] = fit_code3(c, k);
    kmer_first[ri] = pi;
    R.first[c] = pi;
    ri++;
    pi += a < max_alt ? a : max_alt;
  }
  if (t == 1023u) {
    sizes[0] = s_ref[t];
    sizes[1] = s_pair[t];
    kmer_first[s_ref[t]] = s_pair[t];
  }
}

// the kept pairs: entry i of the sorted list is alternate i - start of its reference k-mer; the first max_alt stay, with
// (float)count / (float)total over ALL alternates (no renormalising after the cut)
extern "C" __global__ void __launch_bounds__(256)
k_fit_pairs(const unsigned long long* __restrict__ in_key, const unsigned long long* __restrict__ in_cnt, const uint32_t* __restrict__ perm,
            uint64_t n, uint32_t k, uint32_t max_alt, FitRefs R, uint32_t* __restrict__ pair_alt, unsigned long long* __restrict__ pair_count,
            float* __restrict__ pair_prob) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = perm[i];
  if (p >= n) return;
  const unsigned long long key = in_key[p], cnt = in_cnt[p];
  const uint32_t r2 = fit_code2((uint32_t)(key >> 32), k), start = R.start[r2];
  if (i < start || i - start >= max_alt) return;
  const unsigned long long o = R.first[r2] + (i - start);
  if (o >= n) return;  // (never: the kept pairs are a subset of the list)
  pair_alt[o] = (uint32_t)key;
  pair_count[o] = cnt;
  pair_prob[o] = (float)cnt / (float)R.total[r2];
}

// the sum of one value per thread over the workgroup, in every thread (a fixed tree: the same inputs give the same bits)
template <class V>
SIMMR_DEV V fit_wg_sum(V v, V* lds) {
  const uint32_t t = threadIdx.x;
  __syncthreads();
  lds[t] = v;
  __syncthreads();
  for (uint32_t d = FIT_DENSITY_WG / 2u; d > 0u; d >>= 1) {
    if (t < d) lds[t] += lds[t + d];
    __syncthreads();
  }
  return lds[0];
}

// Column c = blockIdx.x of hist (n_vals counts of the values 0 .. n_vals - 1, `stride` entries apart); blockIdx.y takes
// points pts[y * pts_per_wg ..) of the n_pts; out[c * n_pts + j] = the density at pts[j].  Point mass (bandwidth 0: every
// observation is the same value v): 1.0 where pts[j] == min(v, clamp), 0.0 elsewhere.  A column without observations
// writes zeros.
extern "C" __global__ void __launch_bounds__(FIT_DENSITY_WG)
k_fit_density(const unsigned long long* __restrict__ hist, uint64_t stride, uint32_t n_vals, const double* __restrict__ pts,
              uint32_t n_pts, uint32_t pts_per_wg, double clamp, double* __restrict__ out) {
  __shared__ double lds_d[FIT_DENSITY_WG];
  __shared__ unsigned long long lds_u[FIT_DENSITY_WG];
  const unsigned long long* const h = hist + (uint64_t)blockIdx.x * stride;
  double* const o = out + (uint64_t)blockIdx.x * n_pts;
  const uint32_t t = threadIdx.x;
  unsigned long long n = 0, s1 = 0;
  for (uint32_t v = t; v < n_vals; v += FIT_DENSITY_WG) { n += h[v]; s1 += h[v] * v; }
  n = fit_wg_sum<unsigned long long>(n, lds_u);
  s1 = fit_wg_sum<unsigned long long>(s1, lds_u);
  const double nd = (double)n, mean = n ? (double)s1 / nd : 0.0;
  double var = 0.0;
  for (uint32_t v = t; v < n_vals; v += FIT_DENSITY_WG)
    if (h[v]) var += (double)h[v] * (((double)v - mean) * ((double)v - mean));
  var = fit_wg_sum<double>(var, lds_d);
  const double sd = n ? sqrt(var / nd) : 0.0, bw = 1.06 * sd * pow(nd, -1.0 / 5.0);
  const double norm = sqrt(2.0 * 3.14159265358979323846) * nd * bw;
  const uint32_t j1 = (blockIdx.y + 1u) * pts_per_wg < n_pts ? (blockIdx.y + 1u) * pts_per_wg : n_pts;
  for (uint32_t j = blockIdx.y * pts_per_wg; j < j1; j++) {  // (uniform over the workgroup)
    const double x = pts[j];
    if (!n || !(bw > 0.0)) {
      if (t == 0) o[j] = (n && x == (mean < clamp ? mean : clamp)) ? 1.0 : 0.0;
      continue;
    }
    double s = 0.0;
    for (uint32_t v = t; v < n_vals; v += FIT_DENSITY_WG)
      if (h[v]) {
        const double f = (x - (double)v) / bw;
        s += (double)h[v] * exp(-0.5 * (f * f));
      }
    s = fit_wg_sum<double>(s, lds_d);
    if (t == 0) o[j] = s / norm;
  }
}

}  // namespace simmr
