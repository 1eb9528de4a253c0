// regions_kernels.hip — the gold-standard assembly on the device (gfx950): the stretches of every contig that a depth[]
// array covers well enough, as a region list and as their bases (include/simmr_hip.h states run, region and base stream).
// Included by regions.hip alone, the library's fourth translation unit: nothing here is seen by engine.hip, whose kernel
// budget stays what it was.
//
// Seven kernels.  No rank comes from an atomic: every place is a count and a scan, so launch geometry never changes a byte.
//   k_regions_count    per tile of REGIONS_TILE positions: the run starts and the run ends it holds.  A position is a START
//                      if it qualifies (depth >= min_depth) and its left neighbour does not, or it is a contig's first
//                      position; an END is marked at the position BEHIND a run's last one (so both need the left neighbour
//                      only), and the tiles cover n_positions + 1 positions so that a run reaching the array's end has one.
//   k_regions_scan     ONE workgroup per array: exclusive scan of 64-bit counts into 64-bit prefixes, REGIONS_TOPS_WIDTH
//                      counts per iteration of its loop (any number of tiles); the total behind the last prefix.
//   k_regions_runs     finds the marks again and writes starts and ends at their ranks: the k-th start pairs with the
//                      k-th end, because runs are disjoint and in position order.
//   k_regions_flag     one lane per run: is it a region (end - start >= min_len), and its length if so, summed per
//                      workgroup of REGIONS_RUN_TILE runs.
//   k_regions_compact  the same flags again, ranked: the engine's region table (where the region starts in depth[], its
//                      contig, its offset in the base stream).
//   k_regions_columns  one lane per region: the caller's columns from the region table.
//   k_regions_bases    one lane per 16-byte chunk of the base stream: region by bisection over the offsets, codes from
//                      the 2-bit plane through the funnel-shift window of the emit and truth kernels, one 16-byte store; and
//                      the sum of depth[] over the chunk, reduced over the wave before it is added to depth_sum[region].
// How a wave sees its positions: a wave owns REGIONS_WAVE_SPAN consecutive positions and takes them with four 16-byte
// loads per lane (lane l of load k holds positions span + 256 k + 4 l .. + 3).  The left neighbour of a lane's first
// position is bit 3 of the lane below, taken from one ballot; the wave's first lane loads depth[x - 1] behind a bounds
// check.  Contig boundaries come from one bisection per wave over the contig-first table and a walk from there.
// Tried: this form only (DESIGN.md section 4 has the measured times).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#include "device_types.hpp"

namespace simmr {

constexpr uint32_t REGIONS_WG = 256;           // threads of every workgroup here
constexpr uint32_t REGIONS_TILE = 4096;        // positions of a tile
constexpr uint32_t REGIONS_WAVE_SPAN = 1024;   // consecutive positions of a tile that one wave owns
constexpr uint32_t REGIONS_SUB = 256;          // positions a wave loads with one instruction
constexpr uint32_t REGIONS_SUBS = REGIONS_WAVE_SPAN / REGIONS_SUB;
constexpr uint32_t REGIONS_TOPS_WIDTH = 1024;  // counts k_regions_scan takes per iteration of its loop
constexpr uint32_t REGIONS_RUN_TILE = 256;     // runs of a workgroup of k_regions_flag / k_regions_compact: one per lane
constexpr uint32_t REGIONS_CHUNK = 16;         // bases of a work unit of k_regions_bases
static_assert(REGIONS_TILE == (REGIONS_WG / 64) * REGIONS_WAVE_SPAN && REGIONS_SUB == 64 * 4 && REGIONS_TOPS_WIDTH == REGIONS_WG * 4,
              "four waves, four positions and four counts per lane");

#define REGIONS_DEV __device__ __forceinline__

typedef uint32_t regions_v4u __attribute__((ext_vector_type(4)));
typedef regions_v4u __attribute__((aligned(4))) regions_v4u_a4;  // sixteen entries of depth[] from any entry
typedef uint64_t __attribute__((aligned(4))) regions_u64_a4;     // two plane words from any word

// One tracked contig, in the order of depth[]: where its bases are and what the columns call it.
struct RegionContig {
  const uint32_t* packed;   // the genome's 2-bit plane from its word 0
  const uint32_t* mask;     // its exception plane, nullptr for a genome of pure ACGT
  const ContigDev* entry;   // the contig's record in the genome's device table (base: its first base in the planes)
  uint64_t first;           // its first position in depth[]
  uint32_t genome, contig;  // genome slot, index of the Seq inside the genome
};

// inclusive scan over the wave: four DPP row shifts, then row_bcast:15 and row_bcast:31 (GFX9)
REGIONS_DEV uint32_t regions_wave_scan(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
  return v;
}
// the same for 64-bit values (the lengths of runs: their sum passes 2^32 on a 5 Gbp genome)
REGIONS_DEV uint64_t regions_wave_scan64(uint64_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const uint64_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
REGIONS_DEV uint64_t regions_wave_sum64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- marks ----------------------------------------------------------------------------------------------------------
// The marks of the REGIONS_WAVE_SPAN positions from wave_base (a multiple of it) on: bit 4 k + i of s / e belongs to position
// wave_base + 256 k + 4 lane + i.  s: a run starts here.  e: a run ends in front of here.  depth has n entries and is
// 16-byte aligned; a position at or behind n does not qualify, and no entry at or behind n is loaded.  cfirst has
// n_contigs + 1 ascending entries, the last one n.
struct RegionMarks {
  uint32_t s, e;
};
REGIONS_DEV RegionMarks regions_marks(const uint32_t* __restrict__ depth, uint64_t n, uint32_t min_depth,
                                      const uint64_t* __restrict__ cfirst, uint32_t n_contigs, uint64_t wave_base, uint32_t lane) {
  uint32_t j = 0, hi = n_contigs + 1u;  // the first boundary at or behind wave_base (uniform over the wave)
  while (j < hi) {
    const uint32_t mid = (j + hi) >> 1;
    if (cfirst[mid] < wave_base) j = mid + 1u; else hi = mid;
  }
  uint32_t left0 = 0;  // lane 0: does the position in front of this load's first one qualify
  if (lane == 0 && wave_base > 0 && wave_base - 1u < n) left0 = depth[wave_base - 1u] >= min_depth ? 1u : 0u;
  RegionMarks m{0u, 0u};
#pragma unroll
  for (uint32_t k = 0; k < REGIONS_SUBS; k++) {
    const uint64_t seg = wave_base + (uint64_t)k * REGIONS_SUB, x = seg + 4u * lane;
    uint32_t q = 0;
    if (x + 4u <= n) {
      const regions_v4u v = *reinterpret_cast<const regions_v4u*>(depth + x);
      q = (v.x >= min_depth ? 1u : 0u) | (v.y >= min_depth ? 2u : 0u) | (v.z >= min_depth ? 4u : 0u) | (v.w >= min_depth ? 8u : 0u);
    } else {
#pragma unroll
      for (uint32_t i = 0; i < 4u; i++)
        if (x + i < n && depth[x + i] >= min_depth) q |= 1u << i;
    }
    uint32_t b = 0;  // contig boundaries among this lane's four positions (the walk is uniform over the wave)
    while (j <= n_contigs) {
      const uint64_t c = cfirst[j];
      if (c >= seg + REGIONS_SUB) break;
      if (((c - seg) >> 2) == lane) b |= 1u << ((uint32_t)c & 3u);
      j++;
    }
    const uint64_t top = __ballot((q & 8u) != 0u);
    const uint32_t left = lane ? (uint32_t)(top >> (lane - 1u)) & 1u : left0;
    const uint32_t qp = ((q << 1) | left) & 0xfu;  // the left neighbour of each of the four qualifies
    m.s |= (q & (b | ~qp) & 0xfu) << (4u * k);
    m.e |= (qp & (b | ~q) & 0xfu) << (4u * k);
    left0 = (uint32_t)(top >> 63);
  }
  return m;
}
REGIONS_DEV uint32_t regions_nibble_counts(const RegionMarks& m, uint32_t k) {  // starts | ends << 16 of load k
  return (uint32_t)__builtin_popcount((m.s >> (4u * k)) & 0xfu) | (uint32_t)__builtin_popcount((m.e >> (4u * k)) & 0xfu) << 16;
}

// ---- count ----------------------------------------------------------------------------------------------------------
// tile_count: the starts per tile, and `padded` entries further on the ends per tile (both zeroed by the host up to padded).
// A tile holds at most REGIONS_TILE marks of a kind: the packed 16-bit halves cannot carry into each other.
extern "C" __global__ void __launch_bounds__(REGIONS_WG)
k_regions_count(const uint32_t* __restrict__ depth, uint64_t n, uint32_t min_depth, const uint64_t* __restrict__ cfirst,
                uint32_t n_contigs, uint64_t* __restrict__ tile_count, uint64_t padded) {
  __shared__ uint32_t wsum[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t wave_base = (uint64_t)blockIdx.x * REGIONS_TILE + (uint64_t)wave * REGIONS_WAVE_SPAN;
  const RegionMarks m = regions_marks(depth, n, min_depth, cfirst, n_contigs, wave_base, lane);
  uint32_t v = (uint32_t)__builtin_popcount(m.s) | (uint32_t)__builtin_popcount(m.e) << 16;
  v = regions_wave_scan(v);
  if (lane == 63u) wsum[wave] = v;
  __syncthreads();
  if (tid == 0) {
    const uint32_t t = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    tile_count[blockIdx.x] = t & 0xffffu;
    tile_count[padded + blockIdx.x] = t >> 16;
  }
}

// ---- scan -----------------------------------------------------------------------------------------------------------
// Workgroup a scans array a: count + a * padded (n entries, zeros up to padded, a multiple of REGIONS_TOPS_WIDTH) into
// prefix + a * (padded + 1): the exclusive prefix of every entry, and the total in entry `padded`.
extern "C" __global__ void __launch_bounds__(REGIONS_WG)
k_regions_scan(const uint64_t* __restrict__ count, uint64_t* __restrict__ prefix, uint64_t n, uint64_t padded) {
  __shared__ uint64_t wsum[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  count += (uint64_t)blockIdx.x * padded;
  prefix += (uint64_t)blockIdx.x * (padded + 1u);
  uint64_t carry = 0;
  for (uint64_t base = 0; base < n; base += REGIONS_TOPS_WIDTH) {
    const uint64_t* p = count + base + 4u * tid;
    const uint64_t v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
    const uint64_t s = v0 + v1 + v2 + v3, inc = regions_wave_scan64(s, lane);
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    const uint64_t t0 = wsum[0], t1 = wsum[1], t2 = wsum[2], t3 = wsum[3];
    const uint64_t pre = carry + (wave > 0 ? t0 : 0ull) + (wave > 1 ? t1 : 0ull) + (wave > 2 ? t2 : 0ull) + inc - s;
    uint64_t* o = prefix + base + 4u * tid;
    o[0] = pre;
    o[1] = pre + v0;
    o[2] = pre + v0 + v1;
    o[3] = pre + v0 + v1 + v2;
    carry += t0 + t1 + t2 + t3;
    __syncthreads();  // wsum is written again
  }
  if (tid == 0) prefix[padded] = carry;
}

// ---- runs -----------------------------------------------------------------------------------------------------------
// The marks of k_regions_count again, ranked in position order: inside a wave that is load by load, then lane by lane.
// tile_prefix is the scan of tile_count (starts, and padded + 1 entries further on the ends).  A rank is below n_runs when
// depth[] is what the count saw; the check keeps a store inside the run buffers when it is not.
extern "C" __global__ void __launch_bounds__(REGIONS_WG)
k_regions_runs(const uint32_t* __restrict__ depth, uint64_t n, uint32_t min_depth, const uint64_t* __restrict__ cfirst,
               uint32_t n_contigs, const uint64_t* __restrict__ tile_prefix, uint64_t padded, uint64_t n_runs,
               uint64_t* __restrict__ run_start, uint64_t* __restrict__ run_end) {
  __shared__ uint32_t wsum[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t wave_base = (uint64_t)blockIdx.x * REGIONS_TILE + (uint64_t)wave * REGIONS_WAVE_SPAN;
  const RegionMarks m = regions_marks(depth, n, min_depth, cfirst, n_contigs, wave_base, lane);
  uint32_t excl[REGIONS_SUBS], running = 0;  // packed starts | ends << 16 in front of this lane's marks of load k, inside the wave
#pragma unroll
  for (uint32_t k = 0; k < REGIONS_SUBS; k++) {
    const uint32_t v = regions_nibble_counts(m, k), inc = regions_wave_scan(v);
    excl[k] = running + inc - v;
    running += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
  }
  if (lane == 0) wsum[wave] = running;
  __syncthreads();
  if (!(m.s | m.e)) return;
  const uint32_t before = (wave > 0 ? wsum[0] : 0u) + (wave > 1 ? wsum[1] : 0u) + (wave > 2 ? wsum[2] : 0u);
  const uint64_t ps = tile_prefix[blockIdx.x], pe = tile_prefix[padded + 1u + blockIdx.x];
#pragma unroll
  for (uint32_t k = 0; k < REGIONS_SUBS; k++) {
    const uint64_t x = wave_base + (uint64_t)k * REGIONS_SUB + 4u * lane;
    const uint32_t at = before + excl[k];
    uint64_t rs = ps + (at & 0xffffu), re = pe + (at >> 16);
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) {
      if ((m.s >> (4u * k + i)) & 1u) {
        if (rs < n_runs) run_start[rs] = x + i;
        rs++;
      }
      if ((m.e >> (4u * k + i)) & 1u) {
        if (re < n_runs) run_end[re] = x + i;
        re++;
      }
    }
  }
}

// ---- regions among the runs -----------------------------------------------------------------------------------------
// Run r is positions run_start[r] .. run_end[r] - 1 of depth[].  It is a region iff it has min_len positions.
// run_count: the regions per workgroup, and `padded` entries further on the positions of those regions.
extern "C" __global__ void __launch_bounds__(REGIONS_WG)
k_regions_flag(const uint64_t* __restrict__ run_start, const uint64_t* __restrict__ run_end, uint64_t n_runs, uint64_t min_len,
               uint64_t* __restrict__ run_count, uint64_t padded) {
  __shared__ uint64_t wsum[4][2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t r = (uint64_t)blockIdx.x * REGIONS_RUN_TILE + tid;
  uint64_t len = 0;
  if (r < n_runs) len = run_end[r] - run_start[r];
  const bool is = r < n_runs && len >= min_len;
  const uint64_t cnt = regions_wave_sum64(is ? 1ull : 0ull), sum = regions_wave_sum64(is ? len : 0ull);
  if (lane == 0) { wsum[wave][0] = cnt; wsum[wave][1] = sum; }
  __syncthreads();
  if (tid == 0) {
    run_count[blockIdx.x] = wsum[0][0] + wsum[1][0] + wsum[2][0] + wsum[3][0];
    run_count[padded + blockIdx.x] = wsum[0][1] + wsum[1][1] + wsum[2][1] + wsum[3][1];
  }
}

// The flags again, ranked: region k starts at r_x[k] in depth[], lies on tracked contig r_c[k] and its bases start at
// r_off[k] in the base stream; r_off[n_regions] = n_bases.  run_prefix is the scan of run_count.
extern "C" __global__ void __launch_bounds__(REGIONS_WG)
k_regions_compact(const uint64_t* __restrict__ run_start, const uint64_t* __restrict__ run_end, uint64_t n_runs, uint64_t min_len,
                  const uint64_t* __restrict__ run_prefix, uint64_t padded, const uint64_t* __restrict__ cfirst, uint32_t n_contigs,
                  uint64_t n_regions, uint64_t n_bases, uint64_t* __restrict__ r_x, uint32_t* __restrict__ r_c,
                  uint64_t* __restrict__ r_off) {
  __shared__ uint64_t wsum[4][2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t r = (uint64_t)blockIdx.x * REGIONS_RUN_TILE + tid;
  if (blockIdx.x == 0 && tid == 0) r_off[n_regions] = n_bases;
  uint64_t a = 0, len = 0;
  if (r < n_runs) { a = run_start[r]; len = run_end[r] - a; }
  const bool is = r < n_runs && len >= min_len;
  const uint32_t f = is ? 1u : 0u, finc = regions_wave_scan(f);
  const uint64_t l = is ? len : 0ull, linc = regions_wave_scan64(l, lane);
  if (lane == 63u) { wsum[wave][0] = finc; wsum[wave][1] = linc; }
  __syncthreads();
  if (!is) return;
  uint64_t k = run_prefix[blockIdx.x] + (finc - f), off = run_prefix[padded + 1u + blockIdx.x] + (linc - l);
  for (uint32_t w = 0; w < wave; w++) { k += wsum[w][0]; off += wsum[w][1]; }
  if (k >= n_regions) return;  // (depth[] changed under the plan: stay inside the tables)
  uint32_t c = 0, hi = n_contigs;  // the contig of position a: the last c with cfirst[c] <= a (an empty contig in front of it shares its first)
  while (hi - c > 1u) {
    const uint32_t mid = (c + hi) >> 1;
    if (cfirst[mid] <= a) c = mid; else hi = mid;
  }
  r_x[k] = a;
  r_c[k] = c;
  r_off[k] = off;
}

// ---- columns --------------------------------------------------------------------------------------------------------
// Any column may be nullptr.  seq_off takes n_regions + 1 entries.
struct RegionCols {
  uint32_t* genome;
  uint32_t* contig;
  uint64_t* start;
  uint64_t* len;
  uint64_t* seq_off;
};
extern "C" __global__ void __launch_bounds__(REGIONS_WG)
k_regions_columns(const uint64_t* __restrict__ r_x, const uint32_t* __restrict__ r_c, const uint64_t* __restrict__ r_off,
                  const RegionContig* __restrict__ table, uint64_t n_regions, RegionCols out) {
  const uint64_t k = (uint64_t)blockIdx.x * REGIONS_WG + threadIdx.x;
  if (k > n_regions) return;
  const uint64_t off = r_off[k];
  if (out.seq_off) out.seq_off[k] = off;
  if (k == n_regions) return;
  const RegionContig T = table[r_c[k]];
  if (out.genome) out.genome[k] = T.genome;
  if (out.contig) out.contig[k] = T.contig;
  if (out.start) out.start[k] = r_x[k] - T.first;
  if (out.len) out.len[k] = r_off[k + 1u] - off;
}

// ---- bases ----------------------------------------------------------------------------------------------------------
// 4 codes (8 bits) + 4 exception bits -> 4 ASCII bytes: selector 0-3 -> "ACGT", 4-7 -> "N-N-" (the emit kernels' expand4)
REGIONS_DEV uint32_t regions_expand4(uint32_t c8, uint32_t m4) {
  uint32_t sel = (c8 | (c8 << 6) | (c8 << 12) | (c8 << 18)) & 0x03030303u;
  const uint32_t ms = (m4 | (m4 << 7) | (m4 << 14) | (m4 << 21)) & 0x01010101u;
  sel |= ms << 2;
  return __builtin_amdgcn_perm(0x2D4E2D4Eu, 0x54474341u, sel);
}
// Sixteen codes / exception bits from base p of a plane on: two words from the word of p, funnel-shifted.  The bound the
// loads rely on: the window's last base p + 15 lies inside the region's contig, so the second word is at most ONE word
// behind the word of the contig's last base — the planes carry 24 words behind their last base (engine.hip,
// BACK_PAD_WORDS), and a contig's own padding to 64 bases comes first.
typedef const __attribute__((address_space(1))) regions_u64_a4* regions_plane_ptr;
REGIONS_DEV uint32_t regions_codes16(const uint32_t* __restrict__ packed, uint64_t p) {
  return (uint32_t)(*(regions_plane_ptr)(packed + (p >> 4)) >> ((uint32_t)(p & 15u) * 2u));
}
REGIONS_DEV uint32_t regions_mask16(const uint32_t* __restrict__ mask, uint64_t p) {
  return (uint32_t)(*(regions_plane_ptr)(mask + (p >> 5)) >> (uint32_t)(p & 31u)) & 0xffffu;
}

// A region as the base kernel needs it.
struct RegionSrc {
  const uint32_t* packed;
  const uint32_t* mask;
  uint64_t p0;        // plane position of the region's first base
  uint64_t x0;        // its first position in depth[]
  uint64_t off, end;  // its bytes of the base stream: [off, end)
};
REGIONS_DEV RegionSrc regions_open(uint64_t k, const uint64_t* __restrict__ r_x, const uint32_t* __restrict__ r_c,
                                   const uint64_t* __restrict__ r_off, const RegionContig* __restrict__ table) {
  const RegionContig T = table[r_c[k]];
  const uint64_t x0 = r_x[k];
  return RegionSrc{T.packed, T.mask, T.entry->base + (x0 - T.first), x0, r_off[k], r_off[k + 1u]};
}

// Lane t of the grid owns bytes [16 t, 16 t + 16) of seq (16-byte aligned, at least n_bases bytes).  A chunk inside one
// region is one window and one 16-byte store; a chunk that straddles regions (they may be one base long) or ends the
// stream goes base by base.  seq == nullptr: no bases; depth_sum == nullptr: no sums (the host has zeroed depth_sum).
// Every plane load is inside the region's contig but for the window's second word (above); every depth[] load is inside
// the region.
extern "C" __global__ void __launch_bounds__(REGIONS_WG)
k_regions_bases(const uint32_t* __restrict__ depth, const uint64_t* __restrict__ r_x, const uint32_t* __restrict__ r_c,
                const uint64_t* __restrict__ r_off, const RegionContig* __restrict__ table, uint64_t n_regions, uint64_t n_bases,
                uint8_t* __restrict__ seq, unsigned long long* __restrict__ depth_sum) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t j = ((uint64_t)blockIdx.x * REGIONS_WG + threadIdx.x) * REGIONS_CHUNK;
  uint64_t k = 0, sum = 0;  // this lane's region, and what it has to add to depth_sum[k]
  if (j < n_bases) {
    uint64_t hi = n_regions;  // the last k with r_off[k] <= j (r_off ascends strictly: a region has a base)
    while (hi - k > 1u) {
      const uint64_t mid = (k + hi) >> 1;
      if (r_off[mid] <= j) k = mid; else hi = mid;
    }
    RegionSrc R = regions_open(k, r_x, r_c, r_off, table);
    if (R.end >= j + REGIONS_CHUNK) {
      const uint64_t d = j - R.off;
      if (seq) {
        const uint32_t codes = regions_codes16(R.packed, R.p0 + d), exc = R.mask ? regions_mask16(R.mask, R.p0 + d) : 0u;
        regions_v4u o;
        o.x = regions_expand4(codes & 0xffu, exc & 0xfu);
        o.y = regions_expand4((codes >> 8) & 0xffu, (exc >> 4) & 0xfu);
        o.z = regions_expand4((codes >> 16) & 0xffu, (exc >> 8) & 0xfu);
        o.w = regions_expand4(codes >> 24, (exc >> 12) & 0xfu);
        __builtin_nontemporal_store(o, reinterpret_cast<regions_v4u*>(seq + j));
      }
      if (depth_sum) {
        const regions_v4u_a4* p = reinterpret_cast<const regions_v4u_a4*>(depth + R.x0 + d);
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
          const regions_v4u v = p[i];
          sum += (uint64_t)v.x + v.y + v.z + v.w;
        }
      }
    } else {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      uint64_t part = 0;
#pragma unroll
      for (uint32_t b = 0; b < REGIONS_CHUNK; b++) {
        const uint64_t jj = j + b;
        if (jj < n_bases) {
          if (jj >= R.end) {  // (the next region starts at this byte: regions have a base each)
            if (depth_sum && part) atomicAdd(depth_sum + k, (unsigned long long)part);
            part = 0;
            k++;
            R = regions_open(k, r_x, r_c, r_off, table);
          }
          const uint64_t d = jj - R.off, p = R.p0 + d;
          if (seq) {
            const uint32_t code = (R.packed[p >> 4] >> ((uint32_t)(p & 15u) * 2u)) & 3u;
            const uint32_t exc = R.mask ? (R.mask[p >> 5] >> (uint32_t)(p & 31u)) & 1u : 0u;
            w[b >> 2] |= (regions_expand4(code, exc) & 0xffu) << ((b & 3u) * 8u);
          }
          if (depth_sum) part += depth[R.x0 + d];
        }
      }
      if (depth_sum && part) atomicAdd(depth_sum + k, (unsigned long long)part);
      if (seq) {
        if (j + REGIONS_CHUNK <= n_bases) {
          __builtin_nontemporal_store(regions_v4u{w[0], w[1], w[2], w[3]}, reinterpret_cast<regions_v4u*>(seq + j));
        } else {
#pragma unroll
          for (uint32_t b = 0; b < REGIONS_CHUNK; b++)
            if (j + b < n_bases) seq[j + b] = (uint8_t)(w[b >> 2] >> ((b & 3u) * 8u));
        }
      }
    }
  }
  if (!depth_sum) return;  // (uniform)
  // one add per wave where the wave's sums belong to one region, else one per lane
  const uint64_t have = __ballot(sum != 0);
  if (!have) return;
  const uint64_t k0 = __shfl(k, (int)__builtin_ctzll(have), 64);
  if (__all(sum == 0 || k == k0)) {
    const uint64_t total = regions_wave_sum64(sum);
    if (lane == 0) atomicAdd(depth_sum + k0, (unsigned long long)total);
  } else if (sum) {
    atomicAdd(depth_sum + k, (unsigned long long)sum);
  }
}

}  // namespace simmr
