// depth_kernels.hip — coverage depth on the device (gfx950): where the reads of a run landed (include/simmr_hip.h states
// depth[], the contig rows, the histogram and the windows).  Included by depth.hip alone, the library's second translation
// unit: nothing here is seen by engine.hip, whose kernel budget stays what it was.
//
// Five kernels.
//   k_depth_mark       one lane per read: +1 at the read's first position, -1 behind its last one, in a difference array
//                      of n_positions + 1 int32 (no-return relaxed agent-scope atomics).  The -1 of a read that ends at its
//                      contig's end lands on slot 0 of the next contig, or on the extra last slot: a scan over the dense
//                      layout is still right, because the running sum at x is (starts <= x) - (ends <= x).
//   k_depth_tile_sums  \  the scan of the difference array into depth[]: the sum of every tile of DEPTH_TILE entries, an
//   k_depth_scan_tiles  > exclusive scan of the tile sums by ONE workgroup that loops DEPTH_TOPS_WIDTH sums at a time (any
//   k_depth_apply      /  number of tiles), then every tile scanned again from its prefix.  16-byte loads and stores; a
//                      wave scans with the DPP row ladder and the two row broadcasts, the four waves of a workgroup meet
//                      in LDS once per tile.
//   k_depth_summarize  one wave per window (or per chunk of DEPTH_TILE positions when no windows are asked for): sum,
//                      covered and max of the window, a 256-bin histogram in LDS per workgroup flushed once, and the
//                      contig rows from running sums a wave keeps while it stays on one contig.
// Tried: this form only.  The mark is bound by its scattered 4-byte atomics (two per read), not by its 24 bytes of
// columns; one lane per PAIR that merges the mates' marks, and marks sorted by tile in LDS before the atomics, were
// weighed and not built (DESIGN.md section 4 has the measured time).
//
// What bounds a 32-bit partial: fewer than 2^31 reads are added between two resets (simmr_depth_add refuses more), so
// every sum of difference entries — a tile's, a prefix, a depth — is below 2^31 in magnitude.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"

namespace simmr {

constexpr uint32_t DEPTH_WG = 256;                         // threads of every workgroup here
constexpr uint32_t DEPTH_VEC = 4;                          // entries of a 16-byte load
constexpr uint32_t DEPTH_SUB = DEPTH_WG * DEPTH_VEC;       // entries a workgroup loads with one instruction
constexpr uint32_t DEPTH_TILE = 4096;                      // entries of a scan tile: DEPTH_TILE / DEPTH_SUB loads per lane
constexpr uint32_t DEPTH_SUBS = DEPTH_TILE / DEPTH_SUB;
constexpr uint32_t DEPTH_TOPS_WIDTH = 1024;                // tile sums k_depth_scan_tiles takes per iteration of its loop
static_assert(DEPTH_TILE % DEPTH_SUB == 0 && DEPTH_TOPS_WIDTH == DEPTH_SUB, "whole 16-byte loads per lane");

#define DEPTH_DEV __device__ __forceinline__

typedef int32_t depth_v4i __attribute__((ext_vector_type(4)));
typedef uint32_t depth_v4u __attribute__((ext_vector_type(4)));

// a genome slot of the layout a reset recorded: its contigs are cfirst[cbase .. cbase + n_contigs]; n_contigs == 0: not tracked
struct DepthSlot {
  uint32_t cbase, n_contigs;
};

// inclusive scan over the wave: four DPP row shifts, then row_bcast:15 and row_bcast:31 (GFX9)
DEPTH_DEV uint32_t depth_wave_scan(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
  return v;
}
DEPTH_DEV uint32_t depth_sum4(depth_v4i v) { return (uint32_t)v.x + (uint32_t)v.y + (uint32_t)v.z + (uint32_t)v.w; }

// ---- mark -----------------------------------------------------------------------------------------------------------
// 24 bytes of columns per read.  The bounds check comes before any address is formed from the read: a read that fails it
// sets the error word and adds nothing.  All indices are 64-bit (a 5 Gbp genome passes 2^32 positions).
extern "C" __global__ void __launch_bounds__(DEPTH_WG)
k_depth_mark(const uint64_t* __restrict__ start, const uint64_t* __restrict__ end, const uint32_t* __restrict__ contig,
             const uint32_t* __restrict__ genome, uint64_t n_reads, const DepthSlot* __restrict__ slots, uint32_t n_slots,
             const uint64_t* __restrict__ cfirst, int32_t* __restrict__ diff, uint32_t* __restrict__ err) {
  const uint64_t r = (uint64_t)blockIdx.x * DEPTH_WG + threadIdx.x;
  if (r >= n_reads) return;
  const uint64_t a = start[r], b = end[r];
  const uint32_t c = contig[r], g = genome[r];
  const uint64_t lo = a < b ? a : b, L = a < b ? b - a : a - b;
  DepthSlot s{0u, 0u};
  if (g < n_slots) s = slots[g];
  uint64_t first = 0, len = 0;
  const bool known = c < s.n_contigs;
  if (known) {
    first = cfirst[s.cbase + c];
    len = cfirst[s.cbase + c + 1u] - first;
  }
  if (!known || lo > len || L > len - lo) {
    atomicOr(err, 1u);
    return;
  }
  if (L == 0) return;
  (void)__hip_atomic_fetch_add(diff + first + lo, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_add(diff + first + lo + L, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- scan -----------------------------------------------------------------------------------------------------------
// diff is padded with zeros to whole tiles.  Lane t of a workgroup owns entries s * DEPTH_SUB + 4 t .. + 3 of sub-tile s.
extern "C" __global__ void __launch_bounds__(DEPTH_WG)
k_depth_tile_sums(const depth_v4i* __restrict__ diff, int32_t* __restrict__ tile_sum) {
  __shared__ uint32_t wsum[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const depth_v4i* p = diff + (uint64_t)blockIdx.x * (DEPTH_TILE / DEPTH_VEC) + tid;
  uint32_t s = 0;
#pragma unroll
  for (uint32_t k = 0; k < DEPTH_SUBS; k++) s += depth_sum4(p[k * DEPTH_WG]);
  s = depth_wave_scan(s);
  if (lane == 63u) wsum[wave] = s;
  __syncthreads();
  if (tid == 0) tile_sum[blockIdx.x] = (int32_t)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

// One workgroup: exclusive scan of tile_sum in place (padded with zeros to whole iterations).  The loop makes it right
// for any number of tiles.
extern "C" __global__ void __launch_bounds__(DEPTH_WG)
k_depth_scan_tiles(int32_t* __restrict__ tile_sum, uint64_t n_tiles) {
  __shared__ uint32_t wsum[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t carry = 0;
  for (uint64_t base = 0; base < n_tiles; base += DEPTH_TOPS_WIDTH) {
    depth_v4i* p = reinterpret_cast<depth_v4i*>(tile_sum + base) + tid;
    const depth_v4i v = *p;
    const uint32_t s = depth_sum4(v), inc = depth_wave_scan(s);
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    const uint32_t t0 = wsum[0], t1 = wsum[1], t2 = wsum[2], t3 = wsum[3];
    const uint32_t pre = carry + (wave > 0 ? t0 : 0u) + (wave > 1 ? t1 : 0u) + (wave > 2 ? t2 : 0u) + inc - s;
    depth_v4i o;
    o.x = (int32_t)pre;
    o.y = (int32_t)(pre + (uint32_t)v.x);
    o.z = (int32_t)(pre + (uint32_t)v.x + (uint32_t)v.y);
    o.w = (int32_t)(pre + (uint32_t)v.x + (uint32_t)v.y + (uint32_t)v.z);
    *p = o;
    carry += t0 + t1 + t2 + t3;
    __syncthreads();  // wsum is written again
  }
}

// depth[x] = tile_prefix[tile of x] + the inclusive scan of diff inside the tile.  out holds n_positions entries and is
// 16-byte aligned: whole groups of four are stored at once, the last group of the array entry by entry.
extern "C" __global__ void __launch_bounds__(DEPTH_WG)
k_depth_apply(const depth_v4i* __restrict__ diff, const int32_t* __restrict__ tile_prefix, uint32_t* __restrict__ out,
              uint64_t n_positions) {
  __shared__ uint32_t wsum[DEPTH_SUBS][4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * DEPTH_TILE;
  const depth_v4i* p = diff + base / DEPTH_VEC + tid;
  depth_v4i v[DEPTH_SUBS];
  uint32_t s[DEPTH_SUBS], inc[DEPTH_SUBS];
#pragma unroll
  for (uint32_t k = 0; k < DEPTH_SUBS; k++) v[k] = p[k * DEPTH_WG];
#pragma unroll
  for (uint32_t k = 0; k < DEPTH_SUBS; k++) {
    s[k] = depth_sum4(v[k]);
    inc[k] = depth_wave_scan(s[k]);
    if (lane == 63u) wsum[k][wave] = inc[k];
  }
  __syncthreads();
  uint32_t running = (uint32_t)tile_prefix[blockIdx.x];
#pragma unroll
  for (uint32_t k = 0; k < DEPTH_SUBS; k++) {
    const uint32_t t0 = wsum[k][0], t1 = wsum[k][1], t2 = wsum[k][2], t3 = wsum[k][3];
    const uint32_t pre = running + (wave > 0 ? t0 : 0u) + (wave > 1 ? t1 : 0u) + (wave > 2 ? t2 : 0u) + inc[k] - s[k];
    depth_v4u d;
    d.x = pre + (uint32_t)v[k].x;
    d.y = d.x + (uint32_t)v[k].y;
    d.z = d.y + (uint32_t)v[k].z;
    d.w = d.z + (uint32_t)v[k].w;
    const uint64_t i = base + (uint64_t)k * DEPTH_SUB + (uint64_t)tid * DEPTH_VEC;
    if (i + DEPTH_VEC <= n_positions) {
      *reinterpret_cast<depth_v4u*>(out + i) = d;
    } else {
      if (i < n_positions) out[i] = d.x;
      if (i + 1 < n_positions) out[i + 1] = d.y;
      if (i + 2 < n_positions) out[i + 2] = d.z;
    }
    running += t0 + t1 + t2 + t3;
  }
}

// ---- summarize ------------------------------------------------------------------------------------------------------
// A unit is a window of `window` positions of one contig (the contig's last one partial): contig c owns units
// fwin[c] .. fwin[c + 1] - 1 and positions cfirst[c] .. cfirst[c + 1] - 1.  Wave w of the grid takes units
// [w * units_per_wave, (w + 1) * units_per_wave): consecutive units, so it stays on one contig for long and adds that
// contig's running sums to rows[] (sum, covered, max: three 64-bit words per contig, zeroed by the host) only when it leaves
// it.  win_sum == nullptr: no window columns (the host then asks for chunks of DEPTH_TILE positions).
// The host sizes units_per_wave so that a workgroup sees fewer than 2^32 positions: an LDS bin cannot wrap.
extern "C" __global__ void __launch_bounds__(DEPTH_WG)
k_depth_summarize(const uint32_t* __restrict__ depth, const uint64_t* __restrict__ cfirst, const uint64_t* __restrict__ fwin,
                  uint32_t n_contigs, uint32_t window, uint64_t n_units, uint64_t units_per_wave,
                  unsigned long long* __restrict__ win_sum, uint32_t* __restrict__ win_cov, uint32_t* __restrict__ win_max,
                  unsigned long long* __restrict__ rows, unsigned long long* __restrict__ hist) {
  __shared__ uint32_t bins[SIMMR_DEPTH_HIST_BINS];
  static_assert(SIMMR_DEPTH_HIST_BINS == DEPTH_WG, "one bin per thread");
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  bins[tid] = 0u;
  __syncthreads();
  const uint64_t gw = (uint64_t)blockIdx.x * (DEPTH_WG / 64u) + __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t u0 = gw * units_per_wave;
  const uint64_t u1 = u0 + units_per_wave < n_units ? u0 + units_per_wave : n_units;
  if (u0 < u1) {  // (uniform over the wave, like everything below but the position loop)
    uint32_t c = 0, hi = n_contigs;  // the contig of u0: the first c with fwin[c + 1] > u0
    while (c < hi) {
      const uint32_t mid = (c + hi) >> 1;
      if (fwin[mid + 1u] > u0) hi = mid; else c = mid + 1u;
    }
    unsigned long long csum = 0, ccov = 0, cmax = 0;
    auto leave = [&](uint32_t at) {
      if (lane == 0 && (csum | ccov | cmax)) {
        atomicAdd(rows + 3ull * at, csum);
        atomicAdd(rows + 3ull * at + 1u, ccov);
        atomicMax(rows + 3ull * at + 2u, cmax);
      }
      csum = ccov = cmax = 0;
    };
    for (uint64_t u = u0; u < u1; u++) {
      while (u >= fwin[c + 1u]) { leave(c); c++; }  // (u < n_units = fwin[n_contigs]: c stays below n_contigs)
      const uint64_t a = cfirst[c] + (u - fwin[c]) * window, cend = cfirst[c + 1u];
      const uint64_t b = a + window < cend ? a + window : cend;
      unsigned long long sum = 0;
      uint32_t cov = 0, mx = 0;
      for (uint64_t x = a + lane; x < b; x += 64u) {
        const uint32_t d = depth[x];
        sum += d;
        cov += d ? 1u : 0u;
        mx = d > mx ? d : mx;
        atomicAdd(&bins[d < SIMMR_DEPTH_HIST_BINS ? d : SIMMR_DEPTH_HIST_BINS - 1u], 1u);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        cov += __shfl_xor(cov, o, 64);
        const uint32_t m2 = __shfl_xor(mx, o, 64);
        mx = m2 > mx ? m2 : mx;
      }
      if (win_sum && lane == 0) {
        win_sum[u] = sum;
        win_cov[u] = cov;
        win_max[u] = mx;
      }
      csum += sum;
      ccov += cov;
      cmax = mx > cmax ? mx : cmax;
    }
    leave(c);
  }
  __syncthreads();
  const uint32_t n = bins[tid];
  if (n) atomicAdd(hist + tid, (unsigned long long)n);
}

}  // namespace simmr
