// strain_kernels.hip — strain divergence on the device (gfx950): substitutions drawn per base of a staged genome and
// written into its 2-bit plane in place, with the list of the sites (include/simmr_hip.h states "strain sites, version 1").
// Included by strain.hip alone, the library's third translation unit: nothing here is seen by engine.hip, whose kernel
// budget stays what it was.
//
// Three kernels.
//   k_strain_count       one lane per 32-bit plane word (16 bases = four Philox blocks): the sites of the word, summed over
//                        the STRAIN_TILE bases of the workgroup's tile.
//   k_strain_scan_tiles  ONE workgroup: exclusive scan of the tile counts into 64-bit prefixes, STRAIN_TOPS_WIDTH counts per
//                        iteration of its loop (any number of tiles); the total behind the last prefix.
//   k_strain_apply       draws the word's sites again, ranks them (tile prefix + scan over the workgroup), writes the site
//                        columns at their ranks and the word back.  A lane owns its word, and contigs start on 64-base
//                        boundaries, so a word belongs to one contig and the rewrite has no cross-lane hazard.
// A lane is addressed by plane word, finds its contig by bisection over the genome's contig table (bounds first: a word
// behind the plane, and the padding bases behind a contig's end, are never loaded or stored) and draws with the round of
// rng_device.hpp.  The wave scan is depth_kernels.hip's DPP ladder, restated here because that file defines kernels and
// cannot be included twice into one library.
// Tried: this form only (DESIGN.md section 4 has the measured time).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#include "rng_device.hpp"

namespace simmr {

constexpr uint32_t STRAIN_WG = 256;                                  // threads of every workgroup here
constexpr uint32_t STRAIN_WORD_BASES = 16;                           // bases of a plane word: what one lane owns
constexpr uint32_t STRAIN_TILE = 4096;                               // bases of a tile: one word per lane
constexpr uint32_t STRAIN_TOPS_WIDTH = 1024;                         // tile counts k_strain_scan_tiles takes per iteration of its loop
constexpr uint32_t STRAIN_DOMAIN = 5;                                // second counter word of the draws
static_assert(STRAIN_TILE == STRAIN_WG * STRAIN_WORD_BASES && STRAIN_TOPS_WIDTH == STRAIN_WG * 4, "one word, one 16-byte load per lane");

typedef uint32_t strain_v4u __attribute__((ext_vector_type(4)));

// the draw's integer thresholds and key (simmr_strain_plan computes them once on the host)
struct StrainDraw {
  uint32_t t32, a, b;  // site iff X < t32; s = 1 + (X >= a) + (X >= b)
  uint32_t k0, k1;     // seed low / high word
};

// inclusive scan over the wave: four DPP row shifts, then row_bcast:15 and row_bcast:31 (GFX9)
SIMMR_DEV uint32_t strain_wave_scan(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
  return v;
}

// What a lane knows about its word: contig, position of the word's first base in the contig, and the word's sites.
struct StrainWord {
  uint32_t contig;
  uint64_t pos0;
  uint32_t sites;  // bit b: base b of the word is a site
  uint32_t shift;  // bits [2b, 2b + 2): s of base b (0 where it is no site)
};

// The sites of plane word w (w < plane_words, checked by the caller).  Nothing is loaded for a word that lies wholly in
// the padding behind its contig.
SIMMR_DEV StrainWord strain_draw_word(uint64_t w, const uint32_t* __restrict__ mask, const ContigDev* __restrict__ contigs,
                                      uint32_t n_contigs, const StrainDraw& d) {
  StrainWord r{0u, 0ull, 0u, 0u};
  const uint64_t pb = w * STRAIN_WORD_BASES;
  uint32_t c = 0, hi = n_contigs;  // the last contig whose base is <= pb (contigs[0].base == 0)
  while (hi - c > 1u) {
    const uint32_t mid = (c + hi) >> 1;
    if (contigs[mid].base <= pb) c = mid; else hi = mid;
  }
  const uint64_t pos0 = pb - contigs[c].base, len = contigs[c].len;
  r.contig = c;
  r.pos0 = pos0;
  if (pos0 >= len) return r;
  const uint32_t n_valid = len - pos0 < STRAIN_WORD_BASES ? (uint32_t)(len - pos0) : STRAIN_WORD_BASES;
  uint32_t open = 0xffffu >> (STRAIN_WORD_BASES - n_valid);  // bases that exist and are not under the exception plane
  if (mask) open &= ~(mask[w >> 1] >> ((uint32_t)(w & 1u) * 16u));
  const uint32_t blk0 = (uint32_t)(pos0 >> 2);  // (a contig has fewer than 2^34 bases: simmr_strain_plan)
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    uint32_t x[4];
    philox4x32_10_ctr(blk0 + j, STRAIN_DOMAIN, c, 0x72000003u, d.k0, d.k1, x);
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
      const uint32_t b = 4u * j + i;
      const uint32_t site = x[i] < d.t32 ? 1u : 0u;
      const uint32_t s = 1u + (x[i] >= d.a ? 1u : 0u) + (x[i] >= d.b ? 1u : 0u);
      r.sites |= site << b;
      r.shift |= (site ? s : 0u) << (2u * b);
    }
  }
  r.sites &= open;
  return r;
}

// ---- count ----------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(STRAIN_WG)
k_strain_count(const uint32_t* __restrict__ mask, const ContigDev* __restrict__ contigs, uint32_t n_contigs, uint64_t plane_words,
               StrainDraw d, uint32_t* __restrict__ tile_count) {
  __shared__ uint32_t wsum[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t w = (uint64_t)blockIdx.x * STRAIN_WG + tid;
  uint32_t n = 0;
  if (w < plane_words) n = (uint32_t)__builtin_popcount(strain_draw_word(w, mask, contigs, n_contigs, d).sites);
  n = strain_wave_scan(n);
  if (lane == 63u) wsum[wave] = n;
  __syncthreads();
  if (tid == 0) tile_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// ---- scan -----------------------------------------------------------------------------------------------------------
// One workgroup.  tile_count is padded with zeros to whole iterations and tile_prefix has as many entries plus one: the
// exclusive prefix of every tile, and the total in tile_prefix[padded n_tiles].  A tile holds at most STRAIN_TILE sites, so
// the sums of one iteration fit 32 bits; the carry between iterations is 64 bits (a 5 Gbp genome at identity 0.25 has
// more than 2^32 sites).
extern "C" __global__ void __launch_bounds__(STRAIN_WG)
k_strain_scan_tiles(const uint32_t* __restrict__ tile_count, uint64_t* __restrict__ tile_prefix, uint64_t n_tiles) {
  __shared__ uint32_t wsum[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint64_t carry = 0, base = 0;
  for (; base < n_tiles; base += STRAIN_TOPS_WIDTH) {
    const strain_v4u v = *(reinterpret_cast<const strain_v4u*>(tile_count + base) + tid);
    const uint32_t s = v.x + v.y + v.z + v.w, inc = strain_wave_scan(s);
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    const uint32_t t0 = wsum[0], t1 = wsum[1], t2 = wsum[2], t3 = wsum[3];
    const uint64_t pre = carry + ((wave > 0 ? t0 : 0u) + (wave > 1 ? t1 : 0u) + (wave > 2 ? t2 : 0u) + inc - s);
    uint64_t* o = tile_prefix + base + 4u * tid;
    o[0] = pre;
    o[1] = pre + v.x;
    o[2] = pre + (v.x + v.y);
    o[3] = pre + (v.x + v.y + v.z);
    carry += t0 + t1 + t2 + t3;
    __syncthreads();  // wsum is written again
  }
  if (tid == 0) tile_prefix[base] = carry;
}

// ---- apply ----------------------------------------------------------------------------------------------------------
// Any of the four columns may be nullptr.  The host has checked the columns' capacity against the total of the scan, and
// the draws are those of the count: every rank is below it.
extern "C" __global__ void __launch_bounds__(STRAIN_WG)
k_strain_apply(uint32_t* __restrict__ packed, const uint32_t* __restrict__ mask, const ContigDev* __restrict__ contigs,
               uint32_t n_contigs, uint64_t plane_words, StrainDraw d, const uint64_t* __restrict__ tile_prefix,
               uint32_t* __restrict__ out_contig, uint64_t* __restrict__ out_pos, uint8_t* __restrict__ out_ref,
               uint8_t* __restrict__ out_alt) {
  __shared__ uint32_t wsum[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t w = (uint64_t)blockIdx.x * STRAIN_WG + tid;
  StrainWord sw{0u, 0ull, 0u, 0u};
  if (w < plane_words) sw = strain_draw_word(w, mask, contigs, n_contigs, d);
  const uint32_t n = (uint32_t)__builtin_popcount(sw.sites), inc = strain_wave_scan(n);
  if (lane == 63u) wsum[wave] = inc;
  __syncthreads();
  if (!sw.sites) return;
  const uint32_t t0 = wsum[0], t1 = wsum[1], t2 = wsum[2];
  uint64_t rank = tile_prefix[blockIdx.x] + ((wave > 0 ? t0 : 0u) + (wave > 1 ? t1 : 0u) + (wave > 2 ? t2 : 0u) + inc - n);
  const uint32_t old = packed[w];
  uint32_t word = old;
  for (uint32_t left = sw.sites; left; left &= left - 1u) {
    const uint32_t b = (uint32_t)__builtin_ctz(left);
    const uint32_t code = (old >> (2u * b)) & 3u, alt = (code + ((sw.shift >> (2u * b)) & 3u)) & 3u;
    word ^= (code ^ alt) << (2u * b);
    if (out_contig) out_contig[rank] = sw.contig;
    if (out_pos) out_pos[rank] = sw.pos0 + b;
    if (out_ref) out_ref[rank] = (uint8_t)"ACGT"[code];
    if (out_alt) out_alt[rank] = (uint8_t)"ACGT"[alt];
    rank++;
  }
  packed[w] = word;
}

}  // namespace simmr
