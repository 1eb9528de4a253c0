// pileup_kernels.hip — allele counts at listed sites on the device (gfx950): what the reads of a run show at every site of
// a site list (include/simmr_hip.h states the site list, the observed class and counts[n][2][5]).  Included by pileup.hip
// alone, the library's fifth translation unit: nothing here is seen by the other units, whose kernel budgets stay what
// they were.
//
// Two kernels.
//   k_pileup_keys  one lane per site: the site's 64-bit key first(slot, contig) + pos in the dense layout of depth[], after
//                  the checks that make a key an address — slot staged, contig there, pos < len — and the neighbour check
//                  key[s] > key[s - 1] (a lane makes its left neighbour's key itself, so no lane waits for another).  The
//                  first bad index leaves through an atomic minimum.
//   k_pileup_add   the work is the (read, site) PAIRS, and a read has between none and hundreds of them.  A wave takes 64
//                  consecutive reads: each lane checks its read and bisects the keys twice (the lower bounds of the read's
//                  first position and of the one behind its last), which gives the read's first site and its count; the
//                  wave scans the 64 counts (the DPP row ladder and the two row broadcasts) and then takes the pairs 64 at
//                  a time.  Lane t of step k owns pair 64 k + t: it finds the pair's read by a six-step search over the 64
//                  prefixes through ds_bpermute (no LDS array, no barrier: the waves are independent), fetches that read's
//                  first site and byte address the same way, loads the site's key and ONE byte of seq[], classifies and
//                  complements it, and adds 1 to counts[s][strand][class] with a no-return relaxed agent-scope atomic.
//                  Persistent grid of at most PILEUP_WGS_PER_CU workgroups per CU: a wave loops over its share of the 64-read
//                  batches.
// Tried: this form only.  One lane walking its own read's sites serialises a 20 kb read's 200 sites behind one lane; a
// site-major pass needs the reads sorted by position; counts privatised in LDS per tile of sites only pay at depths where
// same-address atomics dominate (DESIGN.md section 4 says what was weighed and has the measured times).
//
// What bounds a 32-bit count: fewer than 2^31 reads are added between two resets (simmr_pileup_add refuses more), and a read
// adds at most 1 to a site.  A lane hands at most PILEUP_ROUND pairs to one scan, so a wave's prefix stays below 2^31
// whatever the reads' lengths; a read with more sites than that takes further rounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"

namespace simmr {

constexpr uint32_t PILEUP_WG = 256;             // threads of every workgroup here: four independent waves
constexpr uint32_t PILEUP_ROUND = 1u << 24;     // pairs a lane hands to one scan: 64 of them stay below 2^31
constexpr uint32_t PILEUP_CELLS = 10;           // uint32_t counts per site: [strand][class]
constexpr uint32_t PILEUP_WGS_PER_CU = 8;       // the add's grid is capped at this many workgroups per CU; beyond it waves loop

#define PILEUP_DEV __device__ __forceinline__

// a genome slot of the layout a reset recorded: its contigs are cfirst[cbase .. cbase + n_contigs]; n_contigs == 0: not tracked
struct PileupSlot {
  uint32_t cbase, n_contigs;
};

// the columns the add reads (qual is not among them)
struct PileupReads {
  const uint8_t* seq;
  const uint64_t* seq_off;
  const uint64_t* start;
  const uint64_t* end;
  const uint32_t* contig;
  const uint32_t* genome;
  const uint8_t* flags;
  uint64_t seq_capacity;
};

// inclusive scan over the wave: four DPP row shifts, then row_bcast:15 and row_bcast:31 (GFX9) — depth_kernels.hip's ladder,
// restated because including that file would bring its kernels into this unit's budget
PILEUP_DEV uint32_t pileup_wave_scan(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
  return v;
}
// lane `from`'s value (every lane of the wave is active where these are called)
PILEUP_DEV uint32_t pileup_from(uint32_t v, uint32_t from) { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(from << 2), (int)v); }
PILEUP_DEV uint64_t pileup_from64(uint64_t v, uint32_t from) {
  return (uint64_t)pileup_from((uint32_t)v, from) | (uint64_t)pileup_from((uint32_t)(v >> 32), from) << 32;
}

// where contig c of slot g lies in the dense layout, after the checks: false leaves *first and *len alone
PILEUP_DEV bool pileup_contig(const PileupSlot* __restrict__ slots, uint32_t n_slots, const uint64_t* __restrict__ cfirst, uint32_t g,
                              uint32_t c, uint64_t* first, uint64_t* len) {
  PileupSlot s{0u, 0u};
  if (g < n_slots) s = slots[g];
  if (c >= s.n_contigs) return false;
  *first = cfirst[s.cbase + c];
  *len = cfirst[s.cbase + c + 1u] - *first;
  return true;
}

// ---- keys -----------------------------------------------------------------------------------------------------------
PILEUP_DEV bool pileup_site_key(const uint32_t* __restrict__ genome, const uint32_t* __restrict__ contig, const uint64_t* __restrict__ pos,
                                uint64_t s, const PileupSlot* __restrict__ slots, uint32_t n_slots, const uint64_t* __restrict__ cfirst,
                                uint64_t* key) {
  uint64_t first = 0, len = 0;
  const uint64_t p = pos[s];
  if (!pileup_contig(slots, n_slots, cfirst, genome[s], contig[s], &first, &len) || p >= len) return false;
  *key = first + p;
  return true;
}

// bad[0] starts at all ones and receives the smallest index of a site that fails a check.  A site behind a failing one is
// compared with nothing: its neighbour reports itself.
extern "C" __global__ void __launch_bounds__(PILEUP_WG)
k_pileup_keys(const uint32_t* __restrict__ genome, const uint32_t* __restrict__ contig, const uint64_t* __restrict__ pos, uint64_t n,
              const PileupSlot* __restrict__ slots, uint32_t n_slots, const uint64_t* __restrict__ cfirst, uint64_t* __restrict__ keys,
              unsigned long long* __restrict__ bad) {
  const uint64_t s = (uint64_t)blockIdx.x * PILEUP_WG + threadIdx.x;
  if (s >= n) return;
  uint64_t key = 0, left = 0;
  bool ok = pileup_site_key(genome, contig, pos, s, slots, n_slots, cfirst, &key);
  if (ok && s > 0 && pileup_site_key(genome, contig, pos, s - 1, slots, n_slots, cfirst, &left)) ok = key > left;
  keys[s] = key;
  if (!ok) atomicMin(bad, (unsigned long long)s);
}

// ---- add ------------------------------------------------------------------------------------------------------------
// the first index in [lo, hi) whose key is not below k, or hi
PILEUP_DEV uint64_t pileup_lower_bound(const uint64_t* __restrict__ keys, uint64_t lo, uint64_t hi, uint64_t k) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The bounds check comes before any address is formed from the read: slot tracked, contig there, the window inside its
// contig, the read's bytes inside seq[0 .. seq_capacity).  A read that fails it sets the error word and has no pairs.
// All indices are 64-bit wherever n_positions, n or seq_off enter.
extern "C" __global__ void __launch_bounds__(PILEUP_WG)
k_pileup_add(const PileupReads rd, uint64_t n_reads, const PileupSlot* __restrict__ slots, uint32_t n_slots,
             const uint64_t* __restrict__ cfirst, const uint64_t* __restrict__ keys, uint64_t n, uint32_t* __restrict__ counts,
             uint32_t* __restrict__ err) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t n_waves = (uint64_t)gridDim.x * (PILEUP_WG / 64u);
  const uint64_t gw = (uint64_t)blockIdx.x * (PILEUP_WG / 64u) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t n_batches = (n_reads + 63u) / 64u;
  for (uint64_t b = gw; b < n_batches; b += n_waves) {  // (uniform over the wave: every lane stays in the loop)
    // ---- per-read bisections: s0 = the read's first site, rem = how many it covers; at = what turns a site's key into the
    // address of the read's byte there: so + (key - klo) forward, so + L - 1 - (key - klo) reverse
    const uint64_t r = b * 64u + lane;
    uint64_t s0 = 0, rem = 0, at = 0;
    uint32_t rev = 0;
    if (r < n_reads) {
      const uint64_t a = rd.start[r], e = rd.end[r], so = rd.seq_off[r];
      const uint64_t lo = a < e ? a : e, L = a < e ? e - a : a - e;
      uint64_t first = 0, len = 0;
      bool ok = pileup_contig(slots, n_slots, cfirst, rd.genome[r], rd.contig[r], &first, &len);
      ok = ok && lo <= len && L <= len - lo && so <= rd.seq_capacity && L <= rd.seq_capacity - so;
      if (!ok) {
        atomicOr(err, 1u);
      } else if (L > 0) {
        rev = rd.flags[r] & SIMMR_FLAG_REVCOMP;
        const uint64_t klo = first + lo;
        s0 = pileup_lower_bound(keys, 0, n, klo);
        const uint64_t reach = n - s0 < L ? n : s0 + L;  // (keys ascend strictly: L positions hold at most L sites)
        rem = pileup_lower_bound(keys, s0, reach, klo + L) - s0;
        at = rev ? so + (L - 1u) + klo : so - klo;
      }
    }
    // ---- rounds: one for every read the library writes (a read of 2^24 sites or more takes another)
    while (__builtin_amdgcn_ballot_w64(rem != 0) != 0) {
      const uint32_t c = rem < PILEUP_ROUND ? (uint32_t)rem : PILEUP_ROUND;
      const uint32_t inc = pileup_wave_scan(c), excl = inc - c;
      const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
      const uint32_t tag = excl | rev << 31;
      // ---- pair expansion: lane t of a step owns pair q = q0 + t of the wave's `total`
      for (uint32_t q0 = 0; q0 < total; q0 += 64u) {
        const uint32_t q = q0 + lane;
        uint32_t i = 0;  // the last lane whose exclusive prefix is not above q: the pair's read (lanes without pairs share
                         // their right neighbour's prefix, so the last one is the one that has them)
#pragma unroll
        for (uint32_t bit = 32u; bit > 0; bit >>= 1)
          if (pileup_from(excl, i + bit) <= q) i += bit;
        const uint32_t t = pileup_from(tag, i);
        const uint64_t s = pileup_from64(s0, i) + (q - (t & 0x7fffffffu));
        const uint64_t base = pileup_from64(at, i);
        if (q < total) {
          const uint64_t key = keys[s];
          const uint32_t strand = t >> 31;
          const uint8_t byte = rd.seq[strand ? base - key : base + key];
          uint32_t cls = byte == 'A' ? 0u : byte == 'C' ? 1u : byte == 'G' ? 2u : byte == 'T' ? 3u : 4u;
          if (strand && cls < 4u) cls = 3u - cls;  // observed in genome orientation
          (void)__hip_atomic_fetch_add(counts + s * PILEUP_CELLS + strand * 5u + cls, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      rem -= c;
      s0 += c;
    }
  }
}

}  // namespace simmr
