// read_walk.hpp — what a kernel needs to walk reads against the staged planes: the plane routines (fetch_codes16 ..
// expand4, gather_piece: the emit kernels' funnel-shift addressing and code-domain reverse complement) and the read walker
// (walk_open / walk_window) that k_truth, k_read_stats and k_fit_add share, and the scan over a row of 16 lanes that the kernels
// with a row per read use.  Plain device routines, no kernel: a translation unit that includes this file keeps its own kernel
// budget (kernels.hip, truth_kernels.hip and fit_kernels.hip include it, and none of them sees another's kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.hpp"

namespace simmr {

#ifndef SIMMR_DEV
#define SIMMR_DEV __device__ __forceinline__
#endif

// ---- the planes ------------------------------------------------------------------------------------------------------

// 16 bases (32 bits of codes) starting at absolute base position p (may be
// slightly negative: the plane has front padding).
// The planes live in device memory: say so (a pointer that came out of a struct or out of LDS is a
// generic pointer, and a flat load is slower than a global one).
typedef uint64_t __attribute__((aligned(1))) u64_unaligned;
typedef uint32_t v4u32 __attribute__((ext_vector_type(4)));
typedef v4u32 __attribute__((aligned(1))) v4u32_unaligned;
typedef const __attribute__((address_space(1))) u64_unaligned* global_u64_unaligned_ptr;
SIMMR_DEV uint64_t load_plane_u64(const uint32_t* __restrict__ plane, int64_t word) {
  return *(global_u64_unaligned_ptr)(plane + word);  // words `word` and `word + 1`, 4-byte aligned
}
SIMMR_DEV uint32_t fetch_codes16(const uint32_t* __restrict__ packed, int64_t p) {
  return (uint32_t)(load_plane_u64(packed, p >> 4) >> ((uint32_t)(p & 15) * 2u));
}
SIMMR_DEV uint32_t fetch_mask16(const uint32_t* __restrict__ mask, int64_t p) {
  return (uint32_t)(load_plane_u64(mask, p >> 5) >> (uint32_t)(p & 31)) & 0xffffu;
}
// reverse the order of the sixteen 2-bit groups
SIMMR_DEV uint32_t reverse_groups16(uint32_t x) {
  const uint32_t y = __builtin_bitreverse32(x);
  // each bit pair swapped back: odd result bits from y << 1, even ones from y >> 1 — one three-input select (v_bitop3_b32,
  // truth table of c ? a : b with a = y >> 1, b = y << 1, c = 0x55555555)
  return __builtin_amdgcn_bitop3_b32(y >> 1, y << 1, 0x55555555u, 0xe4);
}
// ~reverse_groups16(x): the complement folded into the select's truth table
SIMMR_DEV uint32_t reverse_complement_groups16(uint32_t x) {
  const uint32_t y = __builtin_bitreverse32(x);
  return __builtin_amdgcn_bitop3_b32(y >> 1, y << 1, 0x55555555u, 0x1b);
}
// low bit of each of the sixteen 2-bit codes -> 16 bits
SIMMR_DEV uint32_t c16_odd(uint32_t c) {
  c &= 0x55555555u;
  c = (c | (c >> 1)) & 0x33333333u;
  c = (c | (c >> 2)) & 0x0F0F0F0Fu;
  c = (c | (c >> 4)) & 0x00FF00FFu;
  c = (c | (c >> 8)) & 0x0000FFFFu;
  return c;
}
// 16 mask bits -> 16 two-bit groups (each bit duplicated)
SIMMR_DEV uint32_t spread16(uint32_t m) {
  m = (m | (m << 8)) & 0x00FF00FFu;
  m = (m | (m << 4)) & 0x0F0F0F0Fu;
  m = (m | (m << 2)) & 0x33333333u;
  m = (m | (m << 1)) & 0x55555555u;
  return m * 3u;
}
// 4 codes (8 bits) + 4 exception bits -> 4 ASCII bytes
SIMMR_DEV uint32_t expand4(uint32_t c8, uint32_t m4) {
  uint32_t sel = (c8 | (c8 << 6) | (c8 << 12) | (c8 << 18)) & 0x03030303u;
  uint32_t ms = (m4 | (m4 << 7) | (m4 << 14) | (m4 << 21)) & 0x01010101u;
  sel |= ms << 2;
  // selector 0-3 -> "ACGT" (src1), 4-7 -> "N-N-" (src0)
  return __builtin_amdgcn_perm(0x2D4E2D4Eu, 0x54474341u, sel);
}

struct PieceSrc {
  int64_t pos;   // absolute base position of output byte 0's source
  uint32_t rev;  // mate 2: byte k comes from pos - k, complemented
};

SIMMR_DEV void gather_piece(const GenomeDev& G, const PieceSrc& s, uint32_t k, uint32_t& codes,
                            uint32_t& exc) {
  // codes for output bytes k .. k+15 of this read (garbage past the read end)
  if (!s.rev) {
    int64_t p = s.pos + (int64_t)k;
    codes = fetch_codes16(G.packed, p);
    exc = G.has_exc ? fetch_mask16(G.mask, p) : 0u;
  } else {
    int64_t p = s.pos - (int64_t)k - 15;
    uint32_t c = fetch_codes16(G.packed, p);
    codes = ~reverse_groups16(c);  // complement = 3 - code
    if (G.has_exc) {
      uint32_t m = fetch_mask16(G.mask, p);
      exc = __builtin_bitreverse32(m) >> 16;
      codes ^= spread16(exc);  // exceptions ('N', '-') are their own complement
    } else {
      exc = 0u;
    }
  }
}

struct TruthReads {
  const uint8_t* seq;
  const uint8_t* qual;
  const uint64_t* seq_off;
  const uint64_t* start;
  const uint64_t* end;
  const uint32_t* contig;
  const uint32_t* genome;
  const uint8_t* flags;
  uint64_t seq_capacity;
  uint32_t slot16;
};

typedef const __attribute__((address_space(1))) v4u32_unaligned* global_v4u32_unaligned_ptr;

// bit i = byte i of x is not zero
SIMMR_DEV uint32_t truth_nonzero_bytes(uint32_t x) {
  const uint32_t t = ((x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u) >> 7;
  return (t | (t >> 7) | (t >> 14) | (t >> 21)) & 0xfu;
}

// ---- the read walker: shared by k_truth and k_read_stats (stats_kernels.hip) ----------------------------------------
// Sixteen lanes (one DPP row) share a read.  walk_open checks a row's read once, walk_window loads one lane's 16 bases
// of it; between them they hold every rule that keeps a load inside the read, so both kernels answer to one copy.

// A row's read, opened: L bases of seq[] from byte `so`; output byte k is the reference's pos0 + k (forward) or pos0 - k,
// complemented (reverse): gather_piece.  A refused read, and a row past n_reads, has L = 0 and good = false.
struct ReadWalk {
  uint32_t L, rev;
  uint64_t so;
  int64_t pos0;
  GenomeDev G;
  bool good;
};
// The bounds check: genome staged, contig in range, so <= so1 <= seq_capacity, len <= so1 - so and MAX_L, coordinates
// inside the contig.  Every lane of a row reads the same columns (one address per row) and so takes the same branch:
// all-or-nothing per row, which keeps the DPP rows whole.  A refused read raises the caller's `errbit` in the caller's
// error word `err`, through the one lane of its row that has `raise` set.  (The atomic sits where the read is refused:
// raised by the caller after the checks have joined again, both kernels measured slower.)
template <uint64_t MAX_L>
SIMMR_DEV ReadWalk walk_open(const GenomeDev* __restrict__ genomes, uint32_t n_genomes, const TruthReads& rd, uint64_t r,
                             uint64_t n_reads, uint32_t* __restrict__ err, uint32_t errbit, bool raise) {
  uint32_t L = 0, rev = 0;
  uint64_t so = 0;
  int64_t pos0 = 0;
  bool good = false;
  GenomeDev G{};
  if (r < n_reads) {
    const uint64_t a = rd.start[r], b = rd.end[r];
    const uint64_t lo = a < b ? a : b, len = a < b ? b - a : a - b;
    const uint32_t g = rd.genome[r], c = rd.contig[r];
    so = rd.seq_off[r];
    const uint64_t so1 = rd.seq_off[r + 1];
    rev = rd.flags[r] & SIMMR_FLAG_REVCOMP;
    bool ok = g < n_genomes && len <= MAX_L && so <= so1 && so1 <= rd.seq_capacity && len <= so1 - so;
    if (ok) {
      G = genomes[g];
      ok = G.packed != nullptr && c < G.n_contigs;
    }
    if (ok) {
      const ContigDev C = G.contigs[c];
      ok = lo <= C.len && len <= C.len - lo;
      L = (uint32_t)len;
      pos0 = (int64_t)(C.base + lo) + (rev ? (int64_t)len - 1 : 0);
    }
    good = ok;
    if (!ok) {
      L = 0;
      if (raise) atomicOr(err, errbit);
    }
  }
  return ReadWalk{L, rev, so, pos0, G, good};
}

// Group `grp` (< ceil(L / 16)) of an opened read: bit b of keep = byte b of the window is base k + b and belongs to this
// group; have / qv = the 16 bytes of seq[] / qual[] (qv only with QUAL), want = what the reference holds there, diff =
// the kept bytes where they differ.
struct ReadWindow {
  uint32_t k, keep, diff;
  v4u32 have, qv, want;
};
template <bool QUAL>
SIMMR_DEV ReadWindow walk_window(const ReadWalk& w, uint32_t grp, const uint8_t* seq, const uint8_t* qual) {
  ReadWindow o{};
  const uint32_t k16 = grp * 16u, L = w.L;
  if (L >= 16u) {
    o.k = k16 + 16u <= L ? k16 : L - 16u;         // the last window ends at the read's end
    o.keep = (0xffffu << (k16 - o.k)) & 0xffffu;  // ... and owns only the bases no earlier window had
    o.have = __builtin_nontemporal_load((global_v4u32_unaligned_ptr)(seq + o.k));
    if (QUAL) o.qv = __builtin_nontemporal_load((global_v4u32_unaligned_ptr)(qual + o.k));
  } else {
    uint32_t h[4] = {0u, 0u, 0u, 0u}, q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++)
      if (j < L) {
        h[j >> 2] |= (uint32_t)seq[j] << ((j & 3u) * 8u);
        if (QUAL) q[j >> 2] |= (uint32_t)qual[j] << ((j & 3u) * 8u);
      }
    o.have = v4u32{h[0], h[1], h[2], h[3]};
    o.qv = v4u32{q[0], q[1], q[2], q[3]};
    o.keep = (1u << L) - 1u;
  }
  uint32_t codes, exc;
  gather_piece(w.G, PieceSrc{w.pos0, w.rev}, o.k, codes, exc);
  o.want = v4u32{expand4(codes & 0xffu, exc & 0xfu), expand4((codes >> 8) & 0xffu, (exc >> 4) & 0xfu),
                 expand4((codes >> 16) & 0xffu, (exc >> 8) & 0xfu), expand4(codes >> 24, (exc >> 12) & 0xfu)};
  o.diff = (truth_nonzero_bytes(o.have.x ^ o.want.x) | truth_nonzero_bytes(o.have.y ^ o.want.y) << 4 |
            truth_nonzero_bytes(o.have.z ^ o.want.z) << 8 | truth_nonzero_bytes(o.have.w ^ o.want.w) << 12) & o.keep;
  return o;
}

// ---- a row of 16 lanes -------------------------------------------------------------------------------------------

// inclusive scan of one u32 over each row of 16 lanes (every lane of the row active): four DPP row shifts, one v_add
// with a DPP source each.  The row's last lane holds the row's sum.
SIMMR_DEV uint32_t row_inclusive_scan_u32(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
  return v;
}

}  // namespace simmr
