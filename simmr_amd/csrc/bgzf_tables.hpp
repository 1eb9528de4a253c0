// bgzf_tables.hpp — the host's side of k_bgzf_frame's CRC-32 (bam_kernels.hip): the four byte tables, the multipliers that
// shift a CRC register by whole segments and by the bytes of a short block's last segment, and a plain restatement of the
// kernel's fold, lane by lane, for a CPU to run.  Plain C++ without HIP: bam.hip makes the tables once per engine, and a
// stand-alone program (tests/bgzf_fold_main.cpp) checks tables and fold against zlib's CRC under the sanitizers.
//
// zlib's CRC-32: polynomial 0xEDB88320 (bit-reflected: bit 31 of a word is x^0), start value and final xor 0xffffffff.  The
// register after `data` from start value s is linear in (s, data), so for data = A B
//   reg(s, A B) = reg(s, A) x^(8 |B|) + reg(0, B)   (mod P),
// which is all the fold uses: a lane's register times x^(8 * bytes behind its segment), summed.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace simmr {
namespace bgzf {

constexpr uint32_t POLY = 0xEDB88320u;
constexpr uint32_t SEG = 256u, LANES = 256u, BLOCK = 65280u;  // BGZF_SEG, BGZF_LANES, BGZF_BLOCK of bam_kernels.hip
static_assert(BLOCK == (LANES - 1u) * SEG, "255 lanes take a whole block");

struct Tables {
  uint32_t crc[4 * 256];        // crc[256 k + b]: the register after byte b and k zero bytes, from 0
  uint32_t seg_mul[LANES - 1];  // seg_mul[j] = x^(8 SEG j) mod P
  uint32_t rem_mul[SEG];        // rem_mul[k] = x^(8 k) mod P
};

// a(x) b(x) mod P
inline uint32_t mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t i = 0; i < 32u; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? POLY : 0u);
  }
  return p;
}
// x^(8 k) mod P, by squaring
inline uint32_t xpow8(uint64_t k) {
  uint32_t r = 0x80000000u, sq = 0x00800000u;  // x^0, x^8
  for (; k; k >>= 1) {
    if (k & 1u) r = mulmod(r, sq);
    sq = mulmod(sq, sq);
  }
  return r;
}

inline void make_tables(Tables* t) {
  for (uint32_t b = 0; b < 256u; b++) {
    uint32_t c = b;
    for (int i = 0; i < 8; i++) c = (c >> 1) ^ ((c & 1u) ? POLY : 0u);
    t->crc[b] = c;
  }
  for (uint32_t k = 1; k < 4u; k++)
    for (uint32_t b = 0; b < 256u; b++) {
      const uint32_t c = t->crc[256u * (k - 1u) + b];
      t->crc[256u * k + b] = t->crc[c & 0xffu] ^ (c >> 8);
    }
  for (uint32_t j = 0; j < LANES - 1u; j++) t->seg_mul[j] = xpow8((uint64_t)SEG * j);
  for (uint32_t k = 0; k < SEG; k++) t->rem_mul[k] = xpow8(k);
}

// The CRC-32 of the n (1 .. BLOCK) bytes of a block as the workgroup of k_bgzf_frame computes it: a register per lane over its
// segment (16 bytes at a time through the four tables, then bytewise), lane 0 from the start value, then the fold.
inline uint32_t fold_block(const Tables& t, const uint8_t* p, uint32_t n) {
  const uint32_t n_full = n / SEG, rem = n % SEG;
  uint32_t sum = 0, last = 0;
  for (uint32_t lane = 0; lane < LANES; lane++) {
    const uint32_t seg0 = lane * SEG;
    const uint32_t mine = seg0 >= n ? 0u : (n - seg0 < SEG ? n - seg0 : SEG);
    uint32_t c = lane == 0u ? 0xffffffffu : 0u, i = 0;
    for (; i + 16u <= mine; i += 16u)
      for (uint32_t w = 0; w < 4u; w++) {
        const uint8_t* q = p + seg0 + i + 4u * w;
        c ^= (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
        c = t.crc[768u + (c & 0xffu)] ^ t.crc[512u + ((c >> 8) & 0xffu)] ^ t.crc[256u + ((c >> 16) & 0xffu)] ^ t.crc[c >> 24];
      }
    for (; i < mine; i++) c = t.crc[(c ^ p[seg0 + i]) & 0xffu] ^ (c >> 8);
    if (lane < n_full) sum ^= mulmod(t.seg_mul[n_full - 1u - lane], c);
    if (lane == n_full) last = c;
  }
  if (rem) sum = mulmod(t.rem_mul[rem], sum) ^ last;
  return ~sum;
}

}  // namespace bgzf
}  // namespace simmr
