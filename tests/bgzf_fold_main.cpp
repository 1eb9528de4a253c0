// The host tables of the BGZF CRC (simmr_amd/csrc/bgzf_tables.hpp) and the CPU restatement of k_bgzf_frame's fold, as a program of
// its own for tests/test_bam_host.py to build with -fsanitize=address,undefined.  Reads from stdin: a count, then per case a
// pattern (0: bytes 0, 1: bytes 0xff, 2: byte i = (131 i + 7 + 29 (i >> 8)) & 0xff) and a length of 1 .. 65280; writes the
// CRC-32 of each as eight hex digits.  Before that it checks the multipliers against the byte table: x^(8k) times a register
// is that register after k zero bytes.
#include <stdio.h>

#include <memory>
#include <vector>

#include "../simmr_amd/csrc/bgzf_tables.hpp"

using namespace simmr::bgzf;

int main() {
  auto t = std::make_unique<Tables>();
  make_tables(t.get());
  const uint32_t starts[3] = {0xffffffffu, 0x12345678u, 1u};
  for (uint32_t s : starts) {
    uint32_t c = s;
    for (uint32_t k = 0; k < SEG * 3u + 5u; k++) {
      if (k < SEG && mulmod(t->rem_mul[k], s) != c) { fprintf(stderr, "rem_mul[%u] is wrong\n", k); return 1; }
      if (k % SEG == 0 && mulmod(t->seg_mul[k / SEG], s) != c) { fprintf(stderr, "seg_mul[%u] is wrong\n", k / SEG); return 1; }
      c = t->crc[c & 0xffu] ^ (c >> 8);  // a zero byte
    }
  }
  if (mulmod(t->seg_mul[LANES - 2u], 0x80000000u) != xpow8((uint64_t)SEG * (LANES - 2u))) { fprintf(stderr, "the last multiplier is wrong\n"); return 1; }
  unsigned n_cases = 0;
  if (scanf("%u", &n_cases) != 1) return 2;
  for (unsigned k = 0; k < n_cases; k++) {
    unsigned pattern = 0, n = 0;
    if (scanf("%u %u", &pattern, &n) != 2 || n < 1 || n > BLOCK || pattern > 2) return 2;
    std::vector<uint8_t> data(n);  // (exactly n bytes: a load past them is the sanitizer's to find)
    for (unsigned i = 0; i < n; i++) data[i] = pattern == 0 ? 0u : pattern == 1 ? 0xffu : (uint8_t)(131u * i + 7u + 29u * (i >> 8));
    printf("%08x\n", fold_block(*t, data.data(), n));
  }
  return 0;
}
