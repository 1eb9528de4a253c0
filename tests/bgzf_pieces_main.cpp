// bgzf_pieces_main.cpp — BgzfPieces of simmr_amd/host/simmr_host.hpp in a stand-alone program, for a build under the sanitizers
// (tests/test_bai_host.py).  Input: the number of cases, then per case the blocks of a piece, the number of appends and their
// sizes.  Byte i of a case's input is (131 i + 7) & 0xff.  Output per case: the sizes of the pieces the framing callback got.
// The program checks itself that every piece but the last is a whole piece, and that the pieces end to end are the input.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../simmr_amd/host/simmr_host.hpp"

using simmr_host::BgzfPieces;

int main() {
  int n_cases = 0;
  if (scanf("%d", &n_cases) != 1) return 2;
  for (int c = 0; c < n_cases; c++) {
    unsigned long blocks = 0, n_appends = 0;
    if (scanf("%lu %lu", &blocks, &n_appends) != 2) return 2;
    std::vector<size_t> got_sizes;
    std::vector<uint8_t> got;
    BgzfPieces pieces(blocks, [&](const uint8_t* p, size_t n) {
      got_sizes.push_back(n);
      got.insert(got.end(), p, p + n);
      return true;
    });
    uint64_t at = 0;
    for (unsigned long k = 0; k < n_appends; k++) {
      unsigned long size = 0;
      if (scanf("%lu", &size) != 1) return 2;
      std::vector<uint8_t> src(size);
      for (size_t i = 0; i < size; i++) src[i] = (uint8_t)((131u * (at + i) + 7u) & 0xffu);
      if (!pieces.append(src.data(), size)) return 3;
      at += size;
    }
    if (!pieces.finish() || pieces.bytes() != at || got.size() != at) return 4;
    for (size_t i = 0; i < got.size(); i++)
      if (got[i] != (uint8_t)((131u * i + 7u) & 0xffu)) return 5;
    for (size_t k = 0; k + 1 < got_sizes.size(); k++)
      if (got_sizes[k] != blocks * BgzfPieces::BLOCK) return 6;
    if (!got_sizes.empty() && (got_sizes.back() == 0 || got_sizes.back() > blocks * BgzfPieces::BLOCK)) return 7;
    for (size_t k = 0; k < got_sizes.size(); k++) printf("%s%zu", k ? " " : "", got_sizes[k]);
    printf("\n");
  }
  return 0;
}
