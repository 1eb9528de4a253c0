// A stand-alone driver of sam_merge_sorted_runs (simmr_amd/host/host.cpp) for tests/test_sam_sort_host.py, which builds it
// with -fsanitize=address,undefined and runs it as a child process.  Input on stdin: the number of runs; per run its number of
// lines, then per line "<key> <text without spaces>".  A run's text is its lines, each ended by '\n'; the runs lie back to back
// in the source.  Output: the merged bytes.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

#include "../simmr_amd/host/simmr_host.hpp"

int main() {
  using namespace simmr_host;
  size_t n_runs = 0;
  std::cin >> n_runs;
  std::vector<SamSortedRun> runs(n_runs);
  std::string src;
  for (SamSortedRun& run : runs) {
    size_t n = 0;
    std::cin >> n;
    run.offset = src.size();
    for (size_t i = 0; i < n; i++) {
      uint64_t key;
      std::string text;
      std::cin >> key >> text;
      run.key.push_back(key);
      run.len.push_back(text.size() + 1);
      src += text + "\n";
    }
  }
  if (!std::cin) return 2;
  const bool ok = sam_merge_sorted_runs(
      runs,
      [&](uint64_t at, size_t n, char* p) { if (at + n > src.size()) return false; memcpy(p, src.data() + at, n); return true; },
      [&](const char* p, size_t n) { return fwrite(p, 1, n, stdout) == n; });
  return ok ? 0 : 1;
}
