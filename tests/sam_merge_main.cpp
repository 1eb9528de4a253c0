// A stand-alone driver of sam_merge_sorted_runs (simmr_amd/host/host.cpp) for tests/test_sam_sort_host.py, which builds it
// with -fsanitize=address,undefined and runs it as a child process.  Input on stdin: the number of runs; per run its number of
// lines, then per line "<key> <text without spaces>".  A run's text is its lines, each ended by '\n'; the runs lie back to back
// in the source.  Output: the merged bytes.
// With the arguments `spill <out> [<k>]` the runs go through SortedRunSpill (simmr_host.hpp) for the output file <out> instead:
// added one by one, then merged to stdout by a sink that refuses its k-th call (k from 1; none without k).  Status 3: the
// temporary file <out>.sorting.tmp exists although there is one run at most, or is missing although there are several.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

#include <sys/stat.h>

#include "../simmr_amd/host/simmr_host.hpp"

int main(int argc, char** argv) {
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
  if (argc >= 3 && std::string(argv[1]) == "spill") {
    const long refuse = argc >= 4 ? atol(argv[3]) : 0;
    long calls = 0;
    std::string err;
    SortedRunSpill spill(argv[2]);
    for (size_t k = 0; k < n_runs; k++) {
      const size_t end = k + 1 < n_runs ? (size_t)runs[k + 1].offset : src.size();
      std::vector<uint8_t> bytes(src.begin() + (size_t)runs[k].offset, src.begin() + end);
      SamSortedRun run = runs[k];
      run.offset = 0;  // (the spill gives a run its place)
      if (!spill.add(std::move(run), std::move(bytes), &err)) return 1;
    }
    struct stat st;
    const bool on_disk = stat((std::string(argv[2]) + ".sorting.tmp").c_str(), &st) == 0;
    if (on_disk != (n_runs > 1) || spill.spilled() != on_disk || spill.runs().size() != n_runs) return 3;
    return spill.merge([&](const char* p, size_t n) { return ++calls != refuse && fwrite(p, 1, n, stdout) == n; }, &err) ? 0 : 1;
  }
  const bool ok = sam_merge_sorted_runs(
      runs,
      [&](uint64_t at, size_t n, char* p) { if (at + n > src.size()) return false; memcpy(p, src.data() + at, n); return true; },
      [&](const char* p, size_t n) { return fwrite(p, 1, n, stdout) == n; });
  return ok ? 0 : 1;
}
