// mapeval_report_main.cpp — the report formatter, the rows of --eval-reads and the @SQ reader of simmr_amd/host/host.cpp in a
// stand-alone program, for a build under the sanitizers (tests/test_mapeval_host.py).  Input, a command a block:
//   sq <n_bytes>\n<bytes>            -> "names <k>" and the k names, one a line
//   report\n<19 counts>\n<k> then k rows "<mapq> <correct> <wrong>"   -> the report
//   reads <n>\n then n rows "<key> <best> <hits>"                     -> the rows
// Every answer ends with a line "--".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../simmr_amd/host/simmr_host.hpp"

int main() {
  char cmd[16];
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "sq")) {
      unsigned long n = 0;
      if (scanf("%lu", &n) != 1 || getchar() != '\n') return 2;
      std::vector<char> text(n);  // exactly n bytes: a read past the end is the sanitizer's to find
      if (n && fread(text.data(), 1, n, stdin) != n) return 2;
      std::vector<std::string> names;
      simmr_host::mapeval_sq_names(text.data(), n, &names);
      printf("names %zu\n", names.size());
      for (const std::string& s : names) printf("%s\n", s.c_str());
    } else if (!strcmp(cmd, "report")) {
      std::vector<uint64_t> counts(simmr_host::MAPEVAL_N_COUNTS), by(512, 0);
      for (uint64_t& c : counts) {
        unsigned long long v;
        if (scanf("%llu", &v) != 1) return 2;
        c = v;
      }
      unsigned long k = 0;
      if (scanf("%lu", &k) != 1) return 2;
      for (unsigned long i = 0; i < k; i++) {
        unsigned long q;
        unsigned long long ok, wrong;
        if (scanf("%lu %llu %llu", &q, &ok, &wrong) != 3 || q > 255) return 2;
        by[2 * q] = ok;
        by[2 * q + 1] = wrong;
      }
      fputs(simmr_host::mapeval_report(counts.data(), by.data()).c_str(), stdout);
    } else if (!strcmp(cmd, "reads")) {
      unsigned long n = 0;
      if (scanf("%lu", &n) != 1) return 2;
      std::vector<uint64_t> key(n);
      std::vector<uint32_t> best(n), hits(n);
      for (unsigned long i = 0; i < n; i++) {
        unsigned long long k;
        unsigned b, h;
        if (scanf("%llu %u %u", &k, &b, &h) != 3) return 2;
        key[i] = k; best[i] = b; hits[i] = h;
      }
      fputs(simmr_host::mapeval_read_rows(key.data(), best.data(), hits.data(), n).c_str(), stdout);
    } else {
      return 3;
    }
    printf("--\n");
  }
  return 0;
}
