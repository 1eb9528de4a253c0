// ovleval_report_main.cpp — the report formatter and the rows of --eval-overlaps-pairs of simmr_amd/host/host.cpp in a stand-alone
// program, for a build under the sanitizers (tests/test_ovleval_host.py).  Input, a command a block:
//   report\n<16 counts>\n<k> then k rows "<bits> <found> <not found>"   -> the report
//   pairs <n>\n then n rows "<key_a> <key_b> <ov> <best> <hits>"        -> the rows
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
    if (!strcmp(cmd, "report")) {
      std::vector<uint64_t> counts(simmr_host::OVLEVAL_N_COUNTS), by(2 * simmr_host::OVLEVAL_LEN_ROWS, 0);  // exactly the sizes the formatter may read
      for (uint64_t& c : counts) {
        unsigned long long v;
        if (scanf("%llu", &v) != 1) return 2;
        c = v;
      }
      unsigned long k = 0;
      if (scanf("%lu", &k) != 1) return 2;
      for (unsigned long i = 0; i < k; i++) {
        unsigned long b;
        unsigned long long found, not_found;
        if (scanf("%lu %llu %llu", &b, &found, &not_found) != 3 || b >= simmr_host::OVLEVAL_LEN_ROWS) return 2;
        by[2 * b] = found;
        by[2 * b + 1] = not_found;
      }
      fputs(simmr_host::ovleval_report(counts.data(), by.data()).c_str(), stdout);
    } else if (!strcmp(cmd, "pairs")) {
      unsigned long n = 0;
      if (scanf("%lu", &n) != 1) return 2;
      std::vector<uint64_t> ka(n), kb(n), ov(n);
      std::vector<uint32_t> best(n), hits(n);
      for (unsigned long i = 0; i < n; i++) {
        unsigned long long a, b, o;
        unsigned x, h;
        if (scanf("%llu %llu %llu %u %u", &a, &b, &o, &x, &h) != 5) return 2;
        ka[i] = a; kb[i] = b; ov[i] = o; best[i] = x; hits[i] = h;
      }
      fputs(simmr_host::ovleval_pair_rows(ka.data(), kb.data(), ov.data(), best.data(), hits.data(), n).c_str(), stdout);
    } else {
      return 3;
    }
    printf("--\n");
  }
  return 0;
}
