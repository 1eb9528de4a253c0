// correval_report_main.cpp — the report formatter, the row writer and the ratio of simmr_amd/host/host.cpp's --eval-corrected share in a
// stand-alone program, for a build under the sanitizers (tests/test_correval_host.py).  Input, a command a block:
//   report\n 29 counts, 125 numbers of the cube, 95 x 5 of by_qual, 512 x 5 of by_pos   -> the report
//   sparse <n>\n 29 counts, then n triples (table 0 cube / 1 by_qual / 2 by_pos, index, value)   -> the report of tables that are zero elsewhere
//   rows <n>\n n rows of six numbers (key, length, before, residual, hits, and a 0 that is not read)   -> the rows
//   ratio <negative 0|1> <num> <den>                                                       -> the ratio
// Every answer ends with a line "--".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../simmr_amd/host/simmr_host.hpp"

using namespace simmr_host;

static bool numbers(std::vector<uint64_t>* v) {
  for (uint64_t& x : *v) {
    unsigned long long t;
    if (scanf("%llu", &t) != 1) return false;
    x = t;
  }
  return true;
}

int main() {
  char cmd[16];
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "report") || !strcmp(cmd, "sparse")) {
      std::vector<uint64_t> counts(CORREVAL_N_COUNTS), cube(125), by_qual(CORREVAL_N_QUALS * 5), by_pos(CORREVAL_N_POS * 5);
      if (!strcmp(cmd, "report")) {
        if (!numbers(&counts) || !numbers(&cube) || !numbers(&by_qual) || !numbers(&by_pos)) return 1;
      } else {
        unsigned long n = 0;
        if (scanf("%lu", &n) != 1 || !numbers(&counts)) return 1;
        for (unsigned long i = 0; i < n; i++) {
          std::vector<uint64_t> t(3);
          if (!numbers(&t)) return 1;
          std::vector<uint64_t>& table = t[0] == 0 ? cube : t[0] == 1 ? by_qual : by_pos;
          if (t[0] > 2 || t[1] >= table.size()) return 1;
          table[t[1]] = t[2];
        }
      }
      fputs(correval_report(counts.data(), cube.data(), by_qual.data(), by_pos.data()).c_str(), stdout);
    } else if (!strcmp(cmd, "rows")) {
      unsigned long n = 0;
      if (scanf("%lu", &n) != 1) return 1;
      std::vector<uint64_t> key(n), row(6);
      std::vector<uint32_t> length(n), before(n), residual(n), hits(n);
      for (unsigned long i = 0; i < n; i++) {
        if (!numbers(&row)) return 1;
        key[i] = row[0];
        length[i] = (uint32_t)row[1];
        before[i] = (uint32_t)row[2];
        residual[i] = (uint32_t)row[3];
        hits[i] = (uint32_t)row[4];
      }
      fputs(correval_read_rows(key.data(), length.data(), before.data(), residual.data(), hits.data(), n).c_str(), stdout);
    } else if (!strcmp(cmd, "ratio")) {
      std::vector<uint64_t> v(3);
      if (!numbers(&v)) return 1;
      puts(correval_ratio(v[0] != 0, v[1], v[2]).c_str());
    } else {
      return 2;
    }
    puts("--");
  }
  return 0;
}
