// asmmap_report_main.cpp — the report formatter, the block rows, the contig rows and NGA50 of simmr_amd/host/host.cpp
// (--eval-placement) in a stand-alone program, for a build under the sanitizers (tests/test_asmmap_host.py).  Input, a command a block:
//   report <k> <band> <relocation> <min_anchors> <n genomes> <n blocks>\n the genome names, 27 counts, n genomes x 5 numbers,
//          the block lengths, the blocks' genome rows                                                          -> the report
//   blocks <n contig names> <n truth names> <n>\n the names of either side, then n rows of nine numbers        -> the rows
//   contigs <n names> <n>\n the names, then n rows of six numbers                                              -> the rows
//   nga50 <n> <target>\n n lengths                                                                             -> the number or NA
// Every answer ends with a line "--".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../simmr_amd/host/simmr_host.hpp"

static bool words(std::vector<std::string>* v) {
  for (std::string& s : *v) {
    char text[300];
    if (scanf("%299s", text) != 1) return false;
    s = text;
  }
  return true;
}
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
    if (!strcmp(cmd, "report")) {
      unsigned k = 0, band = 0, relocation = 0, min_anchors = 0;
      unsigned long ng = 0, nb = 0;
      if (scanf("%u %u %u %u %lu %lu", &k, &band, &relocation, &min_anchors, &ng, &nb) != 6) return 2;
      std::vector<std::string> genomes(ng);
      std::vector<uint64_t> counts(simmr_host::ASMMAP_N_COUNTS), by(ng * simmr_host::ASMMAP_GENOME_COLS), len(nb), rows(nb);  // exactly what it may read
      if (!words(&genomes) || !numbers(&counts) || !numbers(&by) || !numbers(&len) || !numbers(&rows)) return 2;
      std::vector<uint32_t> genome_of(rows.begin(), rows.end());
      fputs(simmr_host::asmmap_report(counts.data(), k, band, relocation, min_anchors, genomes, by.data(), len.data(), genome_of.data(), nb).c_str(), stdout);
    } else if (!strcmp(cmd, "blocks")) {
      unsigned long nc = 0, nt = 0, n = 0;
      if (scanf("%lu %lu %lu", &nc, &nt, &n) != 3) return 2;
      std::vector<std::string> contigs(nc), truths(nt);
      if (!words(&contigs) || !words(&truths)) return 2;
      std::vector<uint32_t> c[9];
      for (auto& v : c) v.resize(n);
      for (unsigned long i = 0; i < n; i++)
        for (auto& v : c) {
          unsigned x;
          if (scanf("%u", &x) != 1) return 2;
          v[i] = x;
        }
      const uint32_t* cols[9];
      for (int j = 0; j < 9; j++) cols[j] = c[j].data();
      fputs(simmr_host::asmmap_block_rows(contigs, truths, cols, n).c_str(), stdout);
    } else if (!strcmp(cmd, "contigs")) {
      unsigned long nn = 0, n = 0;
      if (scanf("%lu %lu", &nn, &n) != 2) return 2;
      std::vector<std::string> names(nn);
      if (!words(&names)) return 2;
      std::vector<uint64_t> length(n), bases(n);
      std::vector<uint32_t> c[4];
      for (auto& v : c) v.resize(n);
      for (unsigned long i = 0; i < n; i++) {
        unsigned long long l, bb;
        unsigned a, b, d, e;
        if (scanf("%llu %u %u %u %llu %u", &l, &a, &b, &d, &bb, &e) != 6) return 2;
        length[i] = l; c[0][i] = a; c[1][i] = b; c[2][i] = d; bases[i] = bb; c[3][i] = e;
      }
      fputs(simmr_host::asmmap_contig_rows(names, length.data(), c[0].data(), c[1].data(), c[2].data(), bases.data(), c[3].data(), n).c_str(), stdout);
    } else if (!strcmp(cmd, "nga50")) {
      unsigned long n = 0;
      unsigned long long target = 0;
      if (scanf("%lu %llu", &n, &target) != 2) return 2;
      std::vector<uint64_t> len(n);
      if (!numbers(&len)) return 2;
      printf("%s\n", simmr_host::asmmap_nga50(len.data(), n, target).c_str());
    } else {
      return 3;
    }
    printf("--\n");
  }
  return 0;
}
