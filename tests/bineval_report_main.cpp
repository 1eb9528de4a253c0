// bineval_report_main.cpp — the report formatter, the two row writers, the name readers and the adjusted Rand index of
// simmr_amd/host/host.cpp in a stand-alone program, for a build under the sanitizers (tests/test_bineval_host.py).  Input, a command a
// block:
//   report <n genomes> <n bins>\n the genome names, the bin names, 21 counts, (n genomes + 1) x 7 numbers, n bins rows of five numbers
//          (contigs, bases, none_bases, top_genome, top_bases)                                                            -> the report
//   cells <n bins> <n genomes> <n>\n the bin names, the genome names, n rows of four numbers                              -> the rows
//   contigs <n names> <n genomes> <n bins> <n>\n the three name lists, n rows of four numbers (genome, length, bin, records) -> the rows
//   ari <cells> <bins> <genomes> <n>                                                                                       -> the index
//   truth <n bytes>\n text   -> "<contig>\t<genome>" a record line;   records <n bytes>\n text   -> "<bin>" a record line
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
      unsigned long ng = 0, nb = 0;
      if (scanf("%lu %lu", &ng, &nb) != 2) return 2;
      std::vector<std::string> genomes(ng), bins(nb);
      std::vector<uint64_t> counts(simmr_host::BINEVAL_N_COUNTS), by((ng + 1) * simmr_host::BINEVAL_GENOME_COLS), rows(nb * 5);
      if (!words(&genomes) || !words(&bins) || !numbers(&counts) || !numbers(&by) || !numbers(&rows)) return 2;
      std::vector<uint32_t> contigs(nb), top(nb);  // exactly what it may read
      std::vector<uint64_t> bases(nb), none(nb), top_bases(nb);
      for (unsigned long b = 0; b < nb; b++) {
        contigs[b] = (uint32_t)rows[5 * b]; bases[b] = rows[5 * b + 1]; none[b] = rows[5 * b + 2]; top[b] = (uint32_t)rows[5 * b + 3]; top_bases[b] = rows[5 * b + 4];
      }
      fputs(simmr_host::bineval_report(counts.data(), genomes, by.data(), bins, contigs.data(), bases.data(), none.data(), top.data(), top_bases.data(), nb).c_str(), stdout);
    } else if (!strcmp(cmd, "cells")) {
      unsigned long nb = 0, ng = 0, n = 0;
      if (scanf("%lu %lu %lu", &nb, &ng, &n) != 3) return 2;
      std::vector<std::string> bins(nb), genomes(ng);
      std::vector<uint64_t> rows(n * 4);
      if (!words(&bins) || !words(&genomes) || !numbers(&rows)) return 2;
      std::vector<uint32_t> b(n), g(n), c(n);
      std::vector<uint64_t> bases(n);
      for (unsigned long i = 0; i < n; i++) { b[i] = (uint32_t)rows[4 * i]; g[i] = (uint32_t)rows[4 * i + 1]; c[i] = (uint32_t)rows[4 * i + 2]; bases[i] = rows[4 * i + 3]; }
      fputs(simmr_host::bineval_cell_rows(bins, genomes, b.data(), g.data(), c.data(), bases.data(), n).c_str(), stdout);
    } else if (!strcmp(cmd, "contigs")) {
      unsigned long nn = 0, ng = 0, nb = 0, n = 0;
      if (scanf("%lu %lu %lu %lu", &nn, &ng, &nb, &n) != 4) return 2;
      std::vector<std::string> names(nn), genomes(ng), bins(nb);
      std::vector<uint64_t> rows(n * 4);
      if (!words(&names) || !words(&genomes) || !words(&bins) || !numbers(&rows)) return 2;
      std::vector<uint32_t> g(n), b(n), r(n);
      std::vector<uint64_t> length(n);
      for (unsigned long i = 0; i < n; i++) { g[i] = (uint32_t)rows[4 * i]; length[i] = rows[4 * i + 1]; b[i] = (uint32_t)rows[4 * i + 2]; r[i] = (uint32_t)rows[4 * i + 3]; }
      fputs(simmr_host::bineval_contig_rows(names, genomes, bins, g.data(), length.data(), b.data(), r.data(), n).c_str(), stdout);
    } else if (!strcmp(cmd, "ari")) {
      std::vector<uint64_t> v(4);
      if (!numbers(&v)) return 2;
      printf("%s\n", simmr_host::bineval_ari(v[0], v[1], v[2], v[3]).c_str());
    } else if (!strcmp(cmd, "truth") || !strcmp(cmd, "records")) {
      unsigned long n = 0;
      if (scanf("%lu", &n) != 1 || getchar() != '\n') return 2;
      std::vector<char> text(n);  // (no byte behind the text: a read past it is caught)
      if (n > 0 && fread(text.data(), 1, n, stdin) != n) return 2;
      std::vector<std::string> a, b;
      if (cmd[0] == 't') {
        simmr_host::bineval_truth_names(text.data(), n, &a, &b);
        for (size_t i = 0; i < a.size(); i++) printf("%s\t%s\n", a[i].c_str(), b[i].c_str());
      } else {
        simmr_host::bineval_record_bins(text.data(), n, &b);
        for (const std::string& s : b) printf("%s\n", s.c_str());
      }
    } else {
      return 3;
    }
    printf("--\n");
  }
  return 0;
}
