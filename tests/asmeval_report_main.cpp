// asmeval_report_main.cpp — the report formatter, the contig rows, the FASTA record reader and the contiguity of
// simmr_amd/host/host.cpp in a stand-alone program, for a build under the sanitizers (tests/test_asmeval_host.py).  Input, a
// command a block:
//   report <k> <n genomes> <n truth> <n contigs>\n the genome names, 18 counts, (n genomes + 1) x 5 numbers, the lengths  -> the report
//   contigs <n names> <n genomes> <n>\n the names, the genome names, then n rows of six numbers                           -> the rows
//   fasta <n bytes>\n then that many bytes of text                                            -> "<first word>\t<length>" a record
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
      unsigned k = 0;
      unsigned long ng = 0, nt = 0, nc = 0;
      if (scanf("%u %lu %lu %lu", &k, &ng, &nt, &nc) != 4) return 2;
      std::vector<std::string> genomes(ng);
      std::vector<uint64_t> counts(simmr_host::ASMEVAL_N_COUNTS), by((ng + 1) * simmr_host::ASMEVAL_GENOME_COLS), tl(nt), cl(nc);  // exactly what it may read
      if (!words(&genomes) || !numbers(&counts) || !numbers(&by) || !numbers(&tl) || !numbers(&cl)) return 2;
      fputs(simmr_host::asmeval_report(counts.data(), k, genomes, by.data(), tl.data(), nt, cl.data(), nc).c_str(), stdout);
    } else if (!strcmp(cmd, "contigs")) {
      unsigned long nn = 0, ng = 0, n = 0;
      if (scanf("%lu %lu %lu", &nn, &ng, &n) != 3) return 2;
      std::vector<std::string> names(nn), genomes(ng);
      if (!words(&names) || !words(&genomes)) return 2;
      std::vector<uint64_t> length(n);
      std::vector<uint32_t> c[5];
      for (auto& v : c) v.resize(n);
      for (unsigned long i = 0; i < n; i++) {
        unsigned long long l;
        unsigned a, b, d, e, f;
        if (scanf("%llu %u %u %u %u %u", &l, &a, &b, &d, &e, &f) != 6) return 2;
        length[i] = l; c[0][i] = a; c[1][i] = b; c[2][i] = d; c[3][i] = e; c[4][i] = f;
      }
      fputs(simmr_host::asmeval_contig_rows(names, genomes, length.data(), c[0].data(), c[1].data(), c[2].data(), c[3].data(), c[4].data(), n).c_str(), stdout);
    } else if (!strcmp(cmd, "fasta")) {
      unsigned long n = 0;
      if (scanf("%lu", &n) != 1 || getchar() != '\n') return 2;
      std::vector<char> text(n);  // (no byte behind the text: a read past it is caught)
      if (n > 0 && fread(text.data(), 1, n, stdin) != n) return 2;
      std::vector<std::string> w;
      std::vector<uint64_t> len;
      simmr_host::asmeval_fasta_records(text.data(), n, &w, &len);
      for (size_t i = 0; i < w.size(); i++) printf("%s\t%llu\n", w[i].c_str(), (unsigned long long)len[i]);
    } else {
      return 3;
    }
    printf("--\n");
  }
  return 0;
}
