// vcfeval_report_main.cpp — the report formatter, the rows of --eval-vcf-sites and the ##contig reader of simmr_amd/host/host.cpp in
// a stand-alone program, for a build under the sanitizers (tests/test_vcfeval_host.py).  Input, a command a block:
//   report\n<24 counts>\n<k> then k rows "<qual row> <correct> <wrong>"\n<m> then m rows "<bits> <found> <not found>"   -> the report
//   sites <n names> <n>\n the names, then n rows "<key> <alleles> <ad> <best> <hits>"                                  -> the rows
//   contigs <n bytes>\n then that many bytes of header text                                                            -> a name a line
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
      std::vector<uint64_t> counts(simmr_host::VCFEVAL_N_COUNTS), by_qual(512, 0), by_ad(2 * simmr_host::VCFEVAL_AD_ROWS, 0);  // exactly what the formatter may read
      for (uint64_t& c : counts) {
        unsigned long long v;
        if (scanf("%llu", &v) != 1) return 2;
        c = v;
      }
      for (int table = 0; table < 2; table++) {
        std::vector<uint64_t>& by = table ? by_ad : by_qual;
        unsigned long k = 0;
        if (scanf("%lu", &k) != 1) return 2;
        for (unsigned long i = 0; i < k; i++) {
          unsigned long b;
          unsigned long long x, y;
          if (scanf("%lu %llu %llu", &b, &x, &y) != 3 || 2 * b + 1 >= by.size()) return 2;
          by[2 * b] = x;
          by[2 * b + 1] = y;
        }
      }
      fputs(simmr_host::vcfeval_report(counts.data(), by_qual.data(), by_ad.data()).c_str(), stdout);
    } else if (!strcmp(cmd, "sites")) {
      unsigned long n_names = 0, n = 0;
      if (scanf("%lu %lu", &n_names, &n) != 2) return 2;
      std::vector<std::string> names(n_names);
      for (std::string& s : names) {
        char text[300];
        if (scanf("%299s", text) != 1) return 2;
        s = text;
      }
      std::vector<uint64_t> key(n);
      std::vector<uint32_t> alleles(n), ad(n), best(n), hits(n);
      for (unsigned long i = 0; i < n; i++) {
        unsigned long long k;
        unsigned a, d, x, h;
        if (scanf("%llu %u %u %u %u", &k, &a, &d, &x, &h) != 5) return 2;
        key[i] = k; alleles[i] = a; ad[i] = d; best[i] = x; hits[i] = h;
      }
      fputs(simmr_host::vcfeval_site_rows(names, key.data(), alleles.data(), ad.data(), best.data(), hits.data(), n).c_str(), stdout);
    } else if (!strcmp(cmd, "contigs")) {
      unsigned long n = 0;
      if (scanf("%lu", &n) != 1 || getchar() != '\n') return 2;
      std::vector<char> text(n);  // (no byte behind the text: a read past it is caught)
      if (n > 0 && fread(text.data(), 1, n, stdin) != n) return 2;
      std::vector<std::string> names;
      simmr_host::vcfeval_contig_names(text.data(), n, &names);
      for (const std::string& s : names) printf("%s\n", s.c_str());
    } else {
      return 3;
    }
    printf("--\n");
  }
  return 0;
}
