// taxeval_report_main.cpp — the three formatters of --eval-classified and the two small-file readers of simmr_amd/host/host.cpp in a
// stand-alone program, for a build under the sanitizers (tests/test_taxeval_host.py).  Input, a command a block:
//   report <n nodes>\n<13 counts>\n<40 words of by_rank>\n<40 words of reads_by_rank>\n n rows "<rank code> <true> <called>"   -> the report
//   reads <n genomes> <n>\n n genomes rows "<genome id> <has mask>", then n rows "<id> <genome row> <mates> <seen> <hits>"     -> the rows
//   taxa <n>\n n rows "<taxid> <rank code> <true> <called> <both>"                                                           -> the rows
//   nodes <n bytes>\n then that many bytes of the file   -> "taxid parent rank-code" a line, or "error: ..."
//   map <n bytes>\n then that many bytes of the file     -> "genome_id taxid" a line, or "error: ..."
// Every answer ends with a line "--".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../simmr_amd/host/simmr_host.hpp"

using namespace simmr_host;

static bool words(std::vector<uint64_t>& v) {
  for (uint64_t& c : v) {
    unsigned long long x;
    if (scanf("%llu", &x) != 1) return false;
    c = x;
  }
  return true;
}

static bool block(std::vector<char>* text) {
  unsigned long n = 0;
  if (scanf("%lu", &n) != 1 || getchar() != '\n') return false;
  text->resize(n);  // (no byte behind the text: a read past it is caught)
  return n == 0 || fread(text->data(), 1, n, stdin) == n;
}

int main() {
  char cmd[16];
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "report")) {
      unsigned long n = 0;
      if (scanf("%lu", &n) != 1) return 2;
      std::vector<uint64_t> counts(TAXEVAL_N_COUNTS), by_rank(TAXEVAL_RANKS * TAXEVAL_CLASSES), reads_by_rank(TAXEVAL_RANKS * TAXEVAL_CLASSES);
      if (!words(counts) || !words(by_rank) || !words(reads_by_rank)) return 2;
      std::vector<uint8_t> rank(n);
      std::vector<uint64_t> t(n), c(n);
      for (unsigned long i = 0; i < n; i++) {
        unsigned r;
        unsigned long long x, y;
        if (scanf("%u %llu %llu", &r, &x, &y) != 3) return 2;
        rank[i] = (uint8_t)r; t[i] = x; c[i] = y;
      }
      fputs(taxeval_report(counts.data(), by_rank.data(), reads_by_rank.data(), rank.data(), t.data(), c.data(), n).c_str(), stdout);
    } else if (!strcmp(cmd, "reads")) {
      unsigned long ng = 0, n = 0;
      if (scanf("%lu %lu", &ng, &n) != 2) return 2;
      std::vector<std::string> ids(ng);
      std::vector<uint32_t> has(ng);
      for (unsigned long g = 0; g < ng; g++) {
        char text[300];
        unsigned m;
        if (scanf("%299s %u", text, &m) != 2) return 2;
        ids[g] = text; has[g] = m;
      }
      std::vector<uint64_t> id(n);
      std::vector<uint32_t> genome(n), mates(n), seen(n), hits(n);
      for (unsigned long i = 0; i < n; i++) {
        unsigned long long k;
        unsigned g, m, s, h;
        if (scanf("%llu %u %u %u %u", &k, &g, &m, &s, &h) != 5) return 2;
        id[i] = k; genome[i] = g; mates[i] = m; seen[i] = s; hits[i] = h;
      }
      fputs(taxeval_read_rows(ids, has, id.data(), genome.data(), mates.data(), seen.data(), hits.data(), n).c_str(), stdout);
    } else if (!strcmp(cmd, "taxa")) {
      unsigned long n = 0;
      if (scanf("%lu", &n) != 1) return 2;
      std::vector<uint32_t> taxid(n);
      std::vector<uint8_t> rank(n);
      std::vector<uint64_t> t(n), c(n), b(n);
      for (unsigned long i = 0; i < n; i++) {
        unsigned x, r;
        unsigned long long tt, cc, bb;
        if (scanf("%u %u %llu %llu %llu", &x, &r, &tt, &cc, &bb) != 5) return 2;
        taxid[i] = x; rank[i] = (uint8_t)r; t[i] = tt; c[i] = cc; b[i] = bb;
      }
      fputs(taxeval_taxa_rows(taxid.data(), rank.data(), t.data(), c.data(), b.data(), n).c_str(), stdout);
    } else if (!strcmp(cmd, "nodes")) {
      std::vector<char> text;
      if (!block(&text)) return 2;
      std::vector<uint32_t> taxid, parent;
      std::vector<uint8_t> rank;
      std::string err;
      if (!taxeval_parse_nodes(text.data(), text.size(), &taxid, &parent, &rank, &err)) printf("error: %s\n", err.c_str());
      else
        for (size_t i = 0; i < taxid.size(); i++) printf("%u %u %u\n", taxid[i], parent[i], (unsigned)rank[i]);
    } else if (!strcmp(cmd, "map")) {
      std::vector<char> text;
      if (!block(&text)) return 2;
      std::vector<std::string> ids;
      std::vector<uint32_t> taxid;
      std::string err;
      if (!taxeval_parse_map(text.data(), text.size(), &ids, &taxid, &err)) printf("error: %s\n", err.c_str());
      else
        for (size_t i = 0; i < ids.size(); i++) printf("%s %u\n", ids[i].c_str(), taxid[i]);
    } else {
      return 3;
    }
    printf("--\n");
  }
  return 0;
}
