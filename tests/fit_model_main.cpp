// Stand-alone host harness for tests/test_fit_host.py: the loader of simmr_amd/csrc/custom_model.hpp, the C++ bincode writer and
// the bin builder of simmr_amd/csrc/fit_host.hpp, without a GPU.
//   fit_model_main roundtrip IN OUT   parses IN with parse_model, prints the model's shape, writes serialize_model of it to OUT
//   fit_model_main bins CLAMP FILE    FILE: "value count" lines; prints n, mean, sd, width and the bins make_bins gives
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../simmr_amd/csrc/fit_host.hpp"

using namespace simmr;

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "roundtrip") {
    std::ifstream in(argv[2], std::ios::binary);
    const std::string bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    ModelHost m;
    std::string err;
    if (!parse_model((const uint8_t*)bytes.data(), bytes.size(), &m, &err)) { printf("ERR\t%s\n", err.c_str()); return 1; }
    uint64_t alts = 0;
    for (const auto& p : m.probabilities) alts += p.second.size();
    printf("%llu %llu %llu %llu %d %d %llu %llu %llu %llu %.17g %.17g %.17g %.17g\n", (unsigned long long)m.quality.size(),
           (unsigned long long)m.kmer_size, (unsigned long long)m.probabilities.size(), (unsigned long long)alts, m.is_long ? 1 : 0,
           m.has_insert_bins ? 1 : 0, (unsigned long long)m.read_length_bins.ranges.size(), (unsigned long long)m.read_length_bins.bin_width,
           (unsigned long long)m.insert_bins.ranges.size(), (unsigned long long)m.insert_bins.bin_width, m.read_length_mean, m.read_length_std,
           m.insert_size_mean, m.insert_size_std);
    if (!m.quality.empty()) printf("%llu %zu %zu\n", (unsigned long long)m.quality[0].num_bins, m.quality[0].density.size(), m.quality[0].ranges.size());
    const std::string again = serialize_model(m);
    std::ofstream out(argv[3], std::ios::binary);
    out.write(again.data(), (std::streamsize)again.size());
    return out.good() ? 0 : 1;
  }
  if (argc == 4 && std::string(argv[1]) == "bins") {
    std::vector<uint64_t> hist(65536, 0);
    std::ifstream in(argv[3]);
    uint64_t v, c;
    while (in >> v >> c)
      if (v < hist.size()) hist[v] += c;
    FitBins b;
    std::vector<double> pts;
    make_bins(hist, atoi(argv[2]) != 0, &b, &pts);
    printf("%llu %.17g %.17g %llu %d\n", (unsigned long long)b.n, b.mean, b.sd, (unsigned long long)b.width, b.point_mass ? 1 : 0);
    for (size_t i = 0; i < b.lo.size(); i++) printf("%u %u\n", b.lo[i], b.hi[i]);
    return 0;
  }
  fprintf(stderr, "usage: fit_model_main roundtrip IN OUT | bins CLAMP FILE\n");
  return 2;
}
