// fit_host.hpp — the host arithmetic of the model-fitting pass, free of HIP so that a plain C++ program can run it
// (tests/fit_model_main.cpp): the bins of the length and insert histograms as simmr_fit_plan makes them, and the bincode
// writer of a ModelHost — the inverse of custom_model.hpp's parse_model, byte for byte what simmr_amd/model_io.py writes.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "custom_model.hpp"

namespace simmr {

// one density column over a histogram: its bins and what the host derived for them
struct FitBins {
  std::vector<uint32_t> lo, hi;
  std::vector<double> density;  // filled on the host only for the single point-mass bin
  uint64_t n = 0, width = 0;
  double mean = 0.0, sd = 0.0;
  bool point_mass = false;
};

// Mean, population deviation, Freedman-Diaconis width and the bins of one histogram (hist[v] observations of value v),
// as create_read_length_bins (clamp_ends) / create_insert_size_bins restate them; pts receives the bins' mid-points.
inline void make_bins(const std::vector<uint64_t>& hist, bool clamp_ends, FitBins* b, std::vector<double>* pts) {
  *b = FitBins{};
  pts->clear();
  uint64_t n = 0, s1 = 0, vmin = 0, vmax = 0;
  for (uint64_t v = 0; v < hist.size(); v++)
    if (hist[v]) {
      if (!n) vmin = v;
      vmax = v;
      n += hist[v];
      s1 += hist[v] * v;
    }
  b->n = n;
  if (!n) return;
  b->mean = (double)s1 / (double)n;
  double var = 0.0;
  for (uint64_t v = vmin; v <= vmax; v++)
    if (hist[v]) var += (double)hist[v] * (((double)v - b->mean) * ((double)v - b->mean));
  b->sd = sqrt(var / (double)n);
  // the quartiles: the values at indices floor(n * 0.25) and floor(n * 0.75) of the sorted observations
  const uint64_t i1 = (uint64_t)floor((double)n * 0.25), i3 = (uint64_t)floor((double)n * 0.75);
  uint64_t q1 = vmax, q3 = vmax, cum = 0;
  bool have1 = false, have3 = false;
  for (uint64_t v = vmin; v <= vmax && !have3; v++) {
    cum += hist[v];
    if (!have1 && i1 < cum) { q1 = v; have1 = true; }
    if (!have3 && i3 < cum) { q3 = v; have3 = true; }
  }
  const double fd = 2.0 * ((double)(q3 - q1) / pow((double)n, 1.0 / 3.0));
  const uint64_t width = (uint64_t)fd > 1 ? (uint64_t)fd : 10;
  b->width = width;
  if (vmin == vmax) {  // the point mass: one bin (min, min)
    b->point_mass = true;
    b->lo.assign(1, (uint32_t)vmin);
    b->hi.assign(1, (uint32_t)vmin);
    b->density.assign(1, 1.0);
    return;
  }
  const uint64_t num = (uint64_t)ceil((double)(vmax - vmin) / (double)width);
  for (uint64_t i = 0; i < num; i++) {
    const uint32_t start = (uint32_t)vmin + (uint32_t)(i * width);
    uint32_t end = (uint32_t)vmin + (uint32_t)((i + 1) * width) - 1u;
    if (clamp_ends && end > (uint32_t)vmax) end = (uint32_t)vmax;
    b->lo.push_back(start);
    b->hi.push_back(end);
    pts->push_back((double)(start + end) / 2.0);
  }
}


// ---- bincode 1.3.3, default options: little-endian fixed-width integers, lengths as u64, Option as a u8 tag --------------
template <class T>
inline void fit_put(std::string* out, T v) { out->append((const char*)&v, sizeof v); }
inline void fit_put_bins(std::string* out, const BinsHost& b) {
  fit_put<uint64_t>(out, b.num_bins);
  fit_put<uint64_t>(out, b.bin_width);
  fit_put<uint64_t>(out, b.density.size());
  for (double d : b.density) fit_put<double>(out, d);
  fit_put<uint64_t>(out, b.ranges.size());
  for (const auto& r : b.ranges) { fit_put<uint32_t>(out, r.first); fit_put<uint32_t>(out, r.second); }
}
inline std::string serialize_model(const ModelHost& m) {
  std::string out;
  fit_put<uint64_t>(&out, m.bin_size);
  fit_put<uint64_t>(&out, m.quality.size());
  for (const BinsHost& b : m.quality) fit_put_bins(&out, b);
  fit_put<uint8_t>(&out, m.bit_encoding);
  fit_put<uint64_t>(&out, m.kmer_size);
  fit_put<uint64_t>(&out, m.probabilities.size());
  for (const auto& p : m.probabilities) {
    fit_put<uint32_t>(&out, p.first);
    fit_put<uint64_t>(&out, p.second.size());
    for (const auto& a : p.second) { fit_put<uint32_t>(&out, a.first); fit_put<float>(&out, a.second); }
  }
  fit_put<double>(&out, m.insert_size_mean);
  fit_put<double>(&out, m.insert_size_std);
  fit_put<uint8_t>(&out, m.has_insert_bins ? 1 : 0);
  if (m.has_insert_bins) fit_put_bins(&out, m.insert_bins);
  fit_put<double>(&out, m.read_length_mean);
  fit_put<double>(&out, m.read_length_std);
  fit_put_bins(&out, m.read_length_bins);
  fit_put<uint8_t>(&out, m.is_long ? 1 : 0);
  return out;
}

}  // namespace simmr
