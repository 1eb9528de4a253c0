// fit.hip — fitting a simmrd-format error model from the reads of a run (include/simmr_hip.h: simmr_fit_*): the entry
// points over fit_kernels.hip.  A translation unit of its own; it sees an engine through engine_internal.hpp only and keeps
// its state in the engine's opaque slot (host_support.hpp: unit_state; simmr_engine_destroy deletes it, and its members free what they own).
//
// reset: the tables (dense identity counts, the pair table, the three histograms) zeroed on the stream.
// add:   k_fit_add, enqueue-only.
// plan:  the error word and the length and insert histograms come to the host, which takes the means, the quartiles and
//        the bins from them (a few thousand entries of f64 arithmetic).  Everything else stays on the device: k_fit_compact
//        counts and lists the live pairs, the radix sort shared with sam_sort.hip and overlap.hip (samsort_sort_pairs) orders
//        them in three stable runs (alt, ~count, ref), k_fit_segments / k_fit_ref_scan / k_fit_pairs take the totals, cut and
//        divide, k_fit_density evaluates the quality, length and insert densities.  Two numbers come back: the sizes.
// emit:  device-to-device copies into the caller's columns (the bin ranges, which the host made, go up from the host).
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>
#include <vector>

#include "fit_kernels.hip"
#include "fit_host.hpp"
#include "host_support.hpp"

using namespace simmr;

namespace {

struct FitState {
  uint32_t k = 0, max_alt = 0;
  uint64_t n_dense = 0, n_slots = 0;
  bool ready = false, planned = false;
  // what of qhist a reset has to clear: every add is followed by a plan that says how far its reads reached (dirty_pos, the
  // largest since the tables were last cleared whole); an add without a plan behind it leaves the whole table suspect
  uint64_t dirty_pos = 0, clean_dense = 0, clean_slots = 0;
  bool unplanned_add = true;
  // tables: dense | hkey | hcnt | qhist | lhist | ihist | n_out (8 bytes) | err (8 bytes) | the SAM route's counts
  DevBuf tables, out_key, out_cnt, pts, qdens, ldens, idens;
  // the finish: sort buffers, the per-reference tables (start | n_alt | total | first | sizes[2]), the model's pair columns
  DevBuf skey[2], sidx[2], perm[2], hist, digit_total, refs, kmer_ref, kmer_first, pair_alt, pair_count, pair_prob;
  Spans<1> sp;  // the last add (the SAM route's adds record it through fit_share)
  // the planned model (host side)
  simmr_fit_info info{};
  FitBins len, ins;

  static constexpr uint64_t Q_WORDS = (uint64_t)FIT_MAX_L * SIMMR_FIT_QUALS, L_WORDS = FIT_MAX_L + 1ull, I_WORDS = SIMMR_FIT_MAX_INSERT + 1ull;
  uint64_t words() const { return n_dense + 2 * n_slots + Q_WORDS + L_WORDS + I_WORDS + 2 + FIT_SAM_COUNTS; }
  unsigned long long* w(uint64_t at) const { return tables.as<unsigned long long>() + at; }
  unsigned long long* dense() const { return w(0); }
  unsigned long long* hkey() const { return w(n_dense); }
  unsigned long long* hcnt() const { return w(n_dense + n_slots); }
  unsigned long long* qhist() const { return w(n_dense + 2 * n_slots); }
  unsigned long long* lhist() const { return qhist() + Q_WORDS; }
  unsigned long long* ihist() const { return lhist() + L_WORDS; }
  unsigned long long* n_out() const { return ihist() + I_WORDS; }
  uint32_t* err() const { return (uint32_t*)(n_out() + 1); }
  unsigned long long* sam_counts() const { return n_out() + 2; }
  FitTables dev() const { return FitTables{dense(), hkey(), hcnt(), qhist(), lhist(), ihist(), err(), (uint32_t)(n_slots - 1), k}; }
};

constexpr auto fit_state = unit_state<FitState, ENG_EXT_FIT>;

}  // namespace

namespace simmr {

bool fit_share(simmr_engine* e, FitShare* out) {
  FitState* s = fit_state(e, false);
  if (!s || !s->ready) return false;
  *out = FitShare{s->dev(), s->sam_counts(), {s->sp.ev[0], s->sp.ev[1]}};
  return true;
}

void fit_share_added(simmr_engine* e) {
  FitState* s = fit_state(e, false);
  if (!s) return;
  s->planned = false;
  s->unplanned_add = true;
  s->sp.mark(0);
}

}  // namespace simmr

extern "C" {

int simmr_fit_reset(simmr_engine* e, uint32_t k, uint32_t max_alt_kmers, uint64_t pair_capacity) {
  if (!e) return SIMMR_EINVAL;
  if (k < 3u || k > 10u) return eng_fail(e, SIMMR_EINVAL, "simmr_fit_reset: k is 3 .. 10");
  if (max_alt_kmers == 0u) return eng_fail(e, SIMMR_EINVAL, "simmr_fit_reset: max_alt_kmers is at least 1");
  if (pair_capacity == 0 || pair_capacity > (1ull << 26)) return eng_fail(e, SIMMR_EINVAL, "simmr_fit_reset: pair_capacity is 1 .. 2^26");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  FitState* s = fit_state(e, true);
  s->ready = s->planned = false;
  s->sp.invalidate_from(0);
  if (int rc = s->sp.create_missing(e)) return rc;
  s->k = k;
  s->max_alt = max_alt_kmers;
  s->n_dense = 1ull << (2u * k);
  s->n_slots = 2;
  while (s->n_slots < 2 * pair_capacity) s->n_slots <<= 1;
  const size_t cap_before = s->tables.cap;
  if (!s->tables.ensure(s->words() * 8))
    return eng_fail(e, SIMMR_ENOMEM, "fit table allocation failed (k %u, %llu pair slots)", k, (unsigned long long)s->n_slots);
  hipStream_t st = eng_stream(e);
  // qhist is 49 MB whatever the reads' lengths: cleared whole only where its contents are not known (new memory, another layout,
  // an add no plan has looked at), otherwise up to the longest read the plans since have seen
  const bool whole = s->tables.cap != cap_before || s->clean_dense != s->n_dense || s->clean_slots != s->n_slots || s->unplanned_add;
  if (whole) {
    HIP_TRY(e, hipMemsetAsync(s->tables.p, 0, s->words() * 8, st));
  } else {
    HIP_TRY(e, hipMemsetAsync(s->tables.p, 0, (s->n_dense + 2 * s->n_slots + s->dirty_pos * SIMMR_FIT_QUALS) * 8, st));
    HIP_TRY(e, hipMemsetAsync(s->lhist(), 0, (FitState::L_WORDS + FitState::I_WORDS + 2 + FIT_SAM_COUNTS) * 8, st));
  }
  s->dirty_pos = 0;
  s->unplanned_add = false;
  s->clean_dense = s->n_dense;
  s->clean_slots = s->n_slots;
  HIP_TRY(e, hipMemsetAsync(s->hkey(), 0xff, s->n_slots * 8, st));
  s->ready = true;
  return SIMMR_OK;
}

int simmr_fit_add(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads, uint32_t n_sets) {
  if (!e) return SIMMR_EINVAL;
  if (!reads) return eng_fail(e, SIMMR_EINVAL, "simmr_fit_add: NULL argument");
  if (n_sets != 1u && n_sets != 2u) return eng_fail(e, SIMMR_EINVAL, "simmr_fit_add: n_sets is 1 or 2");
  if (n_sets == 2u && (n_reads & 1u)) return eng_fail(e, SIMMR_EINVAL, "simmr_fit_add: a paired shard has an even number of reads");
  if (!reads->seq || !reads->qual || !reads->seq_off || !reads->start || !reads->end || !reads->contig || !reads->genome || !reads->flags)
    return eng_fail(e, SIMMR_EINVAL, "simmr_fit_add needs seq, qual, seq_off, start, end, contig, genome and flags");
  FitState* s = fit_state(e, false);
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_fit_add called before simmr_fit_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, s->sp.begin(0, st));
  if (n_reads > 0) {
    // persistent: one workgroup per CU (the LDS image takes most of a CU's 160 KB), each looping over its share of the batches
    const uint64_t batches = (n_reads + FIT_WG_READS - 1) / FIT_WG_READS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(batches, (uint64_t)eng_cu_count(e));
    uint32_t n_genomes = 0;
    const GenomeDev* genomes = eng_genome_table(e, &n_genomes);
    const TruthReads rd{reads->seq, reads->qual, reads->seq_off, reads->start, reads->end, reads->contig, reads->genome,
                        reads->flags, reads->seq_capacity, reads->slot_bytes == SIMMR_SLOT16 ? 1u : 0u};
    hipLaunchKernelGGL(k_fit_add, dim3(grid), dim3(FIT_WG), 0, st, genomes, n_genomes, rd, n_reads, n_sets, reads->qual_offset, s->dev());
  }
  HIP_TRY(e, s->sp.end(0, st));
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "fit launch failed: %s", hipGetErrorString(rc));
  s->planned = false;
  s->unplanned_add = true;
  s->sp.mark(0);
  return SIMMR_OK;
}

int simmr_fit_plan(simmr_engine* e, simmr_fit_info* info) {
  if (!e) return SIMMR_EINVAL;
  if (!info) return eng_fail(e, SIMMR_EINVAL, "simmr_fit_plan: NULL argument");
  FitState* s = fit_state(e, false);
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_fit_plan called before simmr_fit_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  s->planned = false;
  // ---- the error word and the two small histograms
  uint32_t errw = 0;
  std::vector<uint64_t> lhist(FitState::L_WORDS), ihist(FitState::I_WORDS);
  HIP_TRY(e, hipMemcpyAsync(&errw, s->err(), 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(lhist.data(), s->lhist(), FitState::L_WORDS * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(ihist.data(), s->ihist(), FitState::I_WORDS * 8, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "fit add")) return rc;
  if (errw & FIT_ERR_READ)
    return eng_fail(e, SIMMR_EINVAL, "a read added since the last simmr_fit_reset names a genome slot or a contig that is not staged, its window "
                                     "leaves its contig or seq[], or it is longer than %u bases", SIMMR_FIT_MAX_L);
  if (errw & FIT_ERR_QUAL)
    return eng_fail(e, SIMMR_EINVAL, "a read added since the last simmr_fit_reset has a quality above %u", SIMMR_FIT_MAX_Q);
  if (errw & FIT_ERR_SAM)
    return eng_fail(e, SIMMR_EINVAL, "a SAM record added since the last simmr_fit_reset is malformed (fewer than 11 fields, a FLAG, MAPQ or TLEN that "
                                     "is no number, a CIGAR that is neither * nor runs of <digits><op>, a QUAL that is neither * nor as long as SEQ "
                                     "or holds a byte outside '!' .. '~')");
  if (errw & FIT_ERR_FULL)
    return eng_fail(e, SIMMR_ERANGE, "the pair table of simmr_fit_reset (%llu slots) is full", (unsigned long long)s->n_slots);
  // ---- lengths and inserts: scalars and bins on the host, mid-points to the device
  std::vector<double> lpts, ipts, pts(SIMMR_FIT_DENSITIES);
  make_bins(lhist, true, &s->len, &lpts);
  make_bins(ihist, false, &s->ins, &ipts);
  uint64_t n_pos = 0;
  for (uint64_t v = 0; v < lhist.size(); v++)
    if (lhist[v]) n_pos = v;
  const bool is_long = s->len.n && s->len.mean > 400.0;
  if (is_long) { s->ins.lo.clear(); s->ins.hi.clear(); s->ins.density.clear(); ipts.clear(); s->ins.point_mass = false; }
  for (uint32_t i = 0; i < SIMMR_FIT_DENSITIES; i++) pts[i] = (double)i;
  const size_t lp0 = pts.size();
  pts.insert(pts.end(), lpts.begin(), lpts.end());
  const size_t ip0 = pts.size();
  pts.insert(pts.end(), ipts.begin(), ipts.end());
  if (!s->pts.ensure(pts.size() * 8) || !s->qdens.ensure(std::max<uint64_t>(n_pos, 1) * SIMMR_FIT_DENSITIES * 8) ||
      !s->ldens.ensure(std::max<size_t>(s->len.lo.size(), 1) * 8) || !s->idens.ensure(std::max<size_t>(s->ins.lo.size(), 1) * 8))
    return eng_fail(e, SIMMR_ENOMEM, "fit density allocation failed (%llu positions)", (unsigned long long)n_pos);
  HIP_TRY(e, hipMemcpyAsync(s->pts.p, pts.data(), pts.size() * 8, hipMemcpyHostToDevice, st));
  // ---- the device work: the densities
  if (n_pos > 0)
    hipLaunchKernelGGL(k_fit_density, dim3((uint32_t)n_pos, 1), dim3(FIT_DENSITY_WG), 0, st, s->qhist(), (uint64_t)SIMMR_FIT_QUALS, SIMMR_FIT_QUALS,
                       s->pts.as<const double>(), SIMMR_FIT_DENSITIES, SIMMR_FIT_DENSITIES, 70.0, s->qdens.as<double>());
  const uint32_t per_wg = 16;
  if (!lpts.empty())
    hipLaunchKernelGGL(k_fit_density, dim3(1, (uint32_t)((lpts.size() + per_wg - 1) / per_wg)), dim3(FIT_DENSITY_WG), 0, st, s->lhist(), 0ull,
                       (uint32_t)FitState::L_WORDS, s->pts.as<const double>() + lp0, (uint32_t)lpts.size(), per_wg, 1e300, s->ldens.as<double>());
  if (!ipts.empty())
    hipLaunchKernelGGL(k_fit_density, dim3(1, (uint32_t)((ipts.size() + per_wg - 1) / per_wg)), dim3(FIT_DENSITY_WG), 0, st, s->ihist(), 0ull,
                       (uint32_t)FitState::I_WORDS, s->pts.as<const double>() + ip0, (uint32_t)ipts.size(), per_wg, 1e300, s->idens.as<double>());
  if (s->len.point_mass) HIP_TRY(e, hipMemcpyAsync(s->ldens.p, s->len.density.data(), 8, hipMemcpyHostToDevice, st));
  if (s->ins.point_mass) HIP_TRY(e, hipMemcpyAsync(s->idens.p, s->ins.density.data(), 8, hipMemcpyHostToDevice, st));
  // ---- the pairs: counted, listed, sorted by (ref, count descending, alt ascending), totalled, cut, divided
  const uint64_t n_scan = s->n_dense + s->n_slots;
  const uint32_t scan_grid = (uint32_t)((n_scan + 255) / 256);
  unsigned long long n_live = 0;
  HIP_TRY(e, hipMemsetAsync(s->n_out(), 0, 8, st));
  hipLaunchKernelGGL(k_fit_compact, dim3(scan_grid), dim3(256), 0, st, s->dev(), s->n_dense, s->n_slots, (unsigned long long*)nullptr,
                     (unsigned long long*)nullptr, 0ull, s->n_out());
  HIP_TRY(e, hipMemcpyAsync(&n_live, s->n_out(), 8, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "fit plan (count)")) return rc;
  if (n_live > n_scan) return eng_fail(e, SIMMR_ENODEV, "fit plan: %llu live pairs in %llu entries", n_live, (unsigned long long)n_scan);
  const uint64_t n = n_live, n1 = std::max<uint64_t>(n, 1), n_tiles = (n + SAMSORT_PAIRS_TILE - 1) / SAMSORT_PAIRS_TILE;
  const uint64_t max_refs = std::min<uint64_t>(n, s->n_dense);
  const uint64_t refs_bytes = s->n_dense * 24 + 16;  // start and n_alt (4 bytes each), total and first (8 each), sizes[2]
  if (!s->out_key.ensure(n1 * 8) || !s->out_cnt.ensure(n1 * 8) || !s->skey[0].ensure(n1 * 8) || !s->skey[1].ensure(n1 * 8) ||
      !s->sidx[0].ensure(n1 * 4) || !s->sidx[1].ensure(n1 * 4) || !s->perm[0].ensure(n1 * 4) || !s->perm[1].ensure(n1 * 4) ||
      !s->hist.ensure(std::max<uint64_t>(n_tiles, 1) * SAMSORT_PAIRS_DIGITS * 4) || !s->digit_total.ensure(SAMSORT_PAIRS_DIGITS * 4) ||
      !s->refs.ensure(refs_bytes) || !s->kmer_ref.ensure((max_refs + 1) * 4) || !s->kmer_first.ensure((max_refs + 1) * 8) ||
      !s->pair_alt.ensure(n1 * 4) || !s->pair_count.ensure(n1 * 8) || !s->pair_prob.ensure(n1 * 4))
    return eng_fail(e, SIMMR_ENOMEM, "fit plan allocation failed (%llu pairs)", n_live);
  unsigned long long* const total = s->refs.as<unsigned long long>();
  const FitRefs R{(uint32_t*)(total + 2 * s->n_dense), (uint32_t*)(total + 2 * s->n_dense) + s->n_dense, total, total + s->n_dense};
  unsigned long long* const sizes = total + 3 * s->n_dense;
  HIP_TRY(e, hipMemsetAsync(s->refs.p, 0, refs_bytes, st));
  HIP_TRY(e, hipMemsetAsync(R.start, 0xff, s->n_dense * 4, st));
  HIP_TRY(e, hipMemsetAsync(s->kmer_first.p, 0, 8, st));
  if (n > 0) {
    HIP_TRY(e, hipMemsetAsync(s->n_out(), 0, 8, st));
    const unsigned long long* in_key = s->out_key.as<const unsigned long long>();
    const unsigned long long* in_cnt = s->out_cnt.as<const unsigned long long>();
    hipLaunchKernelGGL(k_fit_compact, dim3(scan_grid), dim3(256), 0, st, s->dev(), s->n_dense, s->n_slots, s->out_key.as<unsigned long long>(),
                       s->out_cnt.as<unsigned long long>(), n, s->n_out());
    uint64_t* const keys[2] = {s->skey[0].as<uint64_t>(), s->skey[1].as<uint64_t>()};
    uint32_t* const idxs[2] = {s->sidx[0].as<uint32_t>(), s->sidx[1].as<uint32_t>()};
    const uint32_t grid = (uint32_t)((n + 255) / 256), bits[3] = {3u * s->k, 64u, 3u * s->k};
    const uint32_t* perm_prev = nullptr;
    const uint32_t* idx = nullptr;
    for (uint32_t run = 0; run <= 3u; run++) {  // runs 0 .. 2 sort; the last turn only composes the permutation
      uint32_t* const perm_out = s->perm[run & 1u].as<uint32_t>();
      hipLaunchKernelGGL(k_fit_sort_key, dim3(grid), dim3(256), 0, st, run, in_key, in_cnt, perm_prev, idx, n, perm_out,
                         s->skey[0].as<unsigned long long>());
      perm_prev = perm_out;
      if (run < 3u) idx = idxs[samsort_sort_pairs(st, keys, idxs, s->hist.as<uint32_t>(), s->digit_total.as<uint32_t>(), n, bits[run])];
    }
    hipLaunchKernelGGL(k_fit_segments, dim3(grid), dim3(256), 0, st, in_key, in_cnt, perm_prev, n, s->k, R);
    hipLaunchKernelGGL(k_fit_ref_scan, dim3(1), dim3(1024), 0, st, R, (uint32_t)s->n_dense, s->k, s->max_alt, s->kmer_ref.as<uint32_t>(),
                       s->kmer_first.as<unsigned long long>(), sizes);
    hipLaunchKernelGGL(k_fit_pairs, dim3(grid), dim3(256), 0, st, in_key, in_cnt, perm_prev, n, s->k, s->max_alt, R, s->pair_alt.as<uint32_t>(),
                       s->pair_count.as<unsigned long long>(), s->pair_prob.as<float>());
  }
  unsigned long long got[2] = {0, 0};
  HIP_TRY(e, hipMemcpyAsync(got, sizes, 16, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "fit plan")) return rc;
  if (got[0] > max_refs || got[1] > n) return eng_fail(e, SIMMR_ENODEV, "fit plan: %llu reference k-mers and %llu pairs from %llu entries", got[0], got[1], n_live);
  simmr_fit_info f{};
  f.n_ref_kmers = got[0];
  f.n_pairs = got[1];
  f.n_positions = n_pos;
  f.n_length_bins = s->len.lo.size();
  f.n_insert_bins = s->ins.lo.size();
  f.n_reads = s->len.n;
  f.n_inserts = s->ins.n;
  f.length_bin_width = s->len.width;
  f.insert_bin_width = s->ins.width;
  f.read_length_mean = s->len.mean;
  f.read_length_std = s->len.sd;
  f.insert_size_mean = s->ins.mean;
  f.insert_size_std = s->ins.sd;
  f.is_long = is_long ? 1u : 0u;
  f.k = s->k;
  f.max_alt_kmers = s->max_alt;
  s->info = f;
  *info = f;
  s->dirty_pos = std::max(s->dirty_pos, n_pos);
  s->unplanned_add = false;
  s->planned = true;
  return SIMMR_OK;
}

int simmr_fit_emit(simmr_engine* e, const simmr_fit_out* out) {
  if (!e) return SIMMR_EINVAL;
  if (!out) return eng_fail(e, SIMMR_EINVAL, "simmr_fit_emit: NULL argument");
  FitState* s = fit_state(e, false);
  if (!s || !s->ready || !s->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_fit_emit called without a simmr_fit_plan for the reads added");
  const simmr_fit_info& f = s->info;
  if (((out->kmer_ref || out->kmer_first) && out->ref_capacity < f.n_ref_kmers) ||
      ((out->pair_alt || out->pair_count || out->pair_prob) && out->pair_capacity < f.n_pairs) ||
      ((out->qual_hist || out->qual_density) && out->position_capacity < f.n_positions) ||
      ((out->length_density || out->length_lo || out->length_hi) && out->length_bin_capacity < f.n_length_bins) ||
      ((out->insert_density || out->insert_lo || out->insert_hi) && out->insert_bin_capacity < f.n_insert_bins))
    return eng_fail(e, SIMMR_ERANGE, "simmr_fit_emit: a capacity is below the planned size (%llu reference k-mers, %llu pairs, %llu positions, "
                                     "%llu length bins, %llu insert bins)",
                    (unsigned long long)f.n_ref_kmers, (unsigned long long)f.n_pairs, (unsigned long long)f.n_positions,
                    (unsigned long long)f.n_length_bins, (unsigned long long)f.n_insert_bins);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
#define FIT_H2D(dst, vec) \
  if ((dst) && !(vec).empty()) HIP_TRY(e, hipMemcpyAsync((dst), (vec).data(), (vec).size() * sizeof((vec)[0]), hipMemcpyHostToDevice, st))
#define FIT_D2D(dst, src, bytes) \
  if ((dst) && (bytes)) HIP_TRY(e, hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToDevice, st))
  FIT_H2D(out->length_lo, s->len.lo);
  FIT_H2D(out->length_hi, s->len.hi);
  FIT_H2D(out->insert_lo, s->ins.lo);
  FIT_H2D(out->insert_hi, s->ins.hi);
  FIT_D2D(out->kmer_ref, s->kmer_ref.p, f.n_ref_kmers * 4);
  FIT_D2D(out->kmer_first, s->kmer_first.p, (f.n_ref_kmers + 1) * 8);
  FIT_D2D(out->pair_alt, s->pair_alt.p, f.n_pairs * 4);
  FIT_D2D(out->pair_count, s->pair_count.p, f.n_pairs * 8);
  FIT_D2D(out->pair_prob, s->pair_prob.p, f.n_pairs * 4);
  FIT_D2D(out->qual_hist, s->qhist(), f.n_positions * SIMMR_FIT_QUALS * 8);
  FIT_D2D(out->qual_density, s->qdens.p, f.n_positions * SIMMR_FIT_DENSITIES * 8);
  FIT_D2D(out->length_hist, s->lhist(), FitState::L_WORDS * 8);
  FIT_D2D(out->insert_hist, s->ihist(), FitState::I_WORDS * 8);
  FIT_D2D(out->length_density, s->ldens.p, f.n_length_bins * 8);
  FIT_D2D(out->insert_density, s->idens.p, f.n_insert_bins * 8);
#undef FIT_H2D
#undef FIT_D2D
  return sync_check(e, "fit emit");  // (the host vectors must outlive the copies)
}

int simmr_last_fit_ms(simmr_engine* e, float* ms) {
  if (!e || !ms) return SIMMR_EINVAL;
  FitState* s = fit_state(e, false);
  if (!s || !s->sp.valid[0]) return eng_fail(e, SIMMR_ESTATE, "no simmr_fit_add yet");
  return s->sp.total_ms(e, "fit", ms);
}

}  // extern "C"
