// vcfeval.hip — a variant caller's VCF scored against the strain's sites (include/simmr_hip.h: simmr_vcfeval_*): the entry points
// over vcfeval_kernels.hip, on the scaffold of scorer_host.hpp.  The contig names are held as mapeval.hip holds its names.
//
// truth_add:  enqueue-only, so nothing is sized from what the text holds.  The index buffers are sized from n_bytes (a line start
//             per two bytes), the entry columns from the bytes of every truth add since the reset (an entry per VCE_MIN_LINE
//             bytes); a column that has to grow keeps what it holds.  index (count) -> scan -> index (write) -> truth.
// truth_plan: reads the cursor and the largest key, copies the keys to the sort's ping, sorts over the bits of the largest key,
//             gathers the columns into key order and checks the neighbours; zeroes the candidate side.
// add:        index (count) -> scan -> index (write) -> record.
// Time: the adds' span and the plan's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "host_support.hpp"
#include "vcfeval_kernels.hip"
#include "sam_names.hpp"
#include "scorer_host.hpp"

using namespace simmr;

namespace {

enum { SPAN_ADDS = 0, SPAN_PLAN = 1, SPAN_COUNT = 2 };
constexpr size_t QUAL_WORDS = 2u * VCE_QUAL_ROWS, AD_WORDS = 2u * VCE_AD_ROWS;
constexpr size_t COUNT_WORDS = VC_COUNT + QUAL_WORDS + AD_WORDS;  // the counts, by_qual, by_ad

const char* const MALFORMED =
    "fewer than 8 fields, a POS that is no number of 1 to 18 digits, is 0 or above 2^40, a REF that is empty or has a byte outside ACGTNacgtn, an "
    "empty ALT, a QUAL that is neither '.' nor a decimal number";

}  // namespace

struct simmr_vcfeval {
  simmr_engine* e = nullptr;
  DeviceNames rnames;
  uint32_t n_names = 0, use_filtered = 0;
  LineIndex index;  // of one add
  // the truth: the entries as appended (u_*), and in key order (s_*, with the sorted keys in skey)
  DevBuf u_key, u_alleles, u_ad, s_alleles, s_ad;
  PairSort order;
  DevBuf cursor;   // [0] entries, [1] the largest key
  DevBuf counts;   // VC_COUNT words, then by_qual's 512 and by_ad's 66
  DevBuf word;     // the error word
  DevBuf best, hits;
  const uint64_t* skey = nullptr;
  uint64_t entry_cap = 0;   // entries the truth adds since the reset may have appended
  uint64_t n_entries = 0;
  bool reset_once = false, planned = false;
  FoldedSpans<SPAN_COUNT> sp;

  MevNames names() const { return rnames.names(n_names); }
  VceEntries appended() const { return VceEntries{u_key.as<uint64_t>(), u_alleles.as<uint32_t>(), u_ad.as<uint32_t>()}; }
  VceEntries sorted() const { return VceEntries{nullptr, s_alleles.as<uint32_t>(), s_ad.as<uint32_t>()}; }
  unsigned long long* counts_p() const { return counts.as<unsigned long long>(); }
};

namespace {

int check_add(simmr_vcfeval* h, const uint8_t* text, uint64_t n_bytes, const char* who) {
  return check_add_text(h->e, h->reset_once, text, n_bytes, SIMMR_FIT_SAM_MAX_BYTES, who, "simmr_vcfeval_reset", "cut the text at a line's end");
}

// the line index of text[0, n_bytes) into the object's buffers (n_bytes > 0)
int enqueue_index(simmr_vcfeval* h, const uint8_t* text, uint64_t n_bytes, hipStream_t st, MevText* W, uint32_t* rec_grid) {
  simmr_engine* e = h->e;
  const uint64_t n_tiles = (n_bytes + FSAM_TILE - 1) / FSAM_TILE, start_cap = n_bytes / 2 + 1;
  if (!h->index.room(n_tiles, start_cap))
    return eng_fail(e, SIMMR_ENOMEM, "vcfeval line index: allocation failed for %llu bytes of text", (unsigned long long)n_bytes);
  const uint32_t cus = (uint32_t)std::max(eng_cu_count(e), 1);
  *rec_grid = (uint32_t)std::min<uint64_t>(n_bytes / (VCE_WG_RECS * VCE_MIN_LINE) + 1, (uint64_t)cus * 8u);
  h->index.enqueue(st, k_vce_index, k_vce_scan, text, n_bytes, FSAM_TILE, (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)cus * 16u), start_cap, W);
  return SIMMR_OK;
}

}  // namespace

extern "C" {

int simmr_vcfeval_create(simmr_engine* e, simmr_vcfeval** out) { return scorer_create(e, out, "simmr_vcfeval_create"); }

void simmr_vcfeval_destroy(simmr_vcfeval* h) { scorer_destroy(h); }

int simmr_vcfeval_reset(simmr_vcfeval* h, const simmr_vcfeval_config* cfg) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!cfg || (cfg->n_names > 0 && !cfg->rname)) return eng_fail(e, SIMMR_EINVAL, "simmr_vcfeval_reset: NULL argument");
  if (cfg->n_names > (1u << 24)) return eng_fail(e, SIMMR_ERANGE, "simmr_vcfeval_reset: %u names (at most 2^24)", cfg->n_names);
  SortedNames sorted;
  if (int rc = sorted_names(e, cfg->rname, cfg->n_names, SAM_RNAME_MAX, rname_legal, "contig name", nullptr, &sorted)) return rc;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = sync_check(e, "vcfeval reset")) return rc;
  h->planned = false;
  h->reset_once = false;
  if (int rc = h->sp.reset(e)) return rc;
  if (!h->rnames.room(sorted) || !h->cursor.ensure(16) || !h->counts.ensure(COUNT_WORDS * 8) ||
      !h->word.ensure(16))
    return eng_fail(e, SIMMR_ENOMEM, "vcfeval reset: allocation failed");
  hipStream_t st = eng_stream(e);
  if (int rc = h->rnames.upload(e, sorted, st)) return rc;
  HIP_TRY(e, hipMemsetAsync(h->cursor.p, 0, 16, st));
  HIP_TRY(e, hipMemsetAsync(h->counts.p, 0, COUNT_WORDS * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->word.p, 0, 16, st));
  if (int rc = sync_check(e, "vcfeval reset")) return rc;  // (the uploads read host vectors that end here)
  h->n_names = cfg->n_names;
  h->use_filtered = cfg->use_filtered ? 1u : 0u;
  h->entry_cap = 0;
  h->n_entries = 0;
  h->reset_once = true;
  return SIMMR_OK;
}

int simmr_vcfeval_truth_add(simmr_vcfeval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_vcfeval_truth_add")) return rc;
  h->planned = false;
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t cap = h->entry_cap + n_bytes / VCE_MIN_LINE + 1, held = h->entry_cap;
  if (!h->u_key.grow_keep(cap * 8, held * 8, st) || !h->u_alleles.grow_keep(cap * 4, held * 4, st) || !h->u_ad.grow_keep(cap * 4, held * 4, st))
    return eng_fail(e, SIMMR_ENOMEM, "vcfeval truth: allocation failed for %llu entries", (unsigned long long)cap);
  h->entry_cap = cap;
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  uint32_t rec_grid = 1;
  if (int rc = enqueue_index(h, text, n_bytes, st, &W, &rec_grid)) return rc;
  hipLaunchKernelGGL(k_vce_truth, dim3(rec_grid), dim3(VCE_WG), 0, st, W, h->names(), h->appended(), cap, h->cursor.as<unsigned long long>(),
                     h->counts_p(), h->word.as<uint32_t>());
  return h->sp.end(e, SPAN_ADDS, st, "vcfeval truth add");
}

int simmr_vcfeval_truth_plan(simmr_vcfeval* h, uint64_t* n_entries) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_vcfeval_truth_plan called before simmr_vcfeval_reset");
  h->planned = false;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  uint64_t cur2[2] = {0, 0};
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(cur2, h->cursor.p, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "vcfeval truth adds")) return rc;
  if (int rc = h->sp.fold(e, "vcfeval")) return rc;
  if (errw & VCE_ERR_TRUTH)
    return eng_fail(e, SIMMR_EINVAL, "a malformed truth record: %s, a REF or ALT that is not one base of ACGT, REF equal to ALT, a CHROM outside the names, or "
                                     "an AD= item that is not two numbers", MALFORMED);
  const uint64_t n = std::min(cur2[0], h->entry_cap);
  if (n >= (1ull << 31)) return eng_fail(e, SIMMR_ERANGE, "simmr_vcfeval_truth_plan takes fewer than 2^31 truth entries (%llu given)", (unsigned long long)n);
  const uint64_t n1 = std::max<uint64_t>(n, 1);
  bool room = h->order.room(n1);
  for (DevBuf* b : {&h->s_alleles, &h->s_ad, &h->best, &h->hits}) room = room && b->ensure(n1 * 4);
  if (!room) return eng_fail(e, SIMMR_ENOMEM, "vcfeval truth plan: allocation failed (%llu entries)", (unsigned long long)n);
  if (int rc = h->sp.begin(e, SPAN_PLAN, st)) return rc;
  // the candidate side starts over: its counts (the words behind the truth's three), by_qual, by_ad, best and hits
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + VC_LINES, 0, (COUNT_WORDS - VC_LINES) * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->best.p, 0, n1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->hits.p, 0, n1 * 4, st));
  h->skey = h->order.key[0].as<const uint64_t>();
  if (n > 0) {
    HIP_TRY(e, hipMemcpyAsync(h->order.key[0].p, h->u_key.p, n * 8, hipMemcpyDeviceToDevice, st));
    const PairSort::Sorted by_key = h->order.sort(st, n, bits_of(cur2[1]));
    h->skey = by_key.keys;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)std::max(eng_cu_count(e), 1) * 32u);
    hipLaunchKernelGGL(k_vce_gather, dim3(grid), dim3(256), 0, st, h->skey, by_key.perm, h->appended(), h->sorted(), n, h->word.as<uint32_t>());
  }
  if (int rc = h->sp.end(e, SPAN_PLAN, st, "vcfeval truth plan")) return rc;
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "vcfeval truth plan")) return rc;
  if (errw & VCE_ERR_DUP) {
    uint32_t cleared = errw & ~VCE_ERR_DUP;  // (the entries stay; the flag is the plan's alone)
    HIP_TRY(e, hipMemcpy(h->word.p, &cleared, 4, hipMemcpyHostToDevice));
    return eng_fail(e, SIMMR_EINVAL, "two truth records name one position of one contig: the key of an entry is unique");
  }
  h->n_entries = n;
  h->planned = true;
  if (int rc = h->sp.fold(e, "vcfeval")) return rc;
  if (n_entries) *n_entries = n;
  return SIMMR_OK;
}

int simmr_vcfeval_add(simmr_vcfeval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_vcfeval_add")) return rc;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_vcfeval_add called without a simmr_vcfeval_truth_plan in force");
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  uint32_t rec_grid = 1;
  if (int rc = enqueue_index(h, text, n_bytes, st, &W, &rec_grid)) return rc;
  hipLaunchKernelGGL(k_vce_record, dim3(rec_grid), dim3(VCE_WG), 0, st, W, h->names(), h->skey, h->s_alleles.as<const uint32_t>(), h->n_entries,
                     h->use_filtered, h->counts_p(), h->best.as<uint32_t>(), h->hits.as<uint32_t>(), h->word.as<uint32_t>());
  return h->sp.end(e, SPAN_ADDS, st, "vcfeval add");
}

int simmr_vcfeval_read(simmr_vcfeval* h, simmr_vcfeval_counts* counts, uint64_t* by_qual_host, uint64_t* by_ad_host) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_vcfeval_read called before simmr_vcfeval_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + VC_SITES_FOUND, 0, (VC_COUNT - VC_SITES_FOUND) * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + VC_COUNT + QUAL_WORDS, 0, AD_WORDS * 8, st));
  if (h->planned && h->n_entries > 0) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((h->n_entries + 255) / 256, (uint64_t)std::max(eng_cu_count(e), 1) * 16u);
    hipLaunchKernelGGL(k_vce_reduce, dim3(grid), dim3(256), 0, st, h->best.as<const uint32_t>(), h->hits.as<const uint32_t>(), h->s_ad.as<const uint32_t>(),
                       h->n_entries, h->counts_p(), h->counts_p() + VC_COUNT + QUAL_WORDS);
  }
  std::vector<uint64_t> host(COUNT_WORDS);
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(host.data(), h->counts.p, COUNT_WORDS * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "vcfeval read")) return rc;
  if (errw & VCE_ERR_TRUTH) return eng_fail(e, SIMMR_EINVAL, "a malformed truth record: %s, or what a truth record may not hold", MALFORMED);
  if (errw & VCE_ERR_CAND)
    return eng_fail(e, SIMMR_EINVAL, "a malformed candidate record: %s, a GT item that is neither '.' nor a number, or a GT index above the ALT alleles", MALFORMED);
  if (counts) std::memcpy(counts, host.data(), sizeof(*counts));
  if (by_qual_host) std::memcpy(by_qual_host, host.data() + VC_COUNT, QUAL_WORDS * 8);
  if (by_ad_host) std::memcpy(by_ad_host, host.data() + VC_COUNT + QUAL_WORDS, AD_WORDS * 8);
  return SIMMR_OK;
}

int simmr_vcfeval_emit(simmr_vcfeval* h, uint64_t* key_dev, uint32_t* alleles_dev, uint32_t* ad_dev, uint32_t* best_dev, uint32_t* hits_dev,
                       uint64_t capacity) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_vcfeval_emit called without a simmr_vcfeval_truth_plan in force");
  if (capacity < h->n_entries)
    return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu truth entries", (unsigned long long)capacity, (unsigned long long)h->n_entries);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (h->n_entries > 0) {
    if (key_dev) HIP_TRY(e, hipMemcpyAsync(key_dev, h->skey, h->n_entries * 8, hipMemcpyDeviceToDevice, st));
    if (alleles_dev) HIP_TRY(e, hipMemcpyAsync(alleles_dev, h->s_alleles.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
    if (ad_dev) HIP_TRY(e, hipMemcpyAsync(ad_dev, h->s_ad.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
    if (best_dev) HIP_TRY(e, hipMemcpyAsync(best_dev, h->best.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
    if (hits_dev) HIP_TRY(e, hipMemcpyAsync(hits_dev, h->hits.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
  }
  return sync_check(e, "vcfeval emit");
}

int simmr_last_vcfeval_ms(simmr_vcfeval* h, float* ms) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!ms) return eng_fail(e, SIMMR_EINVAL, "simmr_last_vcfeval_ms: NULL ms");
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_vcfeval_reset yet");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  return h->sp.last_ms(e, "vcfeval", ms);
}

}  // extern "C"
