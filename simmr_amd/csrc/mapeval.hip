// mapeval.hip — an aligner's SAM scored against the true alignments (include/simmr_hip.h: simmr_mapeval_*): the entry points over
// mapeval_kernels.hip, on the scaffold of scorer_host.hpp (the object, the text check, the line index, the names, the pair sort).
// Its time is its own: a growing list of spans, one per call, so that the sum is the calls' alone.
//
// truth_add:  enqueue-only, so nothing is sized from what the text holds.  The index buffers are sized from n_bytes (a line start
//             per two bytes), the entry columns from the bytes of every truth add since the reset (an entry per MEV_MIN_LINE
//             bytes); a column that has to grow keeps what it holds.  index (count) -> scan -> index (write) -> truth.
// truth_plan: reads the cursor and the largest key, copies the keys to the sort's ping, sorts over the bits of the largest key,
//             gathers the columns into key order and checks the neighbours; zeroes the aligned side.
// add:        index (count) -> scan -> index (write) -> record.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "mapeval_kernels.hip"
#include "sam_names.hpp"
#include "scorer_host.hpp"

using namespace simmr;

namespace {

struct Span { hipEvent_t a = nullptr, b = nullptr; };

}  // namespace

struct simmr_mapeval {
  simmr_engine* e = nullptr;
  DeviceNames rnames;
  uint32_t n_names = 0, min_pct = 10;
  LineIndex index;  // of one add
  // the truth: the entries as appended (u_*), and in key order (s_*, with the sorted keys in skey)
  DevBuf u_key, u_meta, u_lo, u_hi, s_meta, s_lo, s_hi;
  PairSort order;
  DevBuf cursor;   // [0] entries, [1] the largest key
  DevBuf counts;   // MC_COUNT words, then by_mapq's 512
  DevBuf word;     // the error word
  DevBuf best, hits;
  const uint64_t* skey = nullptr;
  uint64_t entry_cap = 0;   // entries the truth adds since the reset may have appended
  uint64_t n_entries = 0;
  bool reset_once = false, planned = false;
  std::vector<Span> spans;
  float done_ms = 0.f;

  MevNames names() const { return rnames.names(n_names); }
  unsigned long long* counts_p() const { return counts.as<unsigned long long>(); }
  void drop_spans() {
    for (Span& s : spans) {
      if (s.a) (void)hipEventDestroy(s.a);
      if (s.b) (void)hipEventDestroy(s.b);
    }
    spans.clear();
  }
  ~simmr_mapeval() { drop_spans(); }  // (the list grows and is let go span by span: its events are not an Events set)
};

namespace {

constexpr size_t COUNT_WORDS = MC_COUNT + 512u;

int begin_span(simmr_mapeval* h, hipStream_t st) {
  simmr_engine* e = h->e;
  if (h->spans.size() >= 256u) {  // a caller that never asks for the time: the spans that have ended are summed and let go
    size_t kept = 0;
    for (Span& s : h->spans) {
      float one = 0.f;
      if (s.b && hipEventQuery(s.b) == hipSuccess && hipEventElapsedTime(&one, s.a, s.b) == hipSuccess) {
        h->done_ms += one;
        (void)hipEventDestroy(s.a);
        (void)hipEventDestroy(s.b);
      } else {
        h->spans[kept++] = s;
      }
    }
    (void)hipGetLastError();
    h->spans.resize(kept);
  }
  Span s;
  HIP_TRY(e, hipEventCreate(&s.a));
  h->spans.push_back(s);
  HIP_TRY(e, hipEventCreate(&h->spans.back().b));
  HIP_TRY(e, hipEventRecord(h->spans.back().a, st));
  return SIMMR_OK;
}

int check_add(simmr_mapeval* h, const uint8_t* text, uint64_t n_bytes, const char* who) {
  return check_add_text(h->e, h->reset_once, text, n_bytes, SIMMR_FIT_SAM_MAX_BYTES, who, "simmr_mapeval_reset", "cut the text at a line's end");
}

// the line index of text[0, n_bytes) into the object's buffers (n_bytes > 0)
int enqueue_index(simmr_mapeval* h, const uint8_t* text, uint64_t n_bytes, hipStream_t st, MevText* W, uint32_t* rec_grid) {
  simmr_engine* e = h->e;
  const uint64_t n_tiles = (n_bytes + FSAM_TILE - 1) / FSAM_TILE, start_cap = n_bytes / 2 + 1;
  if (!h->index.room(n_tiles, start_cap))
    return eng_fail(e, SIMMR_ENOMEM, "mapeval line index: allocation failed for %llu bytes of text", (unsigned long long)n_bytes);
  const uint32_t cus = (uint32_t)std::max(eng_cu_count(e), 1);
  *rec_grid = (uint32_t)std::min<uint64_t>(n_bytes / (MEV_WG_RECS * MEV_MIN_LINE) + 1, (uint64_t)cus * 8u);
  h->index.enqueue(st, k_mev_index, k_mev_scan, text, n_bytes, FSAM_TILE, (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)cus * 16u), start_cap, W);
  return SIMMR_OK;
}

int end_span(simmr_mapeval* h, hipStream_t st, const char* what) {
  simmr_engine* e = h->e;
  HIP_TRY(e, hipEventRecord(h->spans.back().b, st));
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "%s launch failed: %s", what, hipGetErrorString(rc));
  return SIMMR_OK;
}

}  // namespace

extern "C" {

int simmr_mapeval_create(simmr_engine* e, simmr_mapeval** out) { return scorer_create(e, out, "simmr_mapeval_create"); }

void simmr_mapeval_destroy(simmr_mapeval* h) { scorer_destroy(h); }

int simmr_mapeval_reset(simmr_mapeval* h, const simmr_mapeval_config* cfg) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!cfg || (cfg->n_names > 0 && !cfg->rname)) return eng_fail(e, SIMMR_EINVAL, "simmr_mapeval_reset: NULL argument");
  if (cfg->min_overlap_pct > 100u) return eng_fail(e, SIMMR_EINVAL, "simmr_mapeval_reset: min_overlap_pct is 1 .. 100 (0: the default, 10)");
  if (cfg->n_names > (1u << 24)) return eng_fail(e, SIMMR_ERANGE, "simmr_mapeval_reset: %u names (at most 2^24)", cfg->n_names);
  SortedNames sorted;
  if (int rc = sorted_names(e, cfg->rname, cfg->n_names, SAM_RNAME_MAX, rname_legal, "reference name", nullptr, &sorted)) return rc;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = sync_check(e, "mapeval reset")) return rc;
  h->planned = false;
  h->reset_once = false;
  h->drop_spans();
  h->done_ms = 0.f;
  if (!h->rnames.room(sorted) || !h->cursor.ensure(16) || !h->counts.ensure(COUNT_WORDS * 8) ||
      !h->word.ensure(16))
    return eng_fail(e, SIMMR_ENOMEM, "mapeval reset: allocation failed");
  hipStream_t st = eng_stream(e);
  if (int rc = h->rnames.upload(e, sorted, st)) return rc;
  HIP_TRY(e, hipMemsetAsync(h->cursor.p, 0, 16, st));
  HIP_TRY(e, hipMemsetAsync(h->counts.p, 0, COUNT_WORDS * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->word.p, 0, 16, st));
  if (int rc = sync_check(e, "mapeval reset")) return rc;  // (the uploads read host vectors that end here)
  h->n_names = cfg->n_names;
  h->min_pct = cfg->min_overlap_pct ? cfg->min_overlap_pct : 10u;
  h->entry_cap = 0;
  h->n_entries = 0;
  h->reset_once = true;
  return SIMMR_OK;
}

int simmr_mapeval_truth_add(simmr_mapeval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_mapeval_truth_add")) return rc;
  h->planned = false;
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t cap = h->entry_cap + n_bytes / MEV_MIN_LINE + 1, held = h->entry_cap;
  if (!h->u_key.grow_keep(cap * 8, held * 8, st) || !h->u_meta.grow_keep(cap * 4, held * 4, st) || !h->u_lo.grow_keep(cap * 8, held * 8, st) ||
      !h->u_hi.grow_keep(cap * 8, held * 8, st))
    return eng_fail(e, SIMMR_ENOMEM, "mapeval truth: allocation failed for %llu entries", (unsigned long long)cap);
  h->entry_cap = cap;
  if (int rc = begin_span(h, st)) return rc;
  MevText W;
  uint32_t rec_grid = 1;
  if (int rc = enqueue_index(h, text, n_bytes, st, &W, &rec_grid)) return rc;
  const MevEntries U{h->u_key.as<uint64_t>(), h->u_meta.as<uint32_t>(), h->u_lo.as<uint64_t>(), h->u_hi.as<uint64_t>()};
  hipLaunchKernelGGL(k_mev_truth, dim3(rec_grid), dim3(MEV_WG), 0, st, W, h->names(), U, cap, h->cursor.as<unsigned long long>(), h->counts_p(),
                     h->word.as<uint32_t>());
  return end_span(h, st, "mapeval truth add");
}

int simmr_mapeval_truth_plan(simmr_mapeval* h, uint64_t* n_entries) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_mapeval_truth_plan called before simmr_mapeval_reset");
  h->planned = false;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  uint64_t cur2[2] = {0, 0};
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(cur2, h->cursor.p, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "mapeval truth adds")) return rc;
  if (errw & MEV_ERR_TRUTH)
    return eng_fail(e, SIMMR_EINVAL, "a malformed truth record: fewer than 11 fields, a bad FLAG / POS / MAPQ / CIGAR, a QNAME that is no read id, an RNAME "
                                     "outside the names, or a POS of 0");
  const uint64_t n = std::min(cur2[0], h->entry_cap);
  if (n >= (1ull << 31)) return eng_fail(e, SIMMR_ERANGE, "simmr_mapeval_truth_plan takes fewer than 2^31 truth entries (%llu given)", (unsigned long long)n);
  const uint64_t n1 = std::max<uint64_t>(n, 1);
  bool room = h->order.room(n1) && h->s_lo.ensure(n1 * 8) && h->s_hi.ensure(n1 * 8);
  for (DevBuf* b : {&h->s_meta, &h->best, &h->hits}) room = room && b->ensure(n1 * 4);
  if (!room) return eng_fail(e, SIMMR_ENOMEM, "mapeval truth plan: allocation failed (%llu entries)", (unsigned long long)n);
  if (int rc = begin_span(h, st)) return rc;
  // the aligned side starts over: its counts (the words behind the truth's four), by_mapq, best and hits
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + MC_LINES, 0, (COUNT_WORDS - MC_LINES) * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->best.p, 0, n1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->hits.p, 0, n1 * 4, st));
  h->skey = h->order.key[0].as<const uint64_t>();
  if (n > 0) {
    HIP_TRY(e, hipMemcpyAsync(h->order.key[0].p, h->u_key.p, n * 8, hipMemcpyDeviceToDevice, st));
    const PairSort::Sorted by_key = h->order.sort(st, n, bits_of(cur2[1]));
    h->skey = by_key.keys;
    const MevEntries U{h->u_key.as<uint64_t>(), h->u_meta.as<uint32_t>(), h->u_lo.as<uint64_t>(), h->u_hi.as<uint64_t>()};
    const MevEntries S{nullptr, h->s_meta.as<uint32_t>(), h->s_lo.as<uint64_t>(), h->s_hi.as<uint64_t>()};
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)std::max(eng_cu_count(e), 1) * 32u);
    hipLaunchKernelGGL(k_mev_gather, dim3(grid), dim3(256), 0, st, h->skey, by_key.perm, U, S, n, h->word.as<uint32_t>());
  }
  if (int rc = end_span(h, st, "mapeval truth plan")) return rc;
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "mapeval truth plan")) return rc;
  if (errw & MEV_ERR_DUP) {
    uint32_t cleared = errw & ~MEV_ERR_DUP;  // (the entries stay; the flag is the plan's alone)
    HIP_TRY(e, hipMemcpy(h->word.p, &cleared, 4, hipMemcpyHostToDevice));
    return eng_fail(e, SIMMR_EINVAL, "two truth records have one read id and mate: the key of an entry is unique");
  }
  h->n_entries = n;
  h->planned = true;
  if (n_entries) *n_entries = n;
  return SIMMR_OK;
}

int simmr_mapeval_add(simmr_mapeval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_mapeval_add")) return rc;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_mapeval_add called without a simmr_mapeval_truth_plan in force");
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (int rc = begin_span(h, st)) return rc;
  MevText W;
  uint32_t rec_grid = 1;
  if (int rc = enqueue_index(h, text, n_bytes, st, &W, &rec_grid)) return rc;
  const MevEntries S{nullptr, h->s_meta.as<uint32_t>(), h->s_lo.as<uint64_t>(), h->s_hi.as<uint64_t>()};
  hipLaunchKernelGGL(k_mev_record, dim3(rec_grid), dim3(MEV_WG), 0, st, W, h->names(), h->skey, S, h->n_entries, h->min_pct, h->counts_p(),
                     h->counts_p() + MC_COUNT, h->best.as<uint32_t>(), h->hits.as<uint32_t>(), h->word.as<uint32_t>());
  return end_span(h, st, "mapeval add");
}

int simmr_mapeval_read(simmr_mapeval* h, simmr_mapeval_counts* counts, uint64_t* by_mapq_host) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_mapeval_read called before simmr_mapeval_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + MC_MISSING, 0, 5 * 8, st));
  if (h->planned && h->n_entries > 0) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((h->n_entries + 255) / 256, (uint64_t)std::max(eng_cu_count(e), 1) * 16u);
    hipLaunchKernelGGL(k_mev_reduce, dim3(grid), dim3(256), 0, st, h->best.as<const uint32_t>(), h->hits.as<const uint32_t>(), h->n_entries, h->counts_p());
  }
  std::vector<uint64_t> host(COUNT_WORDS);
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(host.data(), h->counts.p, COUNT_WORDS * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "mapeval read")) return rc;
  if (errw & (MEV_ERR_TRUTH | MEV_ERR_ALIGNED))
    return eng_fail(e, SIMMR_EINVAL, "a malformed %s record: fewer than 11 fields, a bad FLAG / POS / MAPQ / CIGAR, or a POS of 0 where the record is mapped",
                    errw & MEV_ERR_TRUTH ? "truth" : "aligned");
  if (counts) std::memcpy(counts, host.data(), sizeof(*counts));
  if (by_mapq_host) std::memcpy(by_mapq_host, host.data() + MC_COUNT, 512 * 8);
  return SIMMR_OK;
}

int simmr_mapeval_emit(simmr_mapeval* h, uint64_t* key_dev, uint32_t* best_dev, uint32_t* hits_dev, uint64_t capacity) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_mapeval_emit called without a simmr_mapeval_truth_plan in force");
  if (capacity < h->n_entries)
    return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu truth entries", (unsigned long long)capacity, (unsigned long long)h->n_entries);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (h->n_entries > 0) {
    if (key_dev) HIP_TRY(e, hipMemcpyAsync(key_dev, h->skey, h->n_entries * 8, hipMemcpyDeviceToDevice, st));
    if (best_dev) HIP_TRY(e, hipMemcpyAsync(best_dev, h->best.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
    if (hits_dev) HIP_TRY(e, hipMemcpyAsync(hits_dev, h->hits.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
  }
  return sync_check(e, "mapeval emit");
}

int simmr_last_mapeval_ms(simmr_mapeval* h, float* ms) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!ms) return eng_fail(e, SIMMR_EINVAL, "simmr_last_mapeval_ms: NULL ms");
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_mapeval_reset yet");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = sync_check(e, "mapeval")) return rc;
  for (const Span& s : h->spans) {
    float one = 0.f;
    if (s.a && s.b && hipEventElapsedTime(&one, s.a, s.b) == hipSuccess) h->done_ms += one;
    else (void)hipGetLastError();
  }
  h->drop_spans();
  *ms = h->done_ms;
  return SIMMR_OK;
}

}  // extern "C"
