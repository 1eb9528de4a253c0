// ovleval.hip — an overlapper's PAF scored against the true overlaps (include/simmr_hip.h: simmr_ovleval_*): the entry points over
// ovleval_kernels.hip.  A translation unit of libsimmr_hip.so of its own; it sees an engine through engine_internal.hpp only.  The
// engine's slot enum is full, so the state lives in an object of its own that the caller creates on an engine and destroys before
// the engine, as mapeval.hip's does.  The sort is sam_sort.hip's (samsort_sort_pairs), run twice by the plan.
//
// truth_add:  enqueue-only, so nothing is sized from what the text holds.  The index buffers are sized from n_bytes (a line start
//             per two bytes), the entry columns from the bytes of every truth add since the reset (an entry per OVE_MIN_LINE
//             bytes); a column that has to grow keeps what it holds.  index (count) -> scan -> index (write) -> truth.
// truth_plan: reads the cursor and the largest key; sorts the 2 n keys, counts the heads per tile, scans, writes the distinct keys
//             and the ranks; reads the number of distinct keys; makes the entry keys from the ranks, sorts them, gathers the
//             columns into that order and checks the neighbours; zeroes the candidate side.
// add:        index (count) -> scan -> index (write) -> record.
// Time: two spans.  The adds of either side only enqueue: the first begins the span of the adds and every one ends it anew, so a
// run of adds is one span.  A call that synchronises anyway (the plan, simmr_last_ovleval_ms) moves the spans that count into a
// sum and closes them; the plan has a span of its own, so no stretch of the stream is counted twice.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "host_support.hpp"
#include "ovleval_kernels.hip"

using namespace simmr;

namespace {

uint32_t bits_of(uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }

enum { SPAN_ADDS = 0, SPAN_PLAN = 1, SPAN_COUNT = 2 };
constexpr size_t COUNT_WORDS = OC_COUNT + 2u * OVE_LEN_ROWS;

}  // namespace

struct simmr_ovleval {
  simmr_engine* e = nullptr;
  uint32_t min_pct = 10;
  // the line index of one add
  DevBuf tile_sum, tile_prefix, starts;
  // the truth: the entries as appended (u_*), and in pair order (s_*, with the sorted entry keys in key[cur])
  DevBuf u_keys, u_lo_s, u_lo_e, u_hi_s, u_hi_e, u_ov;
  DevBuf s_ka, s_kb, s_lo_s, s_lo_e, s_hi_s, s_hi_e, s_ov;
  DevBuf key[2], idx[2], hist, digit_total;
  DevBuf head_sum, head_prefix, uniq, rk;
  DevBuf cursor;   // [0] entries, [1] the largest key
  DevBuf counts;   // OC_COUNT words, then by_len's 82
  DevBuf word;     // the error word
  DevBuf best, hits;
  const uint64_t* skey = nullptr;
  uint64_t entry_cap = 0;   // entries the truth adds since the reset may have appended
  uint64_t n_entries = 0, n_reads = 0;
  bool reset_once = false, planned = false;
  Spans<SPAN_COUNT> sp;
  bool open = false;  // the span of the adds has begun and is not folded yet
  float done_ms = 0.f;

  OveEntries appended() const {
    return OveEntries{u_keys.as<uint64_t>(), nullptr, nullptr, u_lo_s.as<uint64_t>(), u_lo_e.as<uint64_t>(), u_hi_s.as<uint64_t>(), u_hi_e.as<uint64_t>(),
                      u_ov.as<uint64_t>()};
  }
  OveEntries sorted() const {
    return OveEntries{nullptr, s_ka.as<uint64_t>(), s_kb.as<uint64_t>(), s_lo_s.as<uint64_t>(), s_lo_e.as<uint64_t>(), s_hi_s.as<uint64_t>(),
                      s_hi_e.as<uint64_t>(), s_ov.as<uint64_t>()};
  }
  unsigned long long* counts_p() const { return counts.as<unsigned long long>(); }
};

namespace {

int check_text(simmr_ovleval* h, const uint8_t* text, uint64_t n_bytes, const char* who) {
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "%s called before simmr_ovleval_reset", who);
  if (!text && n_bytes > 0) return eng_fail(e, SIMMR_EINVAL, "%s: NULL text", who);
  if (n_bytes > SIMMR_FIT_SAM_MAX_BYTES)
    return eng_fail(e, SIMMR_ENOTSUP, "%s: %llu bytes in one add (at most %llu: cut the text at a line's end)", who, (unsigned long long)n_bytes,
                    (unsigned long long)SIMMR_FIT_SAM_MAX_BYTES);
  return SIMMR_OK;
}

// the span `which` runs from here, unless it is the adds' and open already
int begin_span(simmr_ovleval* h, int which, hipStream_t st) {
  if (which == SPAN_ADDS && h->open) return SIMMR_OK;
  HIP_TRY(h->e, h->sp.begin(which, st));
  return SIMMR_OK;
}

// the spans that count into the sum, and closed.  Synchronises.
int fold_spans(simmr_ovleval* h) {
  float now = 0.f;
  if (int rc = h->sp.total_ms(h->e, "ovleval", &now)) return rc;
  h->done_ms += now;
  h->sp.invalidate_from(0);
  h->open = false;
  return SIMMR_OK;
}

// ... and ends behind what was enqueued; a launch that failed leaves the span as it was
int end_span(simmr_ovleval* h, int which, hipStream_t st, const char* what) {
  simmr_engine* e = h->e;
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "%s launch failed: %s", what, hipGetErrorString(rc));
  HIP_TRY(e, h->sp.end(which, st));
  if (which == SPAN_ADDS) h->open = true;
  h->sp.mark(which);
  return SIMMR_OK;
}

// the line index of text[0, n_bytes) into the object's buffers (n_bytes > 0)
int enqueue_index(simmr_ovleval* h, const uint8_t* text, uint64_t n_bytes, hipStream_t st, MevText* W, uint32_t* rec_grid) {
  simmr_engine* e = h->e;
  const uint64_t n_tiles = (n_bytes + FSAM_TILE - 1) / FSAM_TILE, start_cap = n_bytes / 2 + 1;
  if (!h->tile_sum.ensure(n_tiles * 8) || !h->tile_prefix.ensure((n_tiles + 1) * 8) || !h->starts.ensure(start_cap * 4))
    return eng_fail(e, SIMMR_ENOMEM, "ovleval line index: allocation failed for %llu bytes of text", (unsigned long long)n_bytes);
  const uint32_t cus = (uint32_t)std::max(eng_cu_count(e), 1);
  const uint32_t tile_grid = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)cus * 16u);
  *rec_grid = (uint32_t)std::min<uint64_t>(n_bytes / (OVE_WG_RECS * OVE_MIN_LINE) + 1, (uint64_t)cus * 8u);
  hipLaunchKernelGGL(k_ove_index, dim3(tile_grid), dim3(FSAM_WG), 0, st, text, n_bytes, n_tiles, h->tile_sum.as<uint64_t>(), (const uint64_t*)nullptr,
                     (uint32_t*)nullptr, 0ull);
  hipLaunchKernelGGL(k_ove_scan, dim3(1), dim3(256), 0, st, h->tile_sum.as<const uint64_t>(), h->tile_prefix.as<uint64_t>(), n_tiles);
  hipLaunchKernelGGL(k_ove_index, dim3(tile_grid), dim3(FSAM_WG), 0, st, text, n_bytes, n_tiles, h->tile_sum.as<uint64_t>(),
                     h->tile_prefix.as<const uint64_t>(), h->starts.as<uint32_t>(), start_cap);
  *W = MevText{text, n_bytes, h->tile_prefix.as<const uint64_t>() + n_tiles, h->starts.as<const uint32_t>()};
  return SIMMR_OK;
}

}  // namespace

extern "C" {

int simmr_ovleval_create(simmr_engine* e, simmr_ovleval** out) {
  if (!e) return SIMMR_EINVAL;
  if (!out) return eng_fail(e, SIMMR_EINVAL, "simmr_ovleval_create: NULL out");
  *out = nullptr;
  simmr_ovleval* h = new (std::nothrow) simmr_ovleval();
  if (!h) return eng_fail(e, SIMMR_ENOMEM, "simmr_ovleval_create: out of memory");
  h->e = e;
  *out = h;
  return SIMMR_OK;
}

void simmr_ovleval_destroy(simmr_ovleval* h) {
  if (!h) return;
  if (hipSetDevice(eng_device(h->e)) == hipSuccess) (void)hipStreamSynchronize(eng_stream(h->e));
  delete h;  // (its buffers and events go with it)
  (void)hipGetLastError();
}

int simmr_ovleval_reset(simmr_ovleval* h, uint32_t min_pct) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (min_pct > 100u) return eng_fail(e, SIMMR_EINVAL, "simmr_ovleval_reset: min_pct is 1 .. 100 (0: the default, 10)");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = sync_check(e, "ovleval reset")) return rc;
  h->planned = false;
  h->reset_once = false;
  h->sp.invalidate_from(0);
  h->open = false;
  h->done_ms = 0.f;
  if (int rc = h->sp.create_missing(e)) return rc;
  if (!h->cursor.ensure(16) || !h->counts.ensure(COUNT_WORDS * 8) || !h->word.ensure(16)) return eng_fail(e, SIMMR_ENOMEM, "ovleval reset: allocation failed");
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemsetAsync(h->cursor.p, 0, 16, st));
  HIP_TRY(e, hipMemsetAsync(h->counts.p, 0, COUNT_WORDS * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->word.p, 0, 16, st));
  if (int rc = sync_check(e, "ovleval reset")) return rc;
  h->min_pct = min_pct ? min_pct : 10u;
  h->entry_cap = 0;
  h->n_entries = 0;
  h->n_reads = 0;
  h->reset_once = true;
  return SIMMR_OK;
}

int simmr_ovleval_truth_add(simmr_ovleval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_text(h, text, n_bytes, "simmr_ovleval_truth_add")) return rc;
  h->planned = false;
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t cap = h->entry_cap + n_bytes / OVE_MIN_LINE + 1, held = h->entry_cap;
  if (!h->u_keys.grow_keep(cap * 16, held * 16, st)) return eng_fail(e, SIMMR_ENOMEM, "ovleval truth: allocation failed for %llu entries", (unsigned long long)cap);
  for (DevBuf* b : {&h->u_lo_s, &h->u_lo_e, &h->u_hi_s, &h->u_hi_e, &h->u_ov})
    if (!b->grow_keep(cap * 8, held * 8, st)) return eng_fail(e, SIMMR_ENOMEM, "ovleval truth: allocation failed for %llu entries", (unsigned long long)cap);
  h->entry_cap = cap;
  if (int rc = begin_span(h, SPAN_ADDS, st)) return rc;
  MevText W;
  uint32_t rec_grid = 1;
  if (int rc = enqueue_index(h, text, n_bytes, st, &W, &rec_grid)) return rc;
  hipLaunchKernelGGL(k_ove_truth, dim3(rec_grid), dim3(OVE_WG), 0, st, W, h->appended(), cap, h->cursor.as<unsigned long long>(), h->counts_p(),
                     h->word.as<uint32_t>());
  return end_span(h, SPAN_ADDS, st, "ovleval truth add");
}

int simmr_ovleval_truth_plan(simmr_ovleval* h, uint64_t* n_entries, uint64_t* n_reads) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_ovleval_truth_plan called before simmr_ovleval_reset");
  h->planned = false;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  uint64_t cur2[2] = {0, 0};
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(cur2, h->cursor.p, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "ovleval truth adds")) return rc;
  if (int rc = fold_spans(h)) return rc;
  if (errw & OVE_ERR_TRUTH)
    return eng_fail(e, SIMMR_EINVAL, "a malformed truth record: fewer than 12 fields, a length, start, end or field 10 .. 12 that is no number, a strand that "
                                     "is neither + nor -, start <= end <= length < 2^40 broken, a name that is no read id, or one read on both sides");
  const uint64_t n = std::min(cur2[0], h->entry_cap);
  if (n >= (1ull << 30)) return eng_fail(e, SIMMR_ERANGE, "simmr_ovleval_truth_plan takes fewer than 2^30 true pairs (%llu given)", (unsigned long long)n);
  const uint64_t n1 = std::max<uint64_t>(n, 1), n2 = 2 * n, sort_tiles = (n2 + SAMSORT_PAIRS_TILE - 1) / SAMSORT_PAIRS_TILE;
  const uint64_t head_tiles = (n2 + OVE_HEAD_TILE - 1) / OVE_HEAD_TILE;
  bool room = h->hist.ensure(std::max<uint64_t>(sort_tiles, 1) * SAMSORT_PAIRS_DIGITS * 4) && h->digit_total.ensure(SAMSORT_PAIRS_DIGITS * 4) &&
              h->head_sum.ensure(std::max<uint64_t>(head_tiles, 1) * 8) && h->head_prefix.ensure((head_tiles + 1) * 8);
  for (DevBuf* b : {&h->key[0], &h->key[1], &h->uniq}) room = room && b->ensure(2 * n1 * 8);
  for (DevBuf* b : {&h->idx[0], &h->idx[1], &h->rk}) room = room && b->ensure(2 * n1 * 4);
  for (DevBuf* b : {&h->s_ka, &h->s_kb, &h->s_lo_s, &h->s_lo_e, &h->s_hi_s, &h->s_hi_e, &h->s_ov}) room = room && b->ensure(n1 * 8);
  for (DevBuf* b : {&h->best, &h->hits}) room = room && b->ensure(n1 * 4);
  if (!room) return eng_fail(e, SIMMR_ENOMEM, "ovleval truth plan: allocation failed (%llu entries)", (unsigned long long)n);
  if (int rc = begin_span(h, SPAN_PLAN, st)) return rc;
  // the candidate side starts over: its counts (the words behind the truth's three), by_len, best and hits
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + OC_LINES, 0, (COUNT_WORDS - OC_LINES) * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->best.p, 0, n1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->hits.p, 0, n1 * 4, st));
  h->skey = h->key[0].as<const uint64_t>();
  uint64_t reads = 0;
  if (n > 0) {
    uint64_t* const keys[2] = {h->key[0].as<uint64_t>(), h->key[1].as<uint64_t>()};
    uint32_t* const idxs[2] = {h->idx[0].as<uint32_t>(), h->idx[1].as<uint32_t>()};
    const uint32_t cus = (uint32_t)std::max(eng_cu_count(e), 1);
    // the reads: the 2 n keys in order, their heads, the ranks
    HIP_TRY(e, hipMemcpyAsync(h->key[0].p, h->u_keys.p, n2 * 8, hipMemcpyDeviceToDevice, st));
    const uint32_t key_bits = bits_of(cur2[1]);
    int cur = samsort_sort_pairs(st, keys, idxs, h->hist.as<uint32_t>(), h->digit_total.as<uint32_t>(), n2, key_bits);
    const uint32_t* perm = key_bits > 0u ? h->idx[cur].as<const uint32_t>() : (const uint32_t*)nullptr;
    const uint32_t head_grid = (uint32_t)std::min<uint64_t>(head_tiles, (uint64_t)cus * 32u);
    hipLaunchKernelGGL(k_ove_heads, dim3(head_grid), dim3(256), 0, st, h->key[cur].as<const uint64_t>(), perm, n2, head_tiles, h->head_sum.as<uint64_t>(),
                       (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_ove_scan, dim3(1), dim3(256), 0, st, h->head_sum.as<const uint64_t>(), h->head_prefix.as<uint64_t>(), head_tiles);
    hipLaunchKernelGGL(k_ove_heads, dim3(head_grid), dim3(256), 0, st, h->key[cur].as<const uint64_t>(), perm, n2, head_tiles, h->head_sum.as<uint64_t>(),
                       h->head_prefix.as<const uint64_t>(), h->uniq.as<uint64_t>(), h->rk.as<uint32_t>());
    HIP_TRY(e, hipMemcpyAsync(&reads, h->head_prefix.as<uint64_t>() + head_tiles, 8, hipMemcpyDeviceToHost, st));
    if (int rc = sync_check(e, "ovleval truth plan (the reads)")) return rc;
    reads = std::min(reads, n2);
    // the entries: their keys from the ranks, in order, the columns behind them
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)cus * 32u);
    hipLaunchKernelGGL(k_ove_keys, dim3(grid), dim3(256), 0, st, h->rk.as<const uint32_t>(), h->key[0].as<uint64_t>(), n);
    const uint32_t pair_bits = OVE_RANK_BITS + bits_of(reads ? reads - 1 : 0);
    cur = samsort_sort_pairs(st, keys, idxs, h->hist.as<uint32_t>(), h->digit_total.as<uint32_t>(), n, pair_bits);
    h->skey = h->key[cur].as<const uint64_t>();
    hipLaunchKernelGGL(k_ove_gather, dim3(grid), dim3(256), 0, st, h->skey, h->idx[cur].as<const uint32_t>(), h->appended(), h->sorted(), n,
                       h->word.as<uint32_t>());
  }
  if (int rc = end_span(h, SPAN_PLAN, st, "ovleval truth plan")) return rc;
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "ovleval truth plan")) return rc;
  if (errw & OVE_ERR_DUP) {
    uint32_t cleared = errw & ~OVE_ERR_DUP;  // (the entries stay; the flag is the plan's alone)
    HIP_TRY(e, hipMemcpy(h->word.p, &cleared, 4, hipMemcpyHostToDevice));
    return eng_fail(e, SIMMR_EINVAL, "two truth records name one pair of reads: the pair of an entry is unique");
  }
  h->n_entries = n;
  h->n_reads = reads;
  h->planned = true;
  if (int rc = fold_spans(h)) return rc;
  if (n_entries) *n_entries = n;
  if (n_reads) *n_reads = reads;
  return SIMMR_OK;
}

int simmr_ovleval_add(simmr_ovleval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_text(h, text, n_bytes, "simmr_ovleval_add")) return rc;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_ovleval_add called without a simmr_ovleval_truth_plan in force");
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (int rc = begin_span(h, SPAN_ADDS, st)) return rc;
  MevText W;
  uint32_t rec_grid = 1;
  if (int rc = enqueue_index(h, text, n_bytes, st, &W, &rec_grid)) return rc;
  hipLaunchKernelGGL(k_ove_record, dim3(rec_grid), dim3(OVE_WG), 0, st, W, h->uniq.as<const uint64_t>(), h->n_reads, h->skey, h->sorted(), h->n_entries,
                     h->min_pct, h->counts_p(), h->best.as<uint32_t>(), h->hits.as<uint32_t>(), h->word.as<uint32_t>());
  return end_span(h, SPAN_ADDS, st, "ovleval add");
}

int simmr_ovleval_read(simmr_ovleval* h, simmr_ovleval_counts* counts, uint64_t* by_len_host) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_ovleval_read called before simmr_ovleval_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + OC_PAIRS_FOUND, 0, (COUNT_WORDS - OC_PAIRS_FOUND) * 8, st));
  if (h->planned && h->n_entries > 0) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((h->n_entries + 255) / 256, (uint64_t)std::max(eng_cu_count(e), 1) * 16u);
    hipLaunchKernelGGL(k_ove_reduce, dim3(grid), dim3(256), 0, st, h->best.as<const uint32_t>(), h->hits.as<const uint32_t>(), h->s_ov.as<const uint64_t>(),
                       h->n_entries, h->counts_p(), h->counts_p() + OC_COUNT);
  }
  std::vector<uint64_t> host(COUNT_WORDS);
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(host.data(), h->counts.p, COUNT_WORDS * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "ovleval read")) return rc;
  if (errw & (OVE_ERR_TRUTH | OVE_ERR_CAND))
    return eng_fail(e, SIMMR_EINVAL, "a malformed %s record: fewer than 12 fields, a length, start, end or field 10 .. 12 that is no number, a strand that is "
                                     "neither + nor -, or start <= end <= length < 2^40 broken", errw & OVE_ERR_TRUTH ? "truth" : "candidate");
  host[OC_T_READS] = h->planned ? h->n_reads : 0;  // (the plan counts them on the host's side of its scan)
  if (counts) std::memcpy(counts, host.data(), sizeof(*counts));
  if (by_len_host) std::memcpy(by_len_host, host.data() + OC_COUNT, 2u * OVE_LEN_ROWS * 8);
  return SIMMR_OK;
}

int simmr_ovleval_emit(simmr_ovleval* h, uint64_t* key_a_dev, uint64_t* key_b_dev, uint64_t* ov_dev, uint32_t* best_dev, uint32_t* hits_dev,
                       uint64_t capacity) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_ovleval_emit called without a simmr_ovleval_truth_plan in force");
  if (capacity < h->n_entries)
    return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu truth entries", (unsigned long long)capacity, (unsigned long long)h->n_entries);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (h->n_entries > 0) {
    if (key_a_dev) HIP_TRY(e, hipMemcpyAsync(key_a_dev, h->s_ka.p, h->n_entries * 8, hipMemcpyDeviceToDevice, st));
    if (key_b_dev) HIP_TRY(e, hipMemcpyAsync(key_b_dev, h->s_kb.p, h->n_entries * 8, hipMemcpyDeviceToDevice, st));
    if (ov_dev) HIP_TRY(e, hipMemcpyAsync(ov_dev, h->s_ov.p, h->n_entries * 8, hipMemcpyDeviceToDevice, st));
    if (best_dev) HIP_TRY(e, hipMemcpyAsync(best_dev, h->best.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
    if (hits_dev) HIP_TRY(e, hipMemcpyAsync(hits_dev, h->hits.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
  }
  return sync_check(e, "ovleval emit");
}

int simmr_last_ovleval_ms(simmr_ovleval* h, float* ms) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!ms) return eng_fail(e, SIMMR_EINVAL, "simmr_last_ovleval_ms: NULL ms");
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_ovleval_reset yet");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = fold_spans(h)) return rc;  // (the next add of either side begins a new span)
  *ms = h->done_ms;
  return SIMMR_OK;
}

}  // extern "C"
