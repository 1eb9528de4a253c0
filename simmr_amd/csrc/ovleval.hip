// ovleval.hip — an overlapper's PAF scored against the true overlaps (include/simmr_hip.h: simmr_ovleval_*): the entry points over
// ovleval_kernels.hip, on the scaffold of scorer_host.hpp.  The pair sort runs twice in the plan.
//
// truth_add:  enqueue-only, so nothing is sized from what the text holds.  The index buffers are sized from n_bytes (a line start
//             per two bytes), the entry columns from the bytes of every truth add since the reset (an entry per OVE_MIN_LINE
//             bytes); a column that has to grow keeps what it holds.  index (count) -> scan -> index (write) -> truth.
// truth_plan: reads the cursor and the largest key; sorts the 2 n keys, counts the heads per tile, scans, writes the distinct keys
//             and the ranks; reads the number of distinct keys; makes the entry keys from the ranks, sorts them, gathers the
//             columns into that order and checks the neighbours; zeroes the candidate side.
// add:        index (count) -> scan -> index (write) -> record.
// Time: the adds' span and the plan's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "host_support.hpp"
#include "ovleval_kernels.hip"
#include "scorer_host.hpp"

using namespace simmr;

namespace {

enum { SPAN_ADDS = 0, SPAN_PLAN = 1, SPAN_COUNT = 2 };
constexpr size_t COUNT_WORDS = OC_COUNT + 2u * OVE_LEN_ROWS;

}  // namespace

struct simmr_ovleval {
  simmr_engine* e = nullptr;
  uint32_t min_pct = 10;
  LineIndex index;  // of one add
  // the truth: the entries as appended (u_*), and in pair order (s_*, with the sorted entry keys in skey)
  DevBuf u_keys, u_lo_s, u_lo_e, u_hi_s, u_hi_e, u_ov;
  DevBuf s_ka, s_kb, s_lo_s, s_lo_e, s_hi_s, s_hi_e, s_ov;
  PairSort order;
  DevBuf head_sum, head_prefix, uniq, rk;
  DevBuf cursor;   // [0] entries, [1] the largest key
  DevBuf counts;   // OC_COUNT words, then by_len's 82
  DevBuf word;     // the error word
  DevBuf best, hits;
  const uint64_t* skey = nullptr;
  uint64_t entry_cap = 0;   // entries the truth adds since the reset may have appended
  uint64_t n_entries = 0, n_reads = 0;
  bool reset_once = false, planned = false;
  FoldedSpans<SPAN_COUNT> sp;

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

int check_add(simmr_ovleval* h, const uint8_t* text, uint64_t n_bytes, const char* who) {
  return check_add_text(h->e, h->reset_once, text, n_bytes, SIMMR_FIT_SAM_MAX_BYTES, who, "simmr_ovleval_reset", "cut the text at a line's end");
}

// the line index of text[0, n_bytes) into the object's buffers (n_bytes > 0)
int enqueue_index(simmr_ovleval* h, const uint8_t* text, uint64_t n_bytes, hipStream_t st, MevText* W, uint32_t* rec_grid) {
  simmr_engine* e = h->e;
  const uint64_t n_tiles = (n_bytes + FSAM_TILE - 1) / FSAM_TILE, start_cap = n_bytes / 2 + 1;
  if (!h->index.room(n_tiles, start_cap))
    return eng_fail(e, SIMMR_ENOMEM, "ovleval line index: allocation failed for %llu bytes of text", (unsigned long long)n_bytes);
  const uint32_t cus = (uint32_t)std::max(eng_cu_count(e), 1);
  *rec_grid = (uint32_t)std::min<uint64_t>(n_bytes / (OVE_WG_RECS * OVE_MIN_LINE) + 1, (uint64_t)cus * 8u);
  h->index.enqueue(st, k_ove_index, k_ove_scan, text, n_bytes, FSAM_TILE, (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)cus * 16u), start_cap, W);
  return SIMMR_OK;
}

}  // namespace

extern "C" {

int simmr_ovleval_create(simmr_engine* e, simmr_ovleval** out) { return scorer_create(e, out, "simmr_ovleval_create"); }

void simmr_ovleval_destroy(simmr_ovleval* h) { scorer_destroy(h); }

int simmr_ovleval_reset(simmr_ovleval* h, uint32_t min_pct) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (min_pct > 100u) return eng_fail(e, SIMMR_EINVAL, "simmr_ovleval_reset: min_pct is 1 .. 100 (0: the default, 10)");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = sync_check(e, "ovleval reset")) return rc;
  h->planned = false;
  h->reset_once = false;
  if (int rc = h->sp.reset(e)) return rc;
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
  if (int rc = check_add(h, text, n_bytes, "simmr_ovleval_truth_add")) return rc;
  h->planned = false;
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t cap = h->entry_cap + n_bytes / OVE_MIN_LINE + 1, held = h->entry_cap;
  if (!h->u_keys.grow_keep(cap * 16, held * 16, st)) return eng_fail(e, SIMMR_ENOMEM, "ovleval truth: allocation failed for %llu entries", (unsigned long long)cap);
  for (DevBuf* b : {&h->u_lo_s, &h->u_lo_e, &h->u_hi_s, &h->u_hi_e, &h->u_ov})
    if (!b->grow_keep(cap * 8, held * 8, st)) return eng_fail(e, SIMMR_ENOMEM, "ovleval truth: allocation failed for %llu entries", (unsigned long long)cap);
  h->entry_cap = cap;
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  uint32_t rec_grid = 1;
  if (int rc = enqueue_index(h, text, n_bytes, st, &W, &rec_grid)) return rc;
  hipLaunchKernelGGL(k_ove_truth, dim3(rec_grid), dim3(OVE_WG), 0, st, W, h->appended(), cap, h->cursor.as<unsigned long long>(), h->counts_p(),
                     h->word.as<uint32_t>());
  return h->sp.end(e, SPAN_ADDS, st, "ovleval truth add");
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
  if (int rc = h->sp.fold(e, "ovleval")) return rc;
  if (errw & OVE_ERR_TRUTH)
    return eng_fail(e, SIMMR_EINVAL, "a malformed truth record: fewer than 12 fields, a length, start, end or field 10 .. 12 that is no number, a strand that "
                                     "is neither + nor -, start <= end <= length < 2^40 broken, a name that is no read id, or one read on both sides");
  const uint64_t n = std::min(cur2[0], h->entry_cap);
  if (n >= (1ull << 30)) return eng_fail(e, SIMMR_ERANGE, "simmr_ovleval_truth_plan takes fewer than 2^30 true pairs (%llu given)", (unsigned long long)n);
  const uint64_t n1 = std::max<uint64_t>(n, 1), n2 = 2 * n, head_tiles = (n2 + OVE_HEAD_TILE - 1) / OVE_HEAD_TILE;
  bool room = h->order.room(2 * n1) && h->head_sum.ensure(std::max<uint64_t>(head_tiles, 1) * 8) && h->head_prefix.ensure((head_tiles + 1) * 8) &&
              h->uniq.ensure(2 * n1 * 8) && h->rk.ensure(2 * n1 * 4);
  for (DevBuf* b : {&h->s_ka, &h->s_kb, &h->s_lo_s, &h->s_lo_e, &h->s_hi_s, &h->s_hi_e, &h->s_ov}) room = room && b->ensure(n1 * 8);
  for (DevBuf* b : {&h->best, &h->hits}) room = room && b->ensure(n1 * 4);
  if (!room) return eng_fail(e, SIMMR_ENOMEM, "ovleval truth plan: allocation failed (%llu entries)", (unsigned long long)n);
  if (int rc = h->sp.begin(e, SPAN_PLAN, st)) return rc;
  // the candidate side starts over: its counts (the words behind the truth's three), by_len, best and hits
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + OC_LINES, 0, (COUNT_WORDS - OC_LINES) * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->best.p, 0, n1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->hits.p, 0, n1 * 4, st));
  h->skey = h->order.key[0].as<const uint64_t>();
  uint64_t reads = 0;
  if (n > 0) {
    const uint32_t cus = (uint32_t)std::max(eng_cu_count(e), 1);
    // the reads: the 2 n keys in order, their heads, the ranks
    HIP_TRY(e, hipMemcpyAsync(h->order.key[0].p, h->u_keys.p, n2 * 8, hipMemcpyDeviceToDevice, st));
    const PairSort::Sorted by_read = h->order.sort(st, n2, bits_of(cur2[1]));
    const uint32_t head_grid = (uint32_t)std::min<uint64_t>(head_tiles, (uint64_t)cus * 32u);
    hipLaunchKernelGGL(k_ove_heads, dim3(head_grid), dim3(256), 0, st, by_read.keys, by_read.perm, n2, head_tiles, h->head_sum.as<uint64_t>(),
                       (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_ove_scan, dim3(1), dim3(256), 0, st, h->head_sum.as<const uint64_t>(), h->head_prefix.as<uint64_t>(), head_tiles);
    hipLaunchKernelGGL(k_ove_heads, dim3(head_grid), dim3(256), 0, st, by_read.keys, by_read.perm, n2, head_tiles, h->head_sum.as<uint64_t>(),
                       h->head_prefix.as<const uint64_t>(), h->uniq.as<uint64_t>(), h->rk.as<uint32_t>());
    HIP_TRY(e, hipMemcpyAsync(&reads, h->head_prefix.as<uint64_t>() + head_tiles, 8, hipMemcpyDeviceToHost, st));
    if (int rc = sync_check(e, "ovleval truth plan (the reads)")) return rc;
    reads = std::min(reads, n2);
    // the entries: their keys from the ranks, in order, the columns behind them
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)cus * 32u);
    hipLaunchKernelGGL(k_ove_keys, dim3(grid), dim3(256), 0, st, h->rk.as<const uint32_t>(), h->order.key[0].as<uint64_t>(), n);
    const PairSort::Sorted by_pair = h->order.sort(st, n, OVE_RANK_BITS + bits_of(reads ? reads - 1 : 0));  // (at least OVE_RANK_BITS bits: a permutation)
    h->skey = by_pair.keys;
    hipLaunchKernelGGL(k_ove_gather, dim3(grid), dim3(256), 0, st, h->skey, by_pair.perm, h->appended(), h->sorted(), n, h->word.as<uint32_t>());
  }
  if (int rc = h->sp.end(e, SPAN_PLAN, st, "ovleval truth plan")) return rc;
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
  if (int rc = h->sp.fold(e, "ovleval")) return rc;
  if (n_entries) *n_entries = n;
  if (n_reads) *n_reads = reads;
  return SIMMR_OK;
}

int simmr_ovleval_add(simmr_ovleval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_ovleval_add")) return rc;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_ovleval_add called without a simmr_ovleval_truth_plan in force");
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  uint32_t rec_grid = 1;
  if (int rc = enqueue_index(h, text, n_bytes, st, &W, &rec_grid)) return rc;
  hipLaunchKernelGGL(k_ove_record, dim3(rec_grid), dim3(OVE_WG), 0, st, W, h->uniq.as<const uint64_t>(), h->n_reads, h->skey, h->sorted(), h->n_entries,
                     h->min_pct, h->counts_p(), h->best.as<uint32_t>(), h->hits.as<uint32_t>(), h->word.as<uint32_t>());
  return h->sp.end(e, SPAN_ADDS, st, "ovleval add");
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
  return h->sp.last_ms(e, "ovleval", ms);
}

}  // extern "C"
