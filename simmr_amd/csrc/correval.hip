// correval.hip — a read error corrector's output scored against the true reads (include/simmr_hip.h: simmr_correval_*): the entry
// points over correval_kernels.hip, on the scaffold of scorer_host.hpp.
//
// truth_add:  enqueue-only, so nothing is sized from what the text holds.  The index buffers are sized from n_bytes (a line start
//             per two bytes), the entry columns and the two planes from the bytes of every truth add since the reset (an entry per
//             CEV_MIN_LINE bytes, a base per byte); a column or plane that has to grow keeps what it holds.
//             index (count) -> scan -> index (write) -> truth.
// truth_plan: reads the cursor and the largest key, copies the keys to the sort's ping, sorts over the bits of the largest key,
//             gathers the columns into key order and checks the neighbours; empties the corrected side.
// add:        lines (count) -> scan -> lines (write) -> score.  A line start per byte: every '\n' ends a line.
// read:       the reduce over the entries, the table to the host, by_pos's kept column from the histogram of the compared lengths.
// Time: the adds' span, the plan's and the read's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "host_support.hpp"
#include "correval_kernels.hip"
#include "scorer_host.hpp"

using namespace simmr;

namespace {

// Workgroups a CU of every grid: beyond them the workgroups loop.  Small, so that a text of a few hundred KB takes every kernel past one trip.
constexpr uint32_t WGS_PER_CU = 2;

enum { SPAN_ADDS = 0, SPAN_PLAN = 1, SPAN_READ = 2, SPAN_COUNT = 3 };

const char* const MALFORMED_TRUTH =
    "fewer than 11 fields, a bad FLAG / POS / MAPQ / CIGAR, a QNAME that is no read id, a POS of 0, a QUAL that is neither '*' nor as long as SEQ or "
    "holds a byte outside '!' .. '~', no MD:Z: field, an MD with '^', another byte or a number of more than 9 digits, or an MD that does not add up to "
    "the length of SEQ";
const char* const MALFORMED_READS =
    "lines that are no multiple of the record's lines, a first line that does not start with '@' ('>' for two-line records), a third line that does "
    "not start with '+', or a quality line whose length differs from the bases'";

}  // namespace

struct simmr_correval {
  simmr_engine* e = nullptr;
  uint32_t lpr = 4;
  LineIndex index;  // of one add
  // the truth: the entries as appended (u_*), and in key order (s_*, with the sorted keys in skey); the planes
  DevBuf u_key, u_len, u_off, u_before, s_len, s_off, s_before;
  PairSort order;
  DevBuf plane_ot, plane_q;
  DevBuf cursor;   // [0] entries, [1] the largest key, [2] plane bytes
  DevBuf table;    // CT_WORDS words
  DevBuf word;     // the error word
  DevBuf residual, hits;
  const uint64_t* skey = nullptr;
  uint64_t entry_cap = 0, plane_cap = 0;   // what the truth adds since the reset may have appended
  uint64_t n_entries = 0;
  bool reset_once = false, planned = false;
  FoldedSpans<SPAN_COUNT> sp;

  unsigned long long* table_p() const { return table.as<unsigned long long>(); }
  CevEntries appended() const { return CevEntries{u_key.as<uint64_t>(), u_len.as<uint32_t>(), u_off.as<uint64_t>(), u_before.as<uint32_t>()}; }
  CevEntries sorted() const { return CevEntries{nullptr, s_len.as<uint32_t>(), s_off.as<uint64_t>(), s_before.as<uint32_t>()}; }
  CevPlanes planes() const { return CevPlanes{plane_ot.as<uint8_t>(), plane_q.as<uint8_t>(), plane_cap}; }
};

namespace {

int check_add(simmr_correval* h, const uint8_t* text, uint64_t n_bytes, const char* who) {
  return check_add_text(h->e, h->reset_once, text, n_bytes, SIMMR_FIT_SAM_MAX_BYTES, who, "simmr_correval_reset", "cut the text at a line's or a record's end");
}

// the line index of text[0, n_bytes) into the object's buffers (n_bytes > 0): the SAM rule (empty lines never enter it), or every line
int enqueue_index(simmr_correval* h, const uint8_t* text, uint64_t n_bytes, bool every_line, hipStream_t st, MevText* W) {
  simmr_engine* e = h->e;
  const uint64_t n_tiles = (n_bytes + CEV_TILE - 1) / CEV_TILE, start_cap = every_line ? n_bytes : n_bytes / 2 + 1;
  if (!h->index.room(n_tiles, start_cap))
    return eng_fail(e, SIMMR_ENOMEM, "correval line index: allocation failed for %llu bytes of text", (unsigned long long)n_bytes);
  h->index.enqueue(st, every_line ? k_cev_lines : k_cev_index, k_cev_scan, text, n_bytes, CEV_TILE, grid_for(e, n_tiles, 1, WGS_PER_CU), start_cap, W);
  return SIMMR_OK;
}

int malformed(simmr_correval* h, uint32_t errw) {
  simmr_engine* e = h->e;
  if (errw & CEV_ERR_TRUTH) return eng_fail(e, SIMMR_EINVAL, "a malformed truth record: %s", MALFORMED_TRUTH);
  if (errw & CEV_ERR_DUP) return eng_fail(e, SIMMR_EINVAL, "two truth records have one read id and mate: the key of an entry is unique");
  if (errw & CEV_ERR_READS) return eng_fail(e, SIMMR_EINVAL, "a malformed corrected text: %s", MALFORMED_READS);
  return SIMMR_OK;
}

}  // namespace

extern "C" {

int simmr_correval_create(simmr_engine* e, simmr_correval** out) { return scorer_create(e, out, "simmr_correval_create"); }

void simmr_correval_destroy(simmr_correval* h) { scorer_destroy(h); }

int simmr_correval_reset(simmr_correval* h, const simmr_correval_config* cfg) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!cfg) return eng_fail(e, SIMMR_EINVAL, "simmr_correval_reset: NULL argument");
  if ((cfg->lines_per_record != 0u && cfg->lines_per_record != 2u && cfg->lines_per_record != 4u) || cfg->reserved != 0u)
    return eng_fail(e, SIMMR_EINVAL, "simmr_correval_reset: lines_per_record is 4 (FASTQ), 2 (two-line FASTA) or 0 (the default, 4); reserved is 0");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = sync_check(e, "correval reset")) return rc;
  h->planned = false;
  h->reset_once = false;
  if (int rc = h->sp.reset(e)) return rc;
  if (!h->cursor.ensure(32) || !h->table.ensure(CT_WORDS * 8) || !h->word.ensure(16)) return eng_fail(e, SIMMR_ENOMEM, "correval reset: allocation failed");
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemsetAsync(h->cursor.p, 0, 32, st));
  HIP_TRY(e, hipMemsetAsync(h->table.p, 0, CT_WORDS * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->word.p, 0, 16, st));
  if (int rc = sync_check(e, "correval reset")) return rc;
  h->lpr = cfg->lines_per_record ? cfg->lines_per_record : 4u;
  h->entry_cap = h->plane_cap = 0;
  h->n_entries = 0;
  h->reset_once = true;
  return SIMMR_OK;
}

int simmr_correval_truth_add(simmr_correval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_correval_truth_add")) return rc;
  h->planned = false;
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t cap = h->entry_cap + n_bytes / CEV_MIN_LINE + 1, held = h->entry_cap, bytes = h->plane_cap + n_bytes;
  if (!h->u_key.grow_keep(cap * 8, held * 8, st) || !h->u_len.grow_keep(cap * 4, held * 4, st) || !h->u_off.grow_keep(cap * 8, held * 8, st) ||
      !h->u_before.grow_keep(cap * 4, held * 4, st) || !h->plane_ot.grow_keep(bytes, h->plane_cap, st) || !h->plane_q.grow_keep(bytes, h->plane_cap, st))
    return eng_fail(e, SIMMR_ENOMEM, "correval truth: allocation failed for %llu entries and %llu bases", (unsigned long long)cap, (unsigned long long)bytes);
  h->entry_cap = cap;
  h->plane_cap = bytes;
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  if (int rc = enqueue_index(h, text, n_bytes, false, st, &W)) return rc;
  const uint32_t grid = grid_for(e, n_bytes / CEV_MIN_LINE + 1, CEV_WG_RECS, WGS_PER_CU);
  hipLaunchKernelGGL(k_cev_truth, dim3(grid), dim3(CEV_WG), 0, st, W, h->appended(), cap, h->planes(), h->cursor.as<unsigned long long>(), h->table_p(),
                     h->word.as<uint32_t>());
  return h->sp.end(e, SPAN_ADDS, st, "correval truth add");
}

int simmr_correval_truth_plan(simmr_correval* h, uint64_t* n_entries) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_correval_truth_plan called before simmr_correval_reset");
  h->planned = false;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  uint64_t cur3[3] = {0, 0, 0};
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(cur3, h->cursor.p, 24, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "correval truth adds")) return rc;
  if (int rc = h->sp.fold(e, "correval")) return rc;
  if (errw & CEV_ERR_TRUTH) return malformed(h, CEV_ERR_TRUTH);
  const uint64_t n = std::min(cur3[0], h->entry_cap);
  if (n >= (1ull << 31)) return eng_fail(e, SIMMR_ERANGE, "simmr_correval_truth_plan takes fewer than 2^31 truth entries (%llu given)", (unsigned long long)n);
  const uint64_t n1 = std::max<uint64_t>(n, 1);
  bool room = h->order.room(n1) && h->s_off.ensure(n1 * 8);
  for (DevBuf* b : {&h->s_len, &h->s_before, &h->residual, &h->hits}) room = room && b->ensure(n1 * 4);
  if (!room) return eng_fail(e, SIMMR_ENOMEM, "correval truth plan: allocation failed (%llu entries)", (unsigned long long)n);
  if (int rc = h->sp.begin(e, SPAN_PLAN, st)) return rc;
  // the corrected side starts over: its counts (the words behind the truth's five), the tables, residual and hits
  HIP_TRY(e, hipMemsetAsync(h->table_p() + CC_LINES, 0, (CT_WORDS - CC_LINES) * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->residual.p, 0xff, n1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->hits.p, 0, n1 * 4, st));
  h->skey = h->order.key[0].as<const uint64_t>();
  if (n > 0) {
    HIP_TRY(e, hipMemcpyAsync(h->order.key[0].p, h->u_key.p, n * 8, hipMemcpyDeviceToDevice, st));
    const PairSort::Sorted by_key = h->order.sort(st, n, bits_of(cur3[1]));
    h->skey = by_key.keys;
    hipLaunchKernelGGL(k_cev_gather, dim3(grid_for(e, n, 256, WGS_PER_CU)), dim3(256), 0, st, h->skey, by_key.perm, h->appended(), h->sorted(), n, h->word.as<uint32_t>());
  }
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = h->sp.end(e, SPAN_PLAN, st, "correval truth plan")) return rc;
  if (int rc = sync_check(e, "correval truth plan")) return rc;
  if (int rc = h->sp.fold(e, "correval")) return rc;
  if (errw & CEV_ERR_DUP) {
    uint32_t cleared = errw & ~CEV_ERR_DUP;  // (the entries stay; the flag is the plan's alone)
    HIP_TRY(e, hipMemcpy(h->word.p, &cleared, 4, hipMemcpyHostToDevice));
    return malformed(h, CEV_ERR_DUP);
  }
  h->n_entries = n;
  h->planned = true;
  if (n_entries) *n_entries = n;
  return SIMMR_OK;
}

int simmr_correval_add(simmr_correval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_correval_add")) return rc;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_correval_add called without a simmr_correval_truth_plan in force");
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  if (int rc = enqueue_index(h, text, n_bytes, true, st, &W)) return rc;
  // a record is at least its lines' ends: lines_per_record bytes
  const uint32_t grid = grid_for(e, n_bytes / h->lpr + 1, CEV_WG_RECS, WGS_PER_CU);
  hipLaunchKernelGGL(k_cev_score, dim3(grid), dim3(CEV_WG), 0, st, W, h->lpr, h->skey, h->sorted(), h->n_entries, h->planes(), h->table_p(),
                     h->residual.as<uint32_t>(), h->hits.as<uint32_t>(), h->word.as<uint32_t>());
  return h->sp.end(e, SPAN_ADDS, st, "correval add");
}

int simmr_correval_read(simmr_correval* h, simmr_correval_counts* counts, uint64_t* cube_host, uint64_t* by_qual_host, uint64_t* by_pos_host) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_correval_read called before simmr_correval_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (int rc = h->sp.fold(e, "correval")) return rc;  // (the adds' span ends here)
  if (int rc = h->sp.begin(e, SPAN_READ, st)) return rc;
  HIP_TRY(e, hipMemsetAsync(h->table_p() + CC_MISSING, 0, 8 * 8, st));
  if (h->planned && h->n_entries > 0)
    hipLaunchKernelGGL(k_cev_reduce, dim3(grid_for(e, h->n_entries, 256, WGS_PER_CU)), dim3(256), 0, st, h->hits.as<const uint32_t>(), h->residual.as<const uint32_t>(),
                       h->s_before.as<const uint32_t>(), h->n_entries, h->table_p());
  std::vector<uint64_t> host(CT_WORDS);
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(host.data(), h->table.p, CT_WORDS * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = h->sp.end(e, SPAN_READ, st, "correval read")) return rc;
  if (int rc = sync_check(e, "correval read")) return rc;
  if (int rc = h->sp.fold(e, "correval")) return rc;
  if (errw & (CEV_ERR_TRUTH | CEV_ERR_READS)) return malformed(h, errw & (CEV_ERR_TRUTH | CEV_ERR_READS));
  if (counts) std::memcpy(counts, host.data(), sizeof(*counts));
  if (cube_host) std::memcpy(cube_host, host.data() + CT_CUBE, 125 * 8);
  if (by_qual_host) std::memcpy(by_qual_host, host.data() + CT_QUAL, CEV_QUALS * 5 * 8);
  if (by_pos_host) {
    // kept at row p = the records that were compared there, less the positions that are not kept: the records with a compared length
    // above p for the rows before the last, and the sum of (length - 511) for the last, which takes every position from 511 on
    std::memcpy(by_pos_host, host.data() + CT_POS, CEV_POS * 5 * 8);
    uint64_t above = host[CT_LEN + CEV_POS];
    for (uint32_t p = CEV_POS - 1u; p-- > 0u;) {  // p = 510 .. 0
      above += host[CT_LEN + p + 1u];
      by_pos_host[p * 5u] = above - host[CT_POS + p * 5u];
    }
    by_pos_host[(CEV_POS - 1u) * 5u] = host[CT_TAIL] - host[CT_POS + (CEV_POS - 1u) * 5u];
  }
  return SIMMR_OK;
}

int simmr_correval_emit(simmr_correval* h, uint64_t* key_dev, uint32_t* length_dev, uint32_t* before_dev, uint32_t* residual_dev, uint32_t* hits_dev,
                        uint64_t capacity) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_correval_emit called without a simmr_correval_truth_plan in force");
  if (capacity < h->n_entries)
    return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu truth entries", (unsigned long long)capacity, (unsigned long long)h->n_entries);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t n = h->n_entries;
  if (n > 0) {
    if (key_dev) HIP_TRY(e, hipMemcpyAsync(key_dev, h->skey, n * 8, hipMemcpyDeviceToDevice, st));
    if (length_dev) HIP_TRY(e, hipMemcpyAsync(length_dev, h->s_len.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (before_dev) HIP_TRY(e, hipMemcpyAsync(before_dev, h->s_before.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (residual_dev) HIP_TRY(e, hipMemcpyAsync(residual_dev, h->residual.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (hits_dev) HIP_TRY(e, hipMemcpyAsync(hits_dev, h->hits.p, n * 4, hipMemcpyDeviceToDevice, st));
  }
  return sync_check(e, "correval emit");
}

int simmr_last_correval_ms(simmr_correval* h, float* ms) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!ms) return eng_fail(e, SIMMR_EINVAL, "simmr_last_correval_ms: NULL ms");
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_correval_reset yet");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  return h->sp.last_ms(e, "correval", ms);
}

}  // extern "C"
