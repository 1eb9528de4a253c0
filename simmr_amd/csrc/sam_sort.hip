// sam_sort.hip — the true alignments in coordinate order (include/simmr_hip.h: simmr_sam_sort_*): the entry points over
// sam_sort_kernels.hip.  The seventh translation unit of libsimmr_hip.so; like sam.hip it sees an engine through
// engine_internal.hpp only and keeps its state in a slot of its own (ENG_EXT_SAM_SORT), so a sorted plan and an unsorted one
// on one engine do not disturb each other.  The names table and the argument checks are sam.hip's (sam_names.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "sam_sort_kernels.hip"
#include "sam_names.hpp"

using namespace simmr;

namespace {

struct SamSortState {
  SamNameTable nt;
  DevBuf len;              // per read
  DevBuf key[2], idx[2];   // the pairs, ping and pong; behind the sort the free key buffer holds the canonical keys and the
                           // free index buffer the sorted lengths
  DevBuf hist, digit_total, line_off, chunk_sum, chunk_prefix;
  DevBuf word;             // the error word
  const uint32_t* perm = nullptr;  // place -> read (nullptr: the identity, a key without bits)
  const uint64_t* ckey = nullptr;  // the canonical key of every place
  SamReads reads{};
  SamEdits edits{};
  uint32_t paired = 0;
  uint64_t n_reads = 0, total = 0, epoch = 0;
  bool ready = false, planned_once = false, emitted = false;
  hipEvent_t ev[4] = {};
  uint32_t* err_p() const { return word.as<uint32_t>(); }
};

void sam_sort_destroy(void* q) {
  SamSortState* s = (SamSortState*)q;
  s->nt.release();
  for (DevBuf* b : {&s->len, &s->key[0], &s->key[1], &s->idx[0], &s->idx[1], &s->hist, &s->digit_total, &s->line_off, &s->chunk_sum,
                    &s->chunk_prefix, &s->word})
    b->release();
  for (hipEvent_t ev : s->ev)
    if (ev) (void)hipEventDestroy(ev);
  delete s;
}

SamSortState* state_of(simmr_engine* e, bool create) {
  void** slot = eng_ext_slot(e, ENG_EXT_SAM_SORT, sam_sort_destroy);
  if (!*slot && create) *slot = new SamSortState();
  return (SamSortState*)*slot;
}

uint32_t bits_of(uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }

}  // namespace

// engine_internal.hpp: the sort itself, for this unit's plan and for overlap.hip's
namespace simmr {
static_assert(SAMSORT_PAIRS_TILE == SAMSORT_TILE && SAMSORT_PAIRS_DIGITS == SAMSORT_DIGITS, "engine_internal.hpp states the tile and the digits");
int samsort_sort_pairs(hipStream_t st, uint64_t* const key[2], uint32_t* const idx[2], uint32_t* hist, uint32_t* digit_total, uint64_t n,
                       uint32_t key_bits) {
  const uint32_t n_passes = (key_bits + SAMSORT_DIGIT_BITS - 1u) / SAMSORT_DIGIT_BITS;
  const uint32_t n_tiles = (uint32_t)((n + SAMSORT_TILE - 1) / SAMSORT_TILE);
  int cur = 0;
  if (n == 0) return cur;
  // least significant digit first, over the bits the caller gives the key: a stable pass per digit
  for (uint32_t p = 0; p < n_passes; p++) {
    const uint32_t shift = p * SAMSORT_DIGIT_BITS;
    hipLaunchKernelGGL(k_samsort_hist, dim3(n_tiles), dim3(256), 0, st, (const uint64_t*)key[cur], n, shift, hist, n_tiles);
    hipLaunchKernelGGL(k_samsort_digit_scan, dim3(SAMSORT_DIGITS), dim3(256), 0, st, hist, n_tiles, digit_total);
    hipLaunchKernelGGL(k_samsort_scatter, dim3(n_tiles), dim3(256), 0, st, (const uint64_t*)key[cur], p ? (const uint32_t*)idx[cur] : (const uint32_t*)nullptr,
                       key[cur ^ 1], idx[cur ^ 1], n, shift, (const uint32_t*)hist, (const uint32_t*)digit_total, n_tiles);
    cur ^= 1;
  }
  return cur;
}
}  // namespace simmr

extern "C" {

int simmr_sam_sort_key_bits(uint64_t n_rows, uint64_t longest_contig, uint32_t* pos_bits, uint32_t* row_bits) {
  if (n_rows > (1ull << 24) || longest_contig >= (1ull << SAMSORT_KEY_POS_BITS)) return SIMMR_ERANGE;
  if (pos_bits) *pos_bits = bits_of(longest_contig);
  if (row_bits) *row_bits = n_rows ? bits_of(n_rows - 1) : 0u;
  return SIMMR_OK;
}

int simmr_sam_sort_plan(simmr_engine* e, const simmr_sam_names* names, const simmr_reads_out* reads, const simmr_truth_out* truth,
                        uint64_t n_reads, int paired, uint64_t* total_bytes) {
  if (!e) return SIMMR_EINVAL;
  if (SamSortState* old = state_of(e, false)) old->ready = old->emitted = false;
  if (int rc = check_plan_args(e, names, reads, truth, n_reads, paired, total_bytes, "simmr_sam_sort_plan")) return rc;
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  SamSortState* s = state_of(e, true);
  if (int rc = sam_sync_check(e, "sorted SAM plan")) return rc;  // (an upload of an earlier plan that failed may still read the host copies)
  if (int rc = s->nt.build(e, names)) return rc;
  uint32_t pos_bits = 0, row_bits = 0;
  if (simmr_sam_sort_key_bits(s->nt.n_rows, s->nt.longest, &pos_bits, &row_bits) != SIMMR_OK)
    return eng_fail(e, SIMMR_ERANGE, "simmr_sam_sort_plan: %llu named contigs, the longest of %llu bases: the key takes at most 2^24 contigs of "
                                     "fewer than 2^40 bases", (unsigned long long)s->nt.n_rows, (unsigned long long)s->nt.longest);
  const uint32_t key_bits = pos_bits + row_bits;
  for (hipEvent_t& ev : s->ev)
    if (!ev) SAM_TRY(e, hipEventCreate(&ev));
  const uint64_t n_chunks = (n_reads + SAM_CHUNK - 1) / SAM_CHUNK, n_tiles = (n_reads + SAMSORT_TILE - 1) / SAMSORT_TILE;
  const uint64_t n1 = std::max<uint64_t>(n_reads, 1);
  if (!s->nt.ensure(true) || !s->len.ensure(n1 * 4) || !s->key[0].ensure(n1 * 8) || !s->key[1].ensure(n1 * 8) || !s->idx[0].ensure(n1 * 4) ||
      !s->idx[1].ensure(n1 * 4) || !s->hist.ensure(std::max<uint64_t>(n_tiles, 1) * SAMSORT_DIGITS * 4) || !s->digit_total.ensure(SAMSORT_DIGITS * 4) ||
      !s->line_off.ensure((n_reads + 1) * 8) || !s->chunk_sum.ensure(std::max<uint64_t>(n_chunks, 1) * 8) ||
      !s->chunk_prefix.ensure((n_chunks + 1) * 8) || !s->word.ensure(16))
    return eng_fail(e, SIMMR_ENOMEM, "sorted SAM plan allocation failed (%llu reads)", (unsigned long long)n_reads);
  hipStream_t st = eng_stream(e);
  SAM_TRY(e, s->nt.upload(st, true));
  SAM_TRY(e, hipMemsetAsync(s->word.p, 0, 16, st));
  SAM_TRY(e, hipEventRecord(s->ev[0], st));
  // a workgroup per chunk (fewer than 2^21 of them): of this unit's grids only the writer's is capped, as k_sam_write's is
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, n_chunks);
  int cur = 0;  // key[cur] / idx[cur] hold the pairs
  bool have_idx = false;
  if (n_reads > 0) {
    hipLaunchKernelGGL(k_samsort_size, dim3(grid), dim3(256), 0, st, sam_reads(reads), sam_edits(truth), s->nt.names(),
                       s->nt.c_bases.as<const uint64_t>(), n_reads, paired ? 1u : 0u, pos_bits, s->len.as<uint32_t>(), s->key[0].as<uint64_t>(), s->err_p());
    uint64_t* const keys[2] = {s->key[0].as<uint64_t>(), s->key[1].as<uint64_t>()};
    uint32_t* const idxs[2] = {s->idx[0].as<uint32_t>(), s->idx[1].as<uint32_t>()};
    cur = samsort_sort_pairs(st, keys, idxs, s->hist.as<uint32_t>(), s->digit_total.as<uint32_t>(), n_reads, key_bits);
    have_idx = key_bits > 0u;
    s->perm = have_idx ? s->idx[cur].as<const uint32_t>() : nullptr;
    s->ckey = s->key[cur ^ 1].as<const uint64_t>();
    uint32_t* slen = s->idx[cur ^ 1].as<uint32_t>();
    hipLaunchKernelGGL(k_samsort_gather, dim3(grid), dim3(256), 0, st, s->len.as<const uint32_t>(), s->key[cur].as<const uint64_t>(), s->perm, n_reads,
                       pos_bits, slen, s->key[cur ^ 1].as<uint64_t>(), s->chunk_sum.as<uint64_t>());
    hipLaunchKernelGGL(k_samsort_scan, dim3(1), dim3(256), 0, st, s->chunk_sum.as<const uint64_t>(), s->chunk_prefix.as<uint64_t>(), n_chunks);
    hipLaunchKernelGGL(k_samsort_offsets, dim3(grid), dim3(256), 0, st, (const uint32_t*)slen, s->chunk_prefix.as<const uint64_t>(), n_reads,
                       s->line_off.as<uint64_t>());
  } else {
    SAM_TRY(e, hipMemsetAsync(s->line_off.p, 0, 8, st));
  }
  SAM_TRY(e, hipEventRecord(s->ev[1], st));
  uint64_t total = 0;
  uint32_t errw = 0;
  SAM_TRY(e, hipMemcpyAsync(&total, s->line_off.as<uint64_t>() + n_reads, 8, hipMemcpyDeviceToHost, st));
  SAM_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sam_sync_check(e, "sorted SAM size and sort passes")) return rc;
  s->planned_once = true;
  if (errw & 2u)
    return eng_fail(e, SIMMR_EINVAL, "a read's genome / contig has no name, or the read ends behind its contig's staged length");
  if (errw)
    return eng_fail(e, SIMMR_EINVAL, "a read's bytes leave seq[], it is longer than %u bases, its edit_off decreases or leaves edits_capacity, or "
                                     "its edit_pos do not ascend inside the read", SAM_MAX_L);
  s->reads = sam_reads(reads);
  s->edits = sam_edits(truth);
  s->paired = paired ? 1u : 0u;
  s->n_reads = n_reads;
  s->total = total;
  s->epoch = eng_staging_epoch(e);
  s->ready = true;
  *total_bytes = total;
  return SIMMR_OK;
}

int simmr_sam_sort_emit(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* truth, uint8_t* dst, uint64_t dst_capacity,
                        uint64_t* key_out, uint64_t* line_off_out) {
  if (!e) return SIMMR_EINVAL;
  if (!reads || !truth) return eng_fail(e, SIMMR_EINVAL, "simmr_sam_sort_emit: NULL argument");
  SamSortState* s = state_of(e, false);
  if (s) s->emitted = false;
  SamReads now_r{};  // (zeroed first: the structs are compared as bytes, padding included)
  SamEdits now_e{};
  std::memset(&now_r, 0, sizeof now_r);
  std::memset(&now_e, 0, sizeof now_e);
  assign_reads(&now_r, reads);
  assign_edits(&now_e, truth);
  if (!s || !s->ready || std::memcmp(&now_r, &s->reads, sizeof now_r) != 0 || std::memcmp(&now_e, &s->edits, sizeof now_e) != 0)
    return eng_fail(e, SIMMR_ESTATE, "simmr_sam_sort_emit called without a simmr_sam_sort_plan for these columns");
  if (s->epoch != eng_staging_epoch(e)) return eng_fail(e, SIMMR_ESTATE, "a genome was staged since simmr_sam_sort_plan: plan again");
  if (int rc = check_columns(e, reads, truth, "simmr_sam_sort_emit")) return rc;
  if (dst_capacity < s->total)
    return eng_fail(e, SIMMR_ERANGE, "dst_capacity %llu < %llu bytes planned", (unsigned long long)dst_capacity, (unsigned long long)s->total);
  if (s->total > 0 && !dst) return eng_fail(e, SIMMR_EINVAL, "simmr_sam_sort_emit: NULL dst");
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  SAM_TRY(e, hipEventRecord(s->ev[2], st));
  if (s->n_reads > 0) {
    const uint64_t n_batches = (s->n_reads + SAM_WG_READS - 1) / SAM_WG_READS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_batches, (uint64_t)eng_cu_count(e) * SAM_WGS_PER_CU);
    hipLaunchKernelGGL(k_samsort_write, dim3(grid), dim3(256), 0, st, s->reads, s->edits, s->nt.names(), s->n_reads, s->paired, s->perm,
                       s->line_off.as<const uint64_t>(), dst, s->err_p());
    if (key_out) SAM_TRY(e, hipMemcpyAsync(key_out, s->ckey, s->n_reads * 8, hipMemcpyDeviceToDevice, st));
  }
  if (line_off_out) SAM_TRY(e, hipMemcpyAsync(line_off_out, s->line_off.p, (s->n_reads + 1) * 8, hipMemcpyDeviceToDevice, st));
  SAM_TRY(e, hipEventRecord(s->ev[3], st));
  uint32_t errw = 0;
  SAM_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sam_sync_check(e, "sorted SAM write pass")) return rc;
  s->emitted = true;
  if (errw) {
    s->ready = false;
    return eng_fail(e, SIMMR_EINVAL, "the columns changed since simmr_sam_sort_plan: a read failed the bounds check of the write pass (no store "
                                     "left its record)");
  }
  return SIMMR_OK;
}

int simmr_last_sam_sort_ms(simmr_engine* e, float* ms) {
  if (!e || !ms) return SIMMR_EINVAL;
  SamSortState* s = state_of(e, false);
  if (!s || !s->planned_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_sam_sort_plan yet");
  if (int rc = sam_sync_check(e, "sorted sam")) return rc;
  float a = 0.f, b = 0.f;
  SAM_TRY(e, hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
  if (s->emitted) SAM_TRY(e, hipEventElapsedTime(&b, s->ev[2], s->ev[3]));
  *ms = a + b;
  return SIMMR_OK;
}

}  // extern "C"
