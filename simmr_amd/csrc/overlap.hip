// overlap.hip — the true read-to-read overlaps as PAF (include/simmr_hip.h: simmr_overlap_*): the entry points over
// overlap_kernels.hip.  The eighth translation unit of libsimmr_hip.so; it sees an engine through engine_internal.hpp only, keeps
// its state in a slot of its own (ENG_EXT_OVERLAP) and sorts with sam_sort.hip's radix sort (samsort_sort_pairs).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "overlap_kernels.hip"
#include "sam_names.hpp"

using namespace simmr;

namespace {

struct OverlapState {
  // the rows the reset fixed
  DevBuf g_cbase, g_ncontig, c_bases;
  uint32_t n_slots = 0, pos_bits = 0, key_bits = 0;
  uint64_t n_rows = 0, epoch = 0;
  // what the adds appended: one entry per read, in the order they were added
  DevBuf key, meta, rid;
  uint64_t n = 0;
  uint32_t paired = 0;
  // the plan
  DevBuf skey[2], sidx[2], hist, digit_total, smeta, srid, cnt, rec_off, chunk_sum, chunk_prefix, rsum, rprefix;
  DevBuf word;  // the error word, and six words of k_ovl_window's answer behind it
  OvlSorted sorted{};
  uint64_t min_overlap = 0, total = 0;
  bool ready = false, planned = false;
  Spans<2> sp;  // plan; an emit call (measured call by call into emit_ms, never marked)
  float emit_ms = 0.f;
  uint32_t* err_p() const { return word.as<uint32_t>(); }
  uint64_t* win_p() const { return word.as<uint64_t>() + 2; }
  OvlRows rows() const { return OvlRows{g_cbase.as<const uint32_t>(), g_ncontig.as<const uint32_t>(), c_bases.as<const uint64_t>(), n_slots}; }
};

constexpr auto overlap_state = unit_state<OverlapState, ENG_EXT_OVERLAP>;

// room for `want` entries of `width` bytes with the first `keep` entries kept: a column that grows by half of itself
bool grow(DevBuf* b, uint64_t keep, uint64_t want, size_t width, hipStream_t st) {
  if (want * width <= b->cap) return true;
  DevBuf nb;
  if (!nb.ensure((size_t)std::max<uint64_t>(want + want / 2, 1024) * width)) return false;
  if (keep > 0 && (hipMemcpyAsync(nb.p, b->p, keep * width, hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) {
    (void)hipGetLastError();
    return false;
  }
  *b = std::move(nb);  // (frees what it held)
  return true;
}

// the run of places from `first`: k_ovl_window's six words
int window_of(simmr_engine* e, OverlapState* s, uint64_t first, uint64_t max_bytes, uint64_t fixed_places, uint64_t out[6], const char* what) {
  if (s->n == 0) {
    for (int i = 0; i < 6; i++) out[i] = 0;
    return SIMMR_OK;
  }
  hipStream_t st = eng_stream(e);
  hipLaunchKernelGGL(k_ovl_window, dim3(1), dim3(256), 0, st, s->sorted, s->rprefix.as<const uint64_t>(), first, max_bytes, fixed_places, s->win_p());
  HIP_TRY(e, hipMemcpyAsync(out, s->win_p(), 48, hipMemcpyDeviceToHost, st));
  return sync_check(e, what);
}

int need_plan(simmr_engine* e, OverlapState* s, const char* who) {
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "%s called before simmr_overlap_reset", who);
  if (s->epoch != eng_staging_epoch(e)) return eng_fail(e, SIMMR_ESTATE, "a genome was staged since simmr_overlap_reset: the rows are the reset's");
  if (!s->planned) return eng_fail(e, SIMMR_ESTATE, "%s called without a simmr_overlap_plan for the reads added", who);
  return SIMMR_OK;
}

}  // namespace

extern "C" {

int simmr_overlap_reset(simmr_engine* e, int paired) {
  if (!e) return SIMMR_EINVAL;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  OverlapState* s = overlap_state(e, true);
  s->ready = s->planned = false;
  s->n = 0;
  if (int rc = sync_check(e, "overlap reset")) return rc;
  if (int rc = s->sp.create_missing(e)) return rc;
  StagedRows rows = staged_rows(e);
  const uint32_t n_slots = rows.n_slots();
  std::vector<uint32_t>& cbase = rows.cbase;
  std::vector<uint32_t>& ncontig = rows.ncontig;
  std::vector<uint64_t>& bases = rows.bases;
  const uint64_t longest = rows.longest;
  cbase.resize(std::max(n_slots, 1u), 0u);
  ncontig.resize(std::max(n_slots, 1u), 0u);
  s->n_rows = bases.size();
  if (bases.empty()) bases.push_back(0);
  // the sort key has one row more than the engine: where reads shorter than min_overlap go
  uint32_t pos_bits = 0, row_bits = 0;
  if (simmr_sam_sort_key_bits(s->n_rows + 1, longest, &pos_bits, &row_bits) != SIMMR_OK)
    return eng_fail(e, SIMMR_ERANGE, "simmr_overlap_reset: %llu contigs, the longest of %llu bases: the key takes fewer than 2^24 contigs of fewer "
                                     "than 2^40 bases", (unsigned long long)s->n_rows, (unsigned long long)longest);
  if (!s->g_cbase.ensure(cbase.size() * 4) || !s->g_ncontig.ensure(ncontig.size() * 4) || !s->c_bases.ensure(bases.size() * 8) || !s->word.ensure(64))
    return eng_fail(e, SIMMR_ENOMEM, "overlap reset allocation failed");
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemcpyAsync(s->g_cbase.p, cbase.data(), cbase.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(e, hipMemcpyAsync(s->g_ncontig.p, ncontig.data(), ncontig.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(e, hipMemcpyAsync(s->c_bases.p, bases.data(), bases.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(e, hipMemsetAsync(s->word.p, 0, 64, st));
  if (int rc = sync_check(e, "overlap reset")) return rc;  // (the tables were copied from vectors of this call)
  s->n_slots = n_slots;
  s->pos_bits = pos_bits;
  s->key_bits = pos_bits + row_bits;
  s->paired = paired ? 1u : 0u;
  s->epoch = eng_staging_epoch(e);
  s->ready = true;
  return SIMMR_OK;
}

int simmr_overlap_add(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads) {
  if (!e) return SIMMR_EINVAL;
  if (!reads) return eng_fail(e, SIMMR_EINVAL, "simmr_overlap_add: NULL argument");
  if (!reads->start || !reads->end || !reads->contig || !reads->genome || !reads->read_id || !reads->flags)
    return eng_fail(e, SIMMR_EINVAL, "simmr_overlap_add needs start, end, contig, genome, read_id and flags");
  OverlapState* s = overlap_state(e, false);
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_overlap_add called before simmr_overlap_reset");
  if (s->epoch != eng_staging_epoch(e)) return eng_fail(e, SIMMR_ESTATE, "a genome was staged since simmr_overlap_reset: the rows are the reset's");
  if (s->paired && (n_reads & 1u)) return eng_fail(e, SIMMR_EINVAL, "simmr_overlap_add: paired with an odd number of reads");
  if (n_reads >= (1ull << 31) || s->n + n_reads >= (1ull << 31))
    return eng_fail(e, SIMMR_ERANGE, "the reads added since simmr_overlap_reset would reach 2^31");
  s->planned = false;
  if (n_reads == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t want = s->n + n_reads;
  if (!grow(&s->key, s->n, want, 8, st) || !grow(&s->meta, s->n, want, 8, st) || !grow(&s->rid, s->n, want, 4, st))
    return eng_fail(e, SIMMR_ENOMEM, "overlap columns allocation failed (%llu reads)", (unsigned long long)want);
  HIP_TRY(e, hipMemsetAsync(s->word.p, 0, 4, st));
  hipLaunchKernelGGL(k_ovl_add, dim3((uint32_t)((n_reads + 255) / 256)), dim3(256), 0, st, reads->start, reads->end, reads->contig, reads->genome,
                     reads->read_id, reads->flags, n_reads, s->rows(), s->paired, s->key.as<uint64_t>() + s->n, s->meta.as<uint64_t>() + s->n,
                     s->rid.as<uint32_t>() + s->n, s->err_p());
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "overlap add")) return rc;
  if (errw)
    return eng_fail(e, SIMMR_EINVAL, "a read's genome slot or contig is not staged, or the read ends behind its contig's staged length: nothing "
                                     "of this call was added");
  s->n = want;
  return SIMMR_OK;
}

int simmr_overlap_plan(simmr_engine* e, uint64_t min_overlap, uint64_t* n_reads, uint64_t* n_pairs, uint64_t* total_bytes) {
  if (!e) return SIMMR_EINVAL;
  OverlapState* s = overlap_state(e, false);
  if (s) s->planned = false;
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_overlap_plan called before simmr_overlap_reset");
  if (s->epoch != eng_staging_epoch(e)) return eng_fail(e, SIMMR_ESTATE, "a genome was staged since simmr_overlap_reset: the rows are the reset's");
  if (min_overlap < 1) return eng_fail(e, SIMMR_EINVAL, "simmr_overlap_plan: min_overlap is at least 1");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  const uint64_t n = s->n, n1 = std::max<uint64_t>(n, 1);
  const uint64_t n_chunks = (n + SAM_CHUNK - 1) / SAM_CHUNK, n_tiles = (n + SAMSORT_PAIRS_TILE - 1) / SAMSORT_PAIRS_TILE;
  if (!s->skey[0].ensure(n1 * 8) || !s->skey[1].ensure(n1 * 8) || !s->sidx[0].ensure(n1 * 4) || !s->sidx[1].ensure(n1 * 4) ||
      !s->hist.ensure(std::max<uint64_t>(n_tiles, 1) * SAMSORT_PAIRS_DIGITS * 4) || !s->digit_total.ensure(SAMSORT_PAIRS_DIGITS * 4) ||
      !s->smeta.ensure(n1 * 8) || !s->srid.ensure(n1 * 4) || !s->cnt.ensure(n1 * 4) || !s->rec_off.ensure((n + 1) * 8) ||
      !s->chunk_sum.ensure(std::max<uint64_t>(n_chunks, 1) * 8) || !s->chunk_prefix.ensure((n_chunks + 1) * 8))
    return eng_fail(e, SIMMR_ENOMEM, "overlap plan allocation failed (%llu reads)", (unsigned long long)n);
  hipStream_t st = eng_stream(e);
  const uint32_t cap = (uint32_t)eng_cu_count(e) * OVL_WGS_PER_CU;
  HIP_TRY(e, s->sp.begin(0, st));
  uint64_t pairs = 0, total = 0;
  s->sorted = OvlSorted{};
  if (n > 0) {
    hipLaunchKernelGGL(k_ovl_keys, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, s->key.as<const uint64_t>(), s->meta.as<const uint64_t>(), n,
                       min_overlap, s->pos_bits, s->n_rows, s->skey[0].as<uint64_t>());
    uint64_t* const keys[2] = {s->skey[0].as<uint64_t>(), s->skey[1].as<uint64_t>()};
    uint32_t* const idxs[2] = {s->sidx[0].as<uint32_t>(), s->sidx[1].as<uint32_t>()};
    const int cur = samsort_sort_pairs(st, keys, idxs, s->hist.as<uint32_t>(), s->digit_total.as<uint32_t>(), n, s->key_bits);
    const uint32_t* perm = s->key_bits > 0u ? s->sidx[cur].as<const uint32_t>() : nullptr;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_chunks, cap);
    hipLaunchKernelGGL(k_ovl_partners, dim3(grid), dim3(256), 0, st, s->skey[cur].as<const uint64_t>(), perm, s->meta.as<const uint64_t>(),
                       s->rid.as<const uint32_t>(), n, min_overlap, s->pos_bits, s->n_rows, s->smeta.as<uint64_t>(), s->srid.as<uint32_t>(),
                       s->cnt.as<uint32_t>(), s->chunk_sum.as<uint64_t>());
    hipLaunchKernelGGL(k_ovl_scan, dim3(1), dim3(256), 0, st, s->chunk_sum.as<const uint64_t>(), s->chunk_prefix.as<uint64_t>(), n_chunks);
    hipLaunchKernelGGL(k_ovl_offsets, dim3(grid), dim3(256), 0, st, s->cnt.as<const uint32_t>(), s->chunk_prefix.as<const uint64_t>(), n,
                       s->rec_off.as<uint64_t>());
    HIP_TRY(e, hipMemcpyAsync(&pairs, s->rec_off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    if (int rc = sync_check(e, "overlap sort and partner count")) return rc;  // (the number of records sizes the second scan)
    const uint64_t r_chunks = (pairs + OVL_CHUNK - 1) / OVL_CHUNK;
    if (!s->rsum.ensure(std::max<uint64_t>(r_chunks, 1) * 8) || !s->rprefix.ensure((r_chunks + 1) * 8))
      return eng_fail(e, SIMMR_ENOMEM, "overlap plan allocation failed (%llu records)", (unsigned long long)pairs);
    s->sorted = OvlSorted{s->skey[cur].as<const uint64_t>(), s->smeta.as<const uint64_t>(), s->srid.as<const uint32_t>(), perm,
                          s->rec_off.as<const uint64_t>(), n, pairs, s->pos_bits, s->paired};
    hipLaunchKernelGGL(k_ovl_size, dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(r_chunks, cap))), dim3(256), 0, st, s->sorted,
                       s->rsum.as<uint64_t>());
    hipLaunchKernelGGL(k_ovl_scan, dim3(1), dim3(256), 0, st, s->rsum.as<const uint64_t>(), s->rprefix.as<uint64_t>(), r_chunks);
    HIP_TRY(e, hipMemcpyAsync(&total, s->rprefix.as<uint64_t>() + r_chunks, 8, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(e, s->sp.end(0, st));
  if (int rc = sync_check(e, "overlap size pass and scan")) return rc;
  s->min_overlap = min_overlap;
  s->total = total;
  s->emit_ms = 0.f;
  s->planned = true;
  s->sp.mark(0);
  if (n_reads) *n_reads = n;
  if (n_pairs) *n_pairs = pairs;
  if (total_bytes) *total_bytes = total;
  return SIMMR_OK;
}

int simmr_overlap_window(simmr_engine* e, uint64_t first_place, uint64_t max_bytes, uint64_t* n_places, uint64_t* n_pairs, uint64_t* bytes) {
  if (!e) return SIMMR_EINVAL;
  OverlapState* s = overlap_state(e, false);
  if (int rc = need_plan(e, s, "simmr_overlap_window")) return rc;
  if (first_place > s->n) return eng_fail(e, SIMMR_EINVAL, "simmr_overlap_window: place %llu of %llu", (unsigned long long)first_place, (unsigned long long)s->n);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  uint64_t w[6];
  if (int rc = window_of(e, s, first_place, max_bytes, ~0ull, w, "overlap window")) return rc;
  if (w[0] == 0 && first_place < s->n) {  // the first place alone does not fit
    if (n_places) *n_places = 0;
    if (n_pairs) *n_pairs = 0;
    if (bytes) *bytes = w[5];
    return eng_fail(e, SIMMR_ERANGE, "the records of place %llu take %llu bytes, more than max_bytes %llu", (unsigned long long)first_place,
                    (unsigned long long)w[5], (unsigned long long)max_bytes);
  }
  if (n_places) *n_places = w[0];
  if (n_pairs) *n_pairs = w[2] - w[1];
  if (bytes) *bytes = w[4] - w[3];
  return SIMMR_OK;
}

int simmr_overlap_emit(simmr_engine* e, uint64_t first_place, uint64_t n_places, const simmr_overlap_cols* cols, uint8_t* dst,
                       uint64_t dst_capacity) {
  if (!e) return SIMMR_EINVAL;
  OverlapState* s = overlap_state(e, false);
  if (int rc = need_plan(e, s, "simmr_overlap_emit")) return rc;
  if (first_place > s->n || n_places > s->n - first_place)
    return eng_fail(e, SIMMR_EINVAL, "simmr_overlap_emit: places %llu + %llu of %llu", (unsigned long long)first_place, (unsigned long long)n_places,
                    (unsigned long long)s->n);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  uint64_t w[6];
  if (int rc = window_of(e, s, first_place, 0, n_places, w, "overlap emit")) return rc;
  const uint64_t j0 = w[1], j1 = w[2], b0 = w[3], bytes = w[4] - w[3];
  OvlCols c{};
  if (cols) c = OvlCols{cols->a, cols->b, cols->ref_start, cols->ref_end, cols->row};
  const bool any = c.a || c.b || c.ref_start || c.ref_end || c.row;
  if (dst && dst_capacity < bytes)
    return eng_fail(e, SIMMR_ERANGE, "dst_capacity %llu < %llu bytes of these places", (unsigned long long)dst_capacity, (unsigned long long)bytes);
  if (any && cols->capacity < j1 - j0)
    return eng_fail(e, SIMMR_ERANGE, "cols->capacity %llu < %llu records of these places", (unsigned long long)cols->capacity, (unsigned long long)(j1 - j0));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, s->sp.begin(1, st));
  if (j1 > j0 && (dst || any)) {
    const uint64_t chunks = (j1 + OVL_CHUNK - 1) / OVL_CHUNK - j0 / OVL_CHUNK;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(chunks, (uint64_t)eng_cu_count(e) * OVL_WGS_PER_CU);
    hipLaunchKernelGGL(k_ovl_write, dim3(grid), dim3(256), 0, st, s->sorted, s->rprefix.as<const uint64_t>(), j0, j1, b0, bytes, dst, c);
  }
  HIP_TRY(e, s->sp.end(1, st));
  if (int rc = sync_check(e, "overlap write pass")) return rc;
  float ms = 0.f;
  HIP_TRY(e, hipEventElapsedTime(&ms, s->sp.ev[2], s->sp.ev[3]));
  s->emit_ms += ms;
  return SIMMR_OK;
}

int simmr_last_overlap_ms(simmr_engine* e, float* ms) {
  if (!e || !ms) return SIMMR_EINVAL;
  OverlapState* s = overlap_state(e, false);
  if (!s || !s->sp.valid[0]) return eng_fail(e, SIMMR_ESTATE, "no simmr_overlap_plan yet");
  float plan = 0.f;
  if (int rc = s->sp.total_ms(e, "overlap", &plan)) return rc;
  *ms = plan + s->emit_ms;
  return SIMMR_OK;
}

}  // extern "C"
