// bam_index.hip — the BAM records in coordinate order and the BAI index of a sorted record stream (include/simmr_hip.h:
// simmr_bam_sort_*, simmr_bai_*): the entry points over bam_index_kernels.hip.  A translation unit of libsimmr_hip.so of its
// own; it sees an engine through engine_internal.hpp only.  The engine's slot enum is full, so the state lives in an object of
// its own that the caller creates on an engine and destroys before the engine (simmr_bam_sort_create / _destroy).  The names
// table and the argument checks are sam.hip's (sam_names.hpp), the sort is sam_sort.hip's (samsort_sort_pairs).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "bam_index_kernels.hip"
#include "sam_names.hpp"

using namespace simmr;

static_assert(BAI_KEY_POS_BITS == 40u, "the canonical key of simmr_sam_sort_emit");

namespace {

uint32_t bits_of(uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }

struct SortState {
  SamNameTable nt;
  DevBuf len, end;         // per read
  DevBuf key[2], idx[2];   // the pairs, ping and pong; behind the sort the free key buffer holds the canonical keys and the
                           // free index buffer the sorted lengths
  DevBuf send;             // the ends in sorted order
  DevBuf hist, digit_total, rec_off, chunk_sum, chunk_prefix;
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
  void release() {
    nt.release();
    for (DevBuf* b : {&len, &end, &key[0], &key[1], &idx[0], &idx[1], &send, &hist, &digit_total, &rec_off, &chunk_sum, &chunk_prefix, &word})
      b->release();
    for (hipEvent_t& e : ev)
      if (e) { (void)hipEventDestroy(e); e = nullptr; }
  }
};

struct BaiState {
  DevBuf rb, chunk_sum, chunk_prefix;
  DevBuf run_key[2], run_idx[2], run_first, hist, digit_total;
  DevBuf bin_key, bin_first;
  DevBuf ref_bin0, ref_rec0, ref_max_end, ref_intv, ref_off, win_off, win;
  DevBuf word;
  // what the plan was made for
  const uint64_t* key = nullptr;
  const uint32_t* end = nullptr;
  const uint64_t* rec_off = nullptr;
  const uint32_t* run_perm = nullptr;
  uint64_t n = 0, n_ref = 0, base = 0, n_runs = 0, n_bins = 0, n_windows = 0, total = 0;
  bool ready = false;
  void release() {
    for (DevBuf* b : {&rb, &chunk_sum, &chunk_prefix, &run_key[0], &run_key[1], &run_idx[0], &run_idx[1], &run_first, &hist, &digit_total, &bin_key,
                      &bin_first, &ref_bin0, &ref_rec0, &ref_max_end, &ref_intv, &ref_off, &win_off, &win, &word})
      b->release();
  }
};

uint32_t item_grid(simmr_engine* e, uint64_t n) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)eng_cu_count(e) * 32u));
}

}  // namespace

struct simmr_bam_sort {
  simmr_engine* e = nullptr;
  SortState s;
  BaiState b;
};

extern "C" {

int simmr_bam_sort_create(simmr_engine* e, simmr_bam_sort** out) {
  if (!e) return SIMMR_EINVAL;
  if (!out) return eng_fail(e, SIMMR_EINVAL, "simmr_bam_sort_create: NULL out");
  *out = nullptr;
  simmr_bam_sort* h = new (std::nothrow) simmr_bam_sort();
  if (!h) return eng_fail(e, SIMMR_ENOMEM, "simmr_bam_sort_create: out of memory");
  h->e = e;
  *out = h;
  return SIMMR_OK;
}

void simmr_bam_sort_destroy(simmr_bam_sort* h) {
  if (!h) return;
  if (hipSetDevice(eng_device(h->e)) == hipSuccess) (void)hipStreamSynchronize(eng_stream(h->e));
  h->s.release();
  h->b.release();
  (void)hipGetLastError();
  delete h;
}

int simmr_bam_sort_plan(simmr_bam_sort* h, const simmr_sam_names* names, const simmr_reads_out* reads, const simmr_truth_out* truth,
                        uint64_t n_reads, int paired, uint64_t* record_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  SortState* s = &h->s;
  s->ready = s->emitted = false;
  if (int rc = check_plan_args(e, names, reads, truth, n_reads, paired, record_bytes, "simmr_bam_sort_plan")) return rc;
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = sam_sync_check(e, "sorted BAM plan")) return rc;  // (an upload of an earlier plan that failed may still read the host copies)
  if (int rc = s->nt.build(e, names)) return rc;
  uint32_t pos_bits = 0, row_bits = 0;
  if (simmr_sam_sort_key_bits(s->nt.n_rows, s->nt.longest, &pos_bits, &row_bits) != SIMMR_OK)
    return eng_fail(e, SIMMR_ERANGE, "simmr_bam_sort_plan: %llu named contigs, the longest of %llu bases: the key takes at most 2^24 contigs of "
                                     "fewer than 2^40 bases", (unsigned long long)s->nt.n_rows, (unsigned long long)s->nt.longest);
  const uint32_t key_bits = pos_bits + row_bits;
  for (hipEvent_t& ev : s->ev)
    if (!ev) SAM_TRY(e, hipEventCreate(&ev));
  const uint64_t n_chunks = (n_reads + SAM_CHUNK - 1) / SAM_CHUNK, n_tiles = (n_reads + SAMSORT_PAIRS_TILE - 1) / SAMSORT_PAIRS_TILE;
  const uint64_t n1 = std::max<uint64_t>(n_reads, 1);
  if (!s->nt.ensure(true) || !s->len.ensure(n1 * 4) || !s->end.ensure(n1 * 4) || !s->send.ensure(n1 * 4) || !s->key[0].ensure(n1 * 8) ||
      !s->key[1].ensure(n1 * 8) || !s->idx[0].ensure(n1 * 4) || !s->idx[1].ensure(n1 * 4) ||
      !s->hist.ensure(std::max<uint64_t>(n_tiles, 1) * SAMSORT_PAIRS_DIGITS * 4) || !s->digit_total.ensure(SAMSORT_PAIRS_DIGITS * 4) ||
      !s->rec_off.ensure((n_reads + 1) * 8) || !s->chunk_sum.ensure(std::max<uint64_t>(n_chunks, 1) * 8) ||
      !s->chunk_prefix.ensure((n_chunks + 1) * 8) || !s->word.ensure(16))
    return eng_fail(e, SIMMR_ENOMEM, "sorted BAM plan allocation failed (%llu reads)", (unsigned long long)n_reads);
  hipStream_t st = eng_stream(e);
  SAM_TRY(e, s->nt.upload(st, true));
  SAM_TRY(e, hipMemsetAsync(s->word.p, 0, 16, st));
  SAM_TRY(e, hipEventRecord(s->ev[0], st));
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, n_chunks);  // a workgroup per chunk (fewer than 2^21 of them)
  if (n_reads > 0) {
    hipLaunchKernelGGL(k_bamsort_size, dim3(grid), dim3(256), 0, st, sam_reads(reads), sam_edits(truth), s->nt.names(),
                       s->nt.c_bases.as<const uint64_t>(), n_reads, paired ? 1u : 0u, pos_bits, s->len.as<uint32_t>(), s->key[0].as<uint64_t>(),
                       s->end.as<uint32_t>(), s->err_p());
    uint64_t* const keys[2] = {s->key[0].as<uint64_t>(), s->key[1].as<uint64_t>()};
    uint32_t* const idxs[2] = {s->idx[0].as<uint32_t>(), s->idx[1].as<uint32_t>()};
    const int cur = samsort_sort_pairs(st, keys, idxs, s->hist.as<uint32_t>(), s->digit_total.as<uint32_t>(), n_reads, key_bits);
    s->perm = key_bits > 0u ? s->idx[cur].as<const uint32_t>() : nullptr;
    s->ckey = s->key[cur ^ 1].as<const uint64_t>();
    uint32_t* slen = s->idx[cur ^ 1].as<uint32_t>();
    hipLaunchKernelGGL(k_bamsort_gather, dim3(grid), dim3(256), 0, st, s->len.as<const uint32_t>(), s->end.as<const uint32_t>(),
                       s->key[cur].as<const uint64_t>(), s->perm, n_reads, pos_bits, slen, s->send.as<uint32_t>(), s->key[cur ^ 1].as<uint64_t>(),
                       s->chunk_sum.as<uint64_t>());
    hipLaunchKernelGGL(k_bamsort_scan, dim3(1), dim3(256), 0, st, s->chunk_sum.as<const uint64_t>(), s->chunk_prefix.as<uint64_t>(), n_chunks);
    hipLaunchKernelGGL(k_bamsort_offsets, dim3(grid), dim3(256), 0, st, (const uint32_t*)slen, s->chunk_prefix.as<const uint64_t>(), n_reads,
                       s->rec_off.as<uint64_t>());
  } else {
    SAM_TRY(e, hipMemsetAsync(s->rec_off.p, 0, 8, st));
  }
  SAM_TRY(e, hipEventRecord(s->ev[1], st));
  uint64_t total = 0;
  uint32_t errw = 0;
  SAM_TRY(e, hipMemcpyAsync(&total, s->rec_off.as<uint64_t>() + n_reads, 8, hipMemcpyDeviceToHost, st));
  SAM_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sam_sync_check(e, "sorted BAM size and sort passes")) return rc;
  s->planned_once = true;
  if (errw & 2u)
    return eng_fail(e, SIMMR_EINVAL, "a read's genome / contig has no name, or the read ends behind its contig's staged length");
  if (errw)
    return eng_fail(e, SIMMR_EINVAL, "a read's bytes leave seq[], it is longer than %u bases, it ends at 2^31 or beyond, its edit_off decreases or "
                                     "leaves edits_capacity, or its edit_pos do not ascend inside the read", SAM_MAX_L);
  s->reads = sam_reads(reads);
  s->edits = sam_edits(truth);
  s->paired = paired ? 1u : 0u;
  s->n_reads = n_reads;
  s->total = total;
  s->epoch = eng_staging_epoch(e);
  s->ready = true;
  *record_bytes = total;
  return SIMMR_OK;
}

int simmr_bam_sort_emit(simmr_bam_sort* h, const simmr_reads_out* reads, const simmr_truth_out* truth, uint8_t* dst, uint64_t dst_capacity,
                        uint64_t* key_out, uint64_t* rec_off_out, uint32_t* end_out) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  SortState* s = &h->s;
  if (!reads || !truth) return eng_fail(e, SIMMR_EINVAL, "simmr_bam_sort_emit: NULL argument");
  s->emitted = false;
  SamReads now_r{};  // (zeroed first: the structs are compared as bytes, padding included)
  SamEdits now_e{};
  std::memset(&now_r, 0, sizeof now_r);
  std::memset(&now_e, 0, sizeof now_e);
  assign_reads(&now_r, reads);
  assign_edits(&now_e, truth);
  if (!s->ready || std::memcmp(&now_r, &s->reads, sizeof now_r) != 0 || std::memcmp(&now_e, &s->edits, sizeof now_e) != 0)
    return eng_fail(e, SIMMR_ESTATE, "simmr_bam_sort_emit called without a simmr_bam_sort_plan for these columns");
  if (s->epoch != eng_staging_epoch(e)) return eng_fail(e, SIMMR_ESTATE, "a genome was staged since simmr_bam_sort_plan: plan again");
  if (int rc = check_columns(e, reads, truth, "simmr_bam_sort_emit")) return rc;
  if (dst_capacity < s->total)
    return eng_fail(e, SIMMR_ERANGE, "dst_capacity %llu < %llu bytes planned", (unsigned long long)dst_capacity, (unsigned long long)s->total);
  if (s->total > 0 && !dst) return eng_fail(e, SIMMR_EINVAL, "simmr_bam_sort_emit: NULL dst");
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  SAM_TRY(e, hipEventRecord(s->ev[2], st));
  if (s->n_reads > 0) {
    const uint64_t n_batches = (s->n_reads + SAM_WG_READS - 1) / SAM_WG_READS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_batches, (uint64_t)eng_cu_count(e) * SAM_WGS_PER_CU);
    hipLaunchKernelGGL(k_bamsort_write, dim3(grid), dim3(256), 0, st, s->reads, s->edits, s->nt.names(), s->n_reads, s->paired, s->perm,
                       s->rec_off.as<const uint64_t>(), dst, s->err_p());
    if (key_out) SAM_TRY(e, hipMemcpyAsync(key_out, s->ckey, s->n_reads * 8, hipMemcpyDeviceToDevice, st));
    if (end_out) SAM_TRY(e, hipMemcpyAsync(end_out, s->send.p, s->n_reads * 4, hipMemcpyDeviceToDevice, st));
  }
  if (rec_off_out) SAM_TRY(e, hipMemcpyAsync(rec_off_out, s->rec_off.p, (s->n_reads + 1) * 8, hipMemcpyDeviceToDevice, st));
  SAM_TRY(e, hipEventRecord(s->ev[3], st));
  uint32_t errw = 0;
  SAM_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sam_sync_check(e, "sorted BAM write pass")) return rc;
  s->emitted = true;
  if (errw) {
    s->ready = false;
    return eng_fail(e, SIMMR_EINVAL, "the columns changed since simmr_bam_sort_plan: a read failed the bounds check of the write pass (no store "
                                     "left its record)");
  }
  return SIMMR_OK;
}

int simmr_last_bam_sort_ms(simmr_bam_sort* h, float* ms) {
  if (!h || !ms) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  SortState* s = &h->s;
  if (!s->planned_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_bam_sort_plan yet");
  if (int rc = sam_sync_check(e, "sorted bam")) return rc;
  float a = 0.f, b = 0.f;
  SAM_TRY(e, hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
  if (s->emitted) SAM_TRY(e, hipEventElapsedTime(&b, s->ev[2], s->ev[3]));
  *ms = a + b;
  return SIMMR_OK;
}

int simmr_bam_sort_ref_lengths(simmr_bam_sort* h, uint64_t* lengths, uint64_t capacity, uint64_t* n_rows) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!n_rows) return eng_fail(e, SIMMR_EINVAL, "simmr_bam_sort_ref_lengths: NULL n_rows");
  if (!h->s.planned_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_bam_sort_plan yet");
  *n_rows = h->s.nt.n_rows;
  if (capacity < h->s.nt.n_rows) return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu rows", (unsigned long long)capacity, (unsigned long long)h->s.nt.n_rows);
  if (h->s.nt.n_rows > 0 && !lengths) return eng_fail(e, SIMMR_EINVAL, "simmr_bam_sort_ref_lengths: NULL lengths");
  for (uint64_t i = 0; i < h->s.nt.n_rows; i++) lengths[i] = h->s.nt.h_bases[i];
  return SIMMR_OK;
}

int simmr_bai_plan(simmr_bam_sort* h, const uint64_t* key, const uint32_t* end, const uint64_t* rec_off, uint64_t n, uint64_t n_ref,
                   const uint64_t* ref_len, uint64_t base, uint64_t* bai_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  BaiState* b = &h->b;
  b->ready = false;
  if (!bai_bytes) return eng_fail(e, SIMMR_EINVAL, "simmr_bai_plan: NULL bai_bytes");
  if (n > 0 && (!key || !end)) return eng_fail(e, SIMMR_EINVAL, "simmr_bai_plan: NULL column");
  if (!rec_off) return eng_fail(e, SIMMR_EINVAL, "simmr_bai_plan: NULL rec_off");
  if (n >= (1ull << 31)) return eng_fail(e, SIMMR_ERANGE, "simmr_bai_plan takes fewer than 2^31 records");
  if (n_ref > (1ull << 24)) return eng_fail(e, SIMMR_ERANGE, "simmr_bai_plan: %llu references: the key takes at most 2^24", (unsigned long long)n_ref);
  if (ref_len)
    for (uint64_t i = 0; i < n_ref; i++)
      if (ref_len[i] >= (uint64_t)BAI_MAX_END)
        return eng_fail(e, SIMMR_ERANGE, "reference %llu has %llu bases: a BAI index covers contigs of fewer than 2^29 bases (CSI is not written)",
                        (unsigned long long)i, (unsigned long long)ref_len[i]);
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t n_chunks = (n + SAM_CHUNK - 1) / SAM_CHUNK;
  if (!b->rb.ensure(std::max<uint64_t>(n, 1) * 8) || !b->chunk_sum.ensure(std::max<uint64_t>(n_chunks, 1) * 8) || !b->chunk_prefix.ensure((n_chunks + 1) * 8) ||
      !b->ref_bin0.ensure((n_ref + 1) * 4) || !b->ref_rec0.ensure((n_ref + 1) * 4) || !b->ref_max_end.ensure(std::max<uint64_t>(n_ref, 1) * 4) ||
      !b->ref_intv.ensure(std::max<uint64_t>(n_ref, 1) * 4) || !b->ref_off.ensure((n_ref + 1) * 8) || !b->win_off.ensure((n_ref + 1) * 8) ||
      !b->digit_total.ensure(SAMSORT_PAIRS_DIGITS * 4) || !b->bin_first.ensure(4) || !b->word.ensure(16))
    return eng_fail(e, SIMMR_ENOMEM, "BAI plan allocation failed (%llu records, %llu references)", (unsigned long long)n, (unsigned long long)n_ref);
  SAM_TRY(e, hipMemsetAsync(b->word.p, 0, 16, st));
  SAM_TRY(e, hipMemsetAsync(b->ref_max_end.p, 0, std::max<uint64_t>(n_ref, 1) * 4, st));
  uint64_t n_runs = 0, n_bins = 0;
  b->run_perm = nullptr;
  if (n > 0) {
    const uint32_t grid = (uint32_t)n_chunks;  // (fewer than 2^21)
    hipLaunchKernelGGL(k_bai_check, dim3(grid), dim3(256), 0, st, key, end, rec_off, n, n_ref, b->rb.as<uint64_t>(), b->ref_max_end.as<uint32_t>(),
                       b->word.as<uint32_t>());
    hipLaunchKernelGGL(k_bai_count, dim3(grid), dim3(256), 0, st, b->rb.as<const uint64_t>(), n, b->chunk_sum.as<uint64_t>());
    hipLaunchKernelGGL(k_bai_scan, dim3(1), dim3(256), 0, st, b->chunk_sum.as<const uint64_t>(), b->chunk_prefix.as<uint64_t>(), n_chunks);
    uint32_t errw = 0;
    uint64_t stream_end = 0;
    SAM_TRY(e, hipMemcpyAsync(&n_runs, b->chunk_prefix.as<uint64_t>() + n_chunks, 8, hipMemcpyDeviceToHost, st));
    SAM_TRY(e, hipMemcpyAsync(&errw, b->word.p, 4, hipMemcpyDeviceToHost, st));
    SAM_TRY(e, hipMemcpyAsync(&stream_end, rec_off + n, 8, hipMemcpyDeviceToHost, st));
    if (int rc = sam_sync_check(e, "BAI check pass")) return rc;
    if (errw & BAI_ERR_ORDER)
      return eng_fail(e, SIMMR_EINVAL, "simmr_bai_plan: the keys do not ascend, rec_off decreases, a record's reference is not below n_ref, or its "
                                       "interval is empty");
    if (errw & BAI_ERR_RANGE) return eng_fail(e, SIMMR_ERANGE, "simmr_bai_plan: a record ends beyond 2^29: a BAI index does not reach there");
    if (stream_end > (1ull << 62) || base > (1ull << 62) || ((base + stream_end) / BGZF_BLOCK + 1) * (uint64_t)BAI_BLOCK_FRAMED >= (1ull << 48))
      return eng_fail(e, SIMMR_ERANGE, "simmr_bai_plan: %llu bytes in front of %llu bytes of records: the compressed offset of a virtual offset has 48 bits",
                      (unsigned long long)base, (unsigned long long)stream_end);
    // the runs, compacted and sorted by (row, bin)
    const uint64_t run_tiles = (n_runs + SAMSORT_PAIRS_TILE - 1) / SAMSORT_PAIRS_TILE;
    if (!b->run_key[0].ensure(n_runs * 8) || !b->run_key[1].ensure(n_runs * 8) || !b->run_idx[0].ensure(n_runs * 4) || !b->run_idx[1].ensure(n_runs * 4) ||
        !b->run_first.ensure((n_runs + 1) * 4) || !b->hist.ensure(run_tiles * SAMSORT_PAIRS_DIGITS * 4))
      return eng_fail(e, SIMMR_ENOMEM, "BAI plan allocation failed (%llu runs)", (unsigned long long)n_runs);
    hipLaunchKernelGGL(k_bai_compact, dim3(grid), dim3(256), 0, st, b->rb.as<const uint64_t>(), n, b->chunk_prefix.as<const uint64_t>(), n_runs,
                       b->run_key[0].as<uint64_t>(), b->run_first.as<uint32_t>());
    uint64_t* const keys[2] = {b->run_key[0].as<uint64_t>(), b->run_key[1].as<uint64_t>()};
    uint32_t* const idxs[2] = {b->run_idx[0].as<uint32_t>(), b->run_idx[1].as<uint32_t>()};
    const uint32_t key_bits = BAI_BIN_BITS + (n_ref ? bits_of(n_ref - 1) : 0u);  // (>= 16: the sort always writes its index)
    const int cur = samsort_sort_pairs(st, keys, idxs, b->hist.as<uint32_t>(), b->digit_total.as<uint32_t>(), n_runs, key_bits);
    const uint64_t* skey = b->run_key[cur].as<const uint64_t>();
    b->run_perm = b->run_idx[cur].as<const uint32_t>();
    // the bins: the distinct keys of the sorted runs
    const uint64_t run_chunks = (n_runs + SAM_CHUNK - 1) / SAM_CHUNK;  // (<= n_chunks: the scan's buffers fit)
    hipLaunchKernelGGL(k_bai_count, dim3((uint32_t)run_chunks), dim3(256), 0, st, skey, n_runs, b->chunk_sum.as<uint64_t>());
    hipLaunchKernelGGL(k_bai_scan, dim3(1), dim3(256), 0, st, b->chunk_sum.as<const uint64_t>(), b->chunk_prefix.as<uint64_t>(), run_chunks);
    SAM_TRY(e, hipMemcpyAsync(&n_bins, b->chunk_prefix.as<uint64_t>() + run_chunks, 8, hipMemcpyDeviceToHost, st));
    if (int rc = sam_sync_check(e, "BAI run sort")) return rc;
    if (!b->bin_key.ensure(n_bins * 8) || !b->bin_first.ensure((n_bins + 1) * 4))
      return eng_fail(e, SIMMR_ENOMEM, "BAI plan allocation failed (%llu bins)", (unsigned long long)n_bins);
    hipLaunchKernelGGL(k_bai_compact, dim3((uint32_t)run_chunks), dim3(256), 0, st, skey, n_runs, b->chunk_prefix.as<const uint64_t>(), n_bins,
                       b->bin_key.as<uint64_t>(), b->bin_first.as<uint32_t>());
    hipLaunchKernelGGL(k_bai_refs, dim3(item_grid(e, n_ref + 1)), dim3(256), 0, st, b->bin_key.as<const uint64_t>(), n_bins, key, n, n_ref,
                       b->ref_bin0.as<uint32_t>(), b->ref_rec0.as<uint32_t>());
  } else {
    SAM_TRY(e, hipMemsetAsync(b->ref_bin0.p, 0, (n_ref + 1) * 4, st));
    SAM_TRY(e, hipMemsetAsync(b->ref_rec0.p, 0, (n_ref + 1) * 4, st));
    SAM_TRY(e, hipMemsetAsync(b->bin_first.p, 0, 4, st));
  }
  hipLaunchKernelGGL(k_bai_layout, dim3(1), dim3(256), 0, st, b->ref_bin0.as<const uint32_t>(), b->bin_first.as<const uint32_t>(),
                     b->ref_max_end.as<const uint32_t>(), n_ref, b->ref_intv.as<uint32_t>(), b->ref_off.as<uint64_t>(), b->win_off.as<uint64_t>());
  uint64_t body = 0, n_windows = 0;
  SAM_TRY(e, hipMemcpyAsync(&body, b->ref_off.as<uint64_t>() + n_ref, 8, hipMemcpyDeviceToHost, st));
  SAM_TRY(e, hipMemcpyAsync(&n_windows, b->win_off.as<uint64_t>() + n_ref, 8, hipMemcpyDeviceToHost, st));
  if (int rc = sam_sync_check(e, "BAI layout")) return rc;
  if (!b->win.ensure(std::max<uint64_t>(n_windows, 1) * 8)) return eng_fail(e, SIMMR_ENOMEM, "BAI plan allocation failed (%llu windows)", (unsigned long long)n_windows);
  b->key = key; b->end = end; b->rec_off = rec_off;
  b->n = n; b->n_ref = n_ref; b->base = base; b->n_runs = n_runs; b->n_bins = n_bins; b->n_windows = n_windows;
  b->total = body + 8;  // n_no_coor
  b->ready = true;
  *bai_bytes = b->total;
  return SIMMR_OK;
}

int simmr_bai_emit(simmr_bam_sort* h, uint8_t* dst, uint64_t dst_capacity) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  BaiState* b = &h->b;
  if (!b->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_bai_emit called without a simmr_bai_plan");
  if (dst_capacity < b->total)
    return eng_fail(e, SIMMR_ERANGE, "dst_capacity %llu < %llu bytes planned", (unsigned long long)dst_capacity, (unsigned long long)b->total);
  if (!dst) return eng_fail(e, SIMMR_EINVAL, "simmr_bai_emit: NULL dst");
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  SAM_TRY(e, hipMemsetAsync(b->win.p, 0xff, std::max<uint64_t>(b->n_windows, 1) * 8, st));
  if (b->n > 0) {
    hipLaunchKernelGGL(k_bai_windows, dim3(item_grid(e, b->n)), dim3(256), 0, st, b->key, b->end, b->rec_off, b->n, b->n_ref, b->base,
                       b->ref_intv.as<const uint32_t>(), b->win_off.as<const uint64_t>(), b->win.as<unsigned long long>());
    hipLaunchKernelGGL(k_bai_write_chunks, dim3(item_grid(e, b->n_runs)), dim3(256), 0, st, b->bin_key.as<const uint64_t>(), b->bin_first.as<const uint32_t>(),
                       b->n_bins, b->run_perm, b->run_first.as<const uint32_t>(), b->n_runs, b->rec_off, b->n, b->n_ref, b->base,
                       b->ref_bin0.as<const uint32_t>(), b->ref_off.as<const uint64_t>(), dst, b->total);
  }
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(b->n_ref, (uint64_t)eng_cu_count(e) * 8u));
  hipLaunchKernelGGL(k_bai_write_refs, dim3(grid), dim3(256), 0, st, b->ref_bin0.as<const uint32_t>(), b->ref_rec0.as<const uint32_t>(),
                     b->bin_first.as<const uint32_t>(), b->ref_intv.as<const uint32_t>(), b->ref_off.as<const uint64_t>(), b->win_off.as<const uint64_t>(),
                     b->win.as<const uint64_t>(), b->rec_off, b->n, b->n_ref, b->base, dst, b->total);
  if (int rc = sam_sync_check(e, "BAI write pass")) return rc;
  return SIMMR_OK;
}

}  // extern "C"
