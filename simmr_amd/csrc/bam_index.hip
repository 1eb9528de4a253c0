// bam_index.hip — the BAM records in coordinate order and the BAI index of a sorted record stream (include/simmr_hip.h:
// simmr_bam_sort_*, simmr_bai_*): the entry points over bam_index_kernels.hip.  A translation unit of libsimmr_hip.so of its
// own; it sees an engine through engine_internal.hpp only.  The engine's slot enum is full, so the state lives in an object of
// its own that the caller creates on an engine and destroys before the engine (simmr_bam_sort_create / _destroy).  The names
// table and the argument checks are sam.hip's (sam_names.hpp), the sort is sam_sort.hip's (samsort_sort_pairs); the plan, the emit
// and the timer of the sorted records are the shared ones of record_stream_host.hpp, given this unit's traits (BamSortFormat, whose
// state is the handle's).  simmr_bai_* is this unit's alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "bam_index_kernels.hip"
#include "record_stream_host.hpp"
#include "scorer_host.hpp"

using namespace simmr;

static_assert(BAI_KEY_POS_BITS == 40u, "the canonical key of simmr_sam_sort_emit");

namespace {

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
};

uint32_t item_grid(simmr_engine* e, uint64_t n) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)eng_cu_count(e) * 32u));
}

}  // namespace

struct simmr_bam_sort {
  simmr_engine* e = nullptr;
  RecordStreamState s;
  BaiState b;
};

namespace {

struct BamSortFormat : RecordFormat {
  static constexpr bool SORTED = true, WITH_END = true;
  static constexpr const char *PLAN = "simmr_bam_sort_plan", *EMIT = "simmr_bam_sort_emit", *NOUN = "sorted BAM", *TIMER = "sorted bam";
  static constexpr const char *SYNC_PLAN = "sorted BAM plan", *SYNC_SIZE = "sorted BAM size and sort passes", *SYNC_WRITE = "sorted BAM write pass";
  static constexpr const char* PLAN_REFUSAL =
      "a read's bytes leave seq[], it is longer than %u bases, it ends at 2^31 or beyond, its edit_off decreases or leaves edits_capacity, or its "
      "edit_pos do not ascend inside the read";
  static simmr_engine* engine(simmr_bam_sort* h) { return h->e; }
  static RecordStreamState* state(simmr_bam_sort* h, bool) { return &h->s; }
  static void size(hipStream_t st, uint32_t grid, RecordStreamState& s, const SamReads& rd, const SamEdits& ed, uint64_t n, uint32_t paired, uint32_t pos_bits) {
    hipLaunchKernelGGL(k_bamsort_size, dim3(grid), dim3(256), 0, st, rd, ed, s.nt.names(), s.nt.c_bases.as<const uint64_t>(), n, paired, pos_bits,
                       s.len.as<uint32_t>(), s.key[0].as<uint64_t>(), s.end.as<uint32_t>(), s.err_p());
  }
  static void gather(hipStream_t st, uint32_t grid, RecordStreamState& s, uint64_t n, uint32_t pos_bits, int cur) {
    hipLaunchKernelGGL(k_bamsort_gather, dim3(grid), dim3(256), 0, st, s.len.as<const uint32_t>(), s.end.as<const uint32_t>(), s.key[cur].as<const uint64_t>(),
                       s.perm, n, pos_bits, s.idx[cur ^ 1].as<uint32_t>(), s.send.as<uint32_t>(), s.key[cur ^ 1].as<uint64_t>(), s.chunk_sum.as<uint64_t>());
  }
  static void scan(hipStream_t st, RecordStreamState& s, uint64_t n_chunks) {
    hipLaunchKernelGGL(k_bamsort_scan, dim3(1), dim3(256), 0, st, s.chunk_sum.as<const uint64_t>(), s.chunk_prefix.as<uint64_t>(), n_chunks);
  }
  static void offsets(hipStream_t st, uint32_t grid, RecordStreamState& s, const uint32_t* slen, uint64_t n) {
    hipLaunchKernelGGL(k_bamsort_offsets, dim3(grid), dim3(256), 0, st, slen, s.chunk_prefix.as<const uint64_t>(), n, s.off.as<uint64_t>());
  }
  static void write(hipStream_t st, uint32_t grid, RecordStreamState& s, uint8_t* dst) {
    hipLaunchKernelGGL(k_bamsort_write, dim3(grid), dim3(256), 0, st, s.reads, s.edits, s.nt.names(), s.n_reads, s.paired, s.perm,
                       s.off.as<const uint64_t>(), dst, s.err_p());
  }
};

}  // namespace

extern "C" {

int simmr_bam_sort_create(simmr_engine* e, simmr_bam_sort** out) { return scorer_create(e, out, "simmr_bam_sort_create"); }

void simmr_bam_sort_destroy(simmr_bam_sort* h) { scorer_destroy(h); }

int simmr_bam_sort_plan(simmr_bam_sort* h, const simmr_sam_names* names, const simmr_reads_out* reads, const simmr_truth_out* truth,
                        uint64_t n_reads, int paired, uint64_t* record_bytes) {
  return record_plan<BamSortFormat>(h, names, reads, truth, n_reads, paired, record_bytes);
}

int simmr_bam_sort_emit(simmr_bam_sort* h, const simmr_reads_out* reads, const simmr_truth_out* truth, uint8_t* dst, uint64_t dst_capacity,
                        uint64_t* key_out, uint64_t* rec_off_out, uint32_t* end_out) {
  return record_emit<BamSortFormat>(h, reads, truth, dst, dst_capacity, key_out, rec_off_out, end_out);
}

int simmr_last_bam_sort_ms(simmr_bam_sort* h, float* ms) { return record_ms<BamSortFormat>(h, ms); }

int simmr_bam_sort_ref_lengths(simmr_bam_sort* h, uint64_t* lengths, uint64_t capacity, uint64_t* n_rows) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!n_rows) return eng_fail(e, SIMMR_EINVAL, "simmr_bam_sort_ref_lengths: NULL n_rows");
  if (!h->s.sp.valid[0]) return eng_fail(e, SIMMR_ESTATE, "no simmr_bam_sort_plan yet");
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
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t n_chunks = (n + SAM_CHUNK - 1) / SAM_CHUNK;
  if (!b->rb.ensure(std::max<uint64_t>(n, 1) * 8) || !b->chunk_sum.ensure(std::max<uint64_t>(n_chunks, 1) * 8) || !b->chunk_prefix.ensure((n_chunks + 1) * 8) ||
      !b->ref_bin0.ensure((n_ref + 1) * 4) || !b->ref_rec0.ensure((n_ref + 1) * 4) || !b->ref_max_end.ensure(std::max<uint64_t>(n_ref, 1) * 4) ||
      !b->ref_intv.ensure(std::max<uint64_t>(n_ref, 1) * 4) || !b->ref_off.ensure((n_ref + 1) * 8) || !b->win_off.ensure((n_ref + 1) * 8) ||
      !b->digit_total.ensure(SAMSORT_PAIRS_DIGITS * 4) || !b->bin_first.ensure(4) || !b->word.ensure(16))
    return eng_fail(e, SIMMR_ENOMEM, "BAI plan allocation failed (%llu records, %llu references)", (unsigned long long)n, (unsigned long long)n_ref);
  HIP_TRY(e, hipMemsetAsync(b->word.p, 0, 16, st));
  HIP_TRY(e, hipMemsetAsync(b->ref_max_end.p, 0, std::max<uint64_t>(n_ref, 1) * 4, st));
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
    HIP_TRY(e, hipMemcpyAsync(&n_runs, b->chunk_prefix.as<uint64_t>() + n_chunks, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipMemcpyAsync(&errw, b->word.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipMemcpyAsync(&stream_end, rec_off + n, 8, hipMemcpyDeviceToHost, st));
    if (int rc = sync_check(e, "BAI check pass")) return rc;
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
    HIP_TRY(e, hipMemcpyAsync(&n_bins, b->chunk_prefix.as<uint64_t>() + run_chunks, 8, hipMemcpyDeviceToHost, st));
    if (int rc = sync_check(e, "BAI run sort")) return rc;
    if (!b->bin_key.ensure(n_bins * 8) || !b->bin_first.ensure((n_bins + 1) * 4))
      return eng_fail(e, SIMMR_ENOMEM, "BAI plan allocation failed (%llu bins)", (unsigned long long)n_bins);
    hipLaunchKernelGGL(k_bai_compact, dim3((uint32_t)run_chunks), dim3(256), 0, st, skey, n_runs, b->chunk_prefix.as<const uint64_t>(), n_bins,
                       b->bin_key.as<uint64_t>(), b->bin_first.as<uint32_t>());
    hipLaunchKernelGGL(k_bai_refs, dim3(item_grid(e, n_ref + 1)), dim3(256), 0, st, b->bin_key.as<const uint64_t>(), n_bins, key, n, n_ref,
                       b->ref_bin0.as<uint32_t>(), b->ref_rec0.as<uint32_t>());
  } else {
    HIP_TRY(e, hipMemsetAsync(b->ref_bin0.p, 0, (n_ref + 1) * 4, st));
    HIP_TRY(e, hipMemsetAsync(b->ref_rec0.p, 0, (n_ref + 1) * 4, st));
    HIP_TRY(e, hipMemsetAsync(b->bin_first.p, 0, 4, st));
  }
  hipLaunchKernelGGL(k_bai_layout, dim3(1), dim3(256), 0, st, b->ref_bin0.as<const uint32_t>(), b->bin_first.as<const uint32_t>(),
                     b->ref_max_end.as<const uint32_t>(), n_ref, b->ref_intv.as<uint32_t>(), b->ref_off.as<uint64_t>(), b->win_off.as<uint64_t>());
  uint64_t body = 0, n_windows = 0;
  HIP_TRY(e, hipMemcpyAsync(&body, b->ref_off.as<uint64_t>() + n_ref, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&n_windows, b->win_off.as<uint64_t>() + n_ref, 8, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "BAI layout")) return rc;
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
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemsetAsync(b->win.p, 0xff, std::max<uint64_t>(b->n_windows, 1) * 8, st));
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
  if (int rc = sync_check(e, "BAI write pass")) return rc;
  return SIMMR_OK;
}

}  // extern "C"
