// sam.hip — the true alignments as SAM text (include/simmr_hip.h: simmr_sam_*): the entry points over sam_kernels.hip.
// The sixth translation unit of libsimmr_hip.so; it sees an engine through engine_internal.hpp only — the device, the
// stream, which slots are staged and the staging epoch: the pass reads the caller's columns, never the genome planes —
// and keeps its state in the engine's opaque slot (freed by simmr_engine_destroy through the hook given there).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "sam_kernels.hip"
#include "sam_names.hpp"

using namespace simmr;

namespace {

struct SamState {
  SamNameTable nt;  // the names of the last plan (sam_names.hpp)
  DevBuf len, off, chunk_sum, chunk_prefix;
  DevBuf word;  // the total (64 bits), then the error word
  // what the plan was made for: every column and both capacities, as the kernels read them
  SamReads reads{};
  SamEdits edits{};
  uint32_t paired = 0;
  uint64_t n_reads = 0, total = 0, epoch = 0;
  bool ready = false, planned_once = false, emitted = false;
  hipEvent_t ev[4] = {};

  SamNames names() const { return nt.names(); }
  uint32_t* err_p() const { return (uint32_t*)(word.as<char>() + 8); }
};

void sam_destroy(void* q) {
  SamState* s = (SamState*)q;
  s->nt.release();
  for (DevBuf* b : {&s->len, &s->off, &s->chunk_sum, &s->chunk_prefix, &s->word}) b->release();
  for (hipEvent_t ev : s->ev)
    if (ev) (void)hipEventDestroy(ev);
  delete s;
}

SamState* state_of(simmr_engine* e, bool create) {
  void** slot = eng_ext_slot(e, ENG_EXT_SAM, sam_destroy);
  if (!*slot && create) *slot = new SamState();
  return (SamState*)*slot;
}

}  // namespace

extern "C" {

int simmr_sam_plan(simmr_engine* e, const simmr_sam_names* names, const simmr_reads_out* reads, const simmr_truth_out* truth,
                   uint64_t n_reads, int paired, uint64_t* total_bytes) {
  if (!e) return SIMMR_EINVAL;
  if (SamState* old = state_of(e, false)) old->ready = old->emitted = false;
  if (int rc = check_plan_args(e, names, reads, truth, n_reads, paired, total_bytes, "simmr_sam_plan")) return rc;
  // ---- the names: a row per contig of every entry, the RNAMEs back to back
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  SamState* s = state_of(e, true);
  if (int rc = sam_sync_check(e, "SAM plan")) return rc;  // (an upload of an earlier plan that failed may still read the host copies)
  if (int rc = s->nt.build(e, names)) return rc;
  for (hipEvent_t& ev : s->ev)
    if (!ev) SAM_TRY(e, hipEventCreate(&ev));
  const uint64_t n_chunks = (n_reads + SAM_CHUNK - 1) / SAM_CHUNK;
  if (!s->nt.ensure(false) || !s->len.ensure(std::max<uint64_t>(n_reads, 1) * 4) || !s->off.ensure((n_reads + 1) * 8) ||
      !s->chunk_sum.ensure(std::max<uint64_t>(n_chunks, 1) * 8) || !s->chunk_prefix.ensure((n_chunks + 1) * 8) || !s->word.ensure(16))
    return eng_fail(e, SIMMR_ENOMEM, "SAM plan allocation failed (%llu reads)", (unsigned long long)n_reads);
  hipStream_t st = eng_stream(e);
  SAM_TRY(e, s->nt.upload(st, false));
  SAM_TRY(e, hipMemsetAsync(s->word.p, 0, 16, st));
  SAM_TRY(e, hipEventRecord(s->ev[0], st));
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_chunks, (uint64_t)eng_cu_count(e) * SAM_WGS_PER_CU));
  if (n_reads > 0)
    hipLaunchKernelGGL(k_sam_size, dim3(grid), dim3(256), 0, st, sam_reads(reads), sam_edits(truth), s->names(), n_reads, paired ? 1u : 0u,
                       s->len.as<uint32_t>(), s->chunk_sum.as<uint64_t>(), s->err_p());
  hipLaunchKernelGGL(k_sam_scan, dim3(1), dim3(256), 0, st, s->chunk_sum.as<const uint64_t>(), s->chunk_prefix.as<uint64_t>(), n_chunks);
  hipLaunchKernelGGL(k_sam_offsets, dim3(grid), dim3(256), 0, st, s->len.as<const uint32_t>(), s->chunk_prefix.as<const uint64_t>(), n_reads,
                     s->off.as<uint64_t>());
  SAM_TRY(e, hipEventRecord(s->ev[1], st));
  uint64_t total = 0;
  uint32_t errw = 0;
  SAM_TRY(e, hipMemcpyAsync(&total, s->off.as<uint64_t>() + n_reads, 8, hipMemcpyDeviceToHost, st));
  SAM_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sam_sync_check(e, "SAM size pass")) return rc;
  s->planned_once = true;
  if (errw)
    return eng_fail(e, SIMMR_EINVAL, "a read's genome / contig has no name, its bytes leave seq[], it is longer than %u bases, its edit_off "
                                     "decreases or leaves edits_capacity, or its edit_pos do not ascend inside the read", SAM_MAX_L);
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

int simmr_sam_emit(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* truth, uint8_t* dst, uint64_t dst_capacity) {
  if (!e) return SIMMR_EINVAL;
  if (!reads || !truth) return eng_fail(e, SIMMR_EINVAL, "simmr_sam_emit: NULL argument");
  SamState* s = state_of(e, false);
  if (s) s->emitted = false;
  SamReads now_r{};  // (zeroed first: the structs are compared as bytes, padding included)
  SamEdits now_e{};
  std::memset(&now_r, 0, sizeof now_r);
  std::memset(&now_e, 0, sizeof now_e);
  assign_reads(&now_r, reads);
  assign_edits(&now_e, truth);
  if (!s || !s->ready || std::memcmp(&now_r, &s->reads, sizeof now_r) != 0 || std::memcmp(&now_e, &s->edits, sizeof now_e) != 0)
    return eng_fail(e, SIMMR_ESTATE, "simmr_sam_emit called without a simmr_sam_plan for these columns");
  if (s->epoch != eng_staging_epoch(e)) return eng_fail(e, SIMMR_ESTATE, "a genome was staged since simmr_sam_plan: plan again");
  if (int rc = check_columns(e, reads, truth, "simmr_sam_emit")) return rc;
  if (dst_capacity < s->total)
    return eng_fail(e, SIMMR_ERANGE, "dst_capacity %llu < %llu bytes planned", (unsigned long long)dst_capacity, (unsigned long long)s->total);
  if (s->total > 0 && !dst) return eng_fail(e, SIMMR_EINVAL, "simmr_sam_emit: NULL dst");
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  SAM_TRY(e, hipEventRecord(s->ev[2], st));
  if (s->n_reads > 0) {
    const uint64_t n_batches = (s->n_reads + SAM_WG_READS - 1) / SAM_WG_READS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_batches, (uint64_t)eng_cu_count(e) * SAM_WGS_PER_CU);
    hipLaunchKernelGGL(k_sam_write, dim3(grid), dim3(256), 0, st, s->reads, s->edits, s->names(), s->n_reads, s->paired,
                       s->off.as<const uint64_t>(), dst, s->err_p());
  }
  SAM_TRY(e, hipEventRecord(s->ev[3], st));
  uint32_t errw = 0;
  SAM_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sam_sync_check(e, "SAM write pass")) return rc;
  s->emitted = true;
  if (errw) {
    s->ready = false;
    return eng_fail(e, SIMMR_EINVAL, "the columns changed since simmr_sam_plan: a read failed the bounds check of the write pass (no store "
                                     "left its record)");
  }
  return SIMMR_OK;
}

int simmr_last_sam_ms(simmr_engine* e, float* ms) {
  if (!e || !ms) return SIMMR_EINVAL;
  SamState* s = state_of(e, false);
  if (!s || !s->planned_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_sam_plan yet");
  if (int rc = sam_sync_check(e, "sam")) return rc;
  float a = 0.f, b = 0.f;
  SAM_TRY(e, hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
  if (s->emitted) SAM_TRY(e, hipEventElapsedTime(&b, s->ev[2], s->ev[3]));
  *ms = a + b;
  return SIMMR_OK;
}

}  // extern "C"
