// truth.hip — ground truth per read (include/simmr_hip.h: simmr_truth_*): the entry points over truth_kernels.hip.  A
// translation unit of its own; it sees an engine through engine_internal.hpp only (the scan of the counts is the engine's,
// eng_scan_u32) and keeps its state in the engine's opaque slot (host_support.hpp: unit_state; simmr_engine_destroy deletes
// it, and its members free what they own).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "truth_host.hpp"

using namespace simmr;

namespace {

struct TruthState {
  // counts, their scan, an error word of its own (a plan of the next shard may own the engine's)
  DevBuf nm, off, err;
  Spans<2> sp;  // plan, emit
  // the plan: what it counted, the columns and the layout it was made for, the staging it counted against
  bool ready = false;
  uint64_t reads = 0, edits = 0, epoch = 0;
  const void *seq = nullptr, *seq_off = nullptr;
  uint32_t slot = 0;

  // a plan is in force until the next simmr_stage_* call (or a call that rewrites staged bases)
  bool in_force(const simmr_engine* e) const { return ready && epoch == eng_staging_epoch(e); }
};

constexpr auto truth_state = unit_state<TruthState, ENG_EXT_TRUTH>;

}  // namespace

extern "C" {

int simmr_truth_plan(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads, uint64_t* n_edits) {
  if (!e) return SIMMR_EINVAL;
  TruthState* s = truth_state(e, true);
  s->ready = false;
  s->sp.invalidate_from(0);
  if (!reads || !n_edits) return eng_fail(e, SIMMR_EINVAL, "simmr_truth_plan: NULL argument");
  int rc;
  if ((rc = check_read_columns(e, reads, n_reads, "simmr_truth_plan"))) return rc;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = s->sp.create_missing(e)) return rc;
  if (!s->nm.ensure_slack(std::max<uint64_t>(n_reads, 1) * 4) || !s->err.ensure_slack(64))
    return eng_fail(e, SIMMR_ENOMEM, "truth count allocation failed");
  hipStream_t st = eng_stream(e);
  uint32_t n_genomes = 0;
  const GenomeDev* genomes = eng_genome_table(e, &n_genomes);
  HIP_TRY(e, hipMemsetAsync(s->err.p, 0, 64, st));
  HIP_TRY(e, s->sp.begin(0, st));
  if (n_reads > 0)
    hipLaunchKernelGGL(k_truth<false>, dim3(row_grid(e, n_reads, TRUTH_WGS_PER_CU)), dim3(256), 0, st, genomes, n_genomes, truth_reads(reads),
                       n_reads, s->nm.as<uint32_t>(), (const uint64_t*)nullptr, TruthCols{nullptr, nullptr, nullptr, nullptr},
                       s->err.as<uint32_t>());
  uint64_t total = 0;
  if (!s->off.ensure_slack((n_reads + 1) * 8)) return eng_fail(e, SIMMR_ENOMEM, "offset allocation failed");
  if ((rc = eng_scan_u32(e, s->nm.as<const uint32_t>(), n_reads, s->off.as<uint64_t>(), &total))) return rc;
  HIP_TRY(e, s->sp.end(0, st));
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(&errw, s->err.p, 4, hipMemcpyDeviceToHost, st));
  if ((rc = sync_check(e, "truth count readback"))) return rc;
  if (errw & SIMMR_ERRBIT_TRUTH)
    return eng_fail(e, SIMMR_EINVAL, "a read names a genome or contig that is not staged, or its coordinates leave the contig or seq[]");
  s->reads = n_reads;
  s->edits = total;
  s->seq = reads->seq;
  s->seq_off = reads->seq_off;
  s->slot = reads->slot_bytes == SIMMR_SLOT16 ? 1u : 0u;
  s->epoch = eng_staging_epoch(e);
  s->ready = true;
  s->sp.mark(0);
  *n_edits = total;
  return SIMMR_OK;
}

int simmr_truth_emit(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* out) {
  if (!e) return SIMMR_EINVAL;
  TruthState* s = truth_state(e, false);
  if (s) s->sp.invalidate_from(1);  // (simmr_last_truth_ms: an emit that fails adds nothing to the plan's time)
  if (!reads || !out) return eng_fail(e, SIMMR_EINVAL, "simmr_truth_emit: NULL argument");
  if (!s || !s->in_force(e) || reads->seq != s->seq || reads->seq_off != s->seq_off ||
      (reads->slot_bytes == SIMMR_SLOT16 ? 1u : 0u) != s->slot)
    return eng_fail(e, SIMMR_ESTATE, "simmr_truth_emit called without a simmr_truth_plan for these columns");
  // (seq and seq_off are the plan's, which checked them; so is the layout)
  if (int rc = check_read_columns(e, reads, s->reads, "simmr_truth_emit", false)) return rc;
  const bool any_edit = out->edit_pos || out->edit_ref || out->edit_alt || out->edit_qual;
  if (any_edit && !out->edit_off) return eng_fail(e, SIMMR_EINVAL, "edit columns without edit_off");
  if ((out->nm || out->edit_off) && out->reads_capacity < s->reads)
    return eng_fail(e, SIMMR_ERANGE, "reads_capacity %llu < %llu reads planned", (unsigned long long)out->reads_capacity,
                    (unsigned long long)s->reads);
  if (any_edit && out->edits_capacity < s->edits)
    return eng_fail(e, SIMMR_ERANGE, "edits_capacity %llu < %llu edits planned", (unsigned long long)out->edits_capacity,
                    (unsigned long long)s->edits);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  uint32_t n_genomes = 0;
  const GenomeDev* genomes = eng_genome_table(e, &n_genomes);
  HIP_TRY(e, s->sp.begin(1, st));
  if (out->nm && s->reads > 0) HIP_TRY(e, hipMemcpyAsync(out->nm, s->nm.p, s->reads * 4, hipMemcpyDeviceToDevice, st));
  if (out->edit_off) HIP_TRY(e, hipMemcpyAsync(out->edit_off, s->off.p, (s->reads + 1) * 8, hipMemcpyDeviceToDevice, st));
  if (any_edit && s->edits > 0)
    hipLaunchKernelGGL(k_truth<true>, dim3(row_grid(e, s->reads, TRUTH_WGS_PER_CU)), dim3(256), 0, st, genomes, n_genomes, truth_reads(reads),
                       s->reads, (uint32_t*)nullptr, (const uint64_t*)s->off.as<uint64_t>(),
                       TruthCols{out->edit_pos, out->edit_ref, out->edit_alt, out->edit_qual}, s->err.as<uint32_t>());
  HIP_TRY(e, s->sp.end(1, st));
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "truth launch failed: %s", hipGetErrorString(rc));
  s->sp.mark(1);
  return SIMMR_OK;
}

int simmr_last_truth_ms(simmr_engine* e, float* ms) {
  if (!e || !ms) return SIMMR_EINVAL;
  TruthState* s = truth_state(e, false);
  if (!s || !s->in_force(e)) return eng_fail(e, SIMMR_ESTATE, "no truth plan yet");
  return s->sp.total_ms(e, "truth", ms);
}

}  // extern "C"
