// sam.hip — the true alignments as SAM text (include/simmr_hip.h: simmr_sam_*): the entry points over sam_kernels.hip.
// The sixth translation unit of libsimmr_hip.so; it sees an engine through engine_internal.hpp only — the device, the
// stream, which slots are staged and the staging epoch: the pass reads the caller's columns, never the genome planes —
// and keeps its state in the engine's opaque slot (host_support.hpp: unit_state).  The plan, the
// emit and the timer are record_plan / record_emit / record_ms of record_stream_host.hpp, shared with sam_sort.hip, bam.hip and
// bam_index.hip: this unit gives them its state, its words and the launches of its four kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "sam_kernels.hip"
#include "record_stream_host.hpp"

using namespace simmr;

namespace {

struct SamFormat : RecordFormat {
  static constexpr const char *PLAN = "simmr_sam_plan", *EMIT = "simmr_sam_emit", *NOUN = "SAM", *TIMER = "sam";
  static constexpr const char *SYNC_PLAN = "SAM plan", *SYNC_SIZE = "SAM size pass", *SYNC_WRITE = "SAM write pass";
  static constexpr const char* PLAN_REFUSAL =
      "a read's genome / contig has no name, its bytes leave seq[], it is longer than %u bases, its edit_off decreases or leaves edits_capacity, or its "
      "edit_pos do not ascend inside the read";
  static RecordStreamState* state(simmr_engine* e, bool create) { return unit_state<RecordStreamState, ENG_EXT_SAM>(e, create); }
  static void size(hipStream_t st, uint32_t grid, RecordStreamState& s, const SamReads& rd, const SamEdits& ed, uint64_t n, uint32_t paired, uint32_t) {
    hipLaunchKernelGGL(k_sam_size, dim3(grid), dim3(256), 0, st, rd, ed, s.nt.names(), n, paired, s.len.as<uint32_t>(), s.chunk_sum.as<uint64_t>(), s.err_p());
  }
  static void scan(hipStream_t st, RecordStreamState& s, uint64_t n_chunks) {
    hipLaunchKernelGGL(k_sam_scan, dim3(1), dim3(256), 0, st, s.chunk_sum.as<const uint64_t>(), s.chunk_prefix.as<uint64_t>(), n_chunks);
  }
  static void offsets(hipStream_t st, uint32_t grid, RecordStreamState& s, const uint32_t* len, uint64_t n) {
    hipLaunchKernelGGL(k_sam_offsets, dim3(grid), dim3(256), 0, st, len, s.chunk_prefix.as<const uint64_t>(), n, s.off.as<uint64_t>());
  }
  static void write(hipStream_t st, uint32_t grid, RecordStreamState& s, uint8_t* dst) {
    hipLaunchKernelGGL(k_sam_write, dim3(grid), dim3(256), 0, st, s.reads, s.edits, s.nt.names(), s.n_reads, s.paired, s.off.as<const uint64_t>(), dst, s.err_p());
  }
};

}  // namespace

extern "C" {

int simmr_sam_plan(simmr_engine* e, const simmr_sam_names* names, const simmr_reads_out* reads, const simmr_truth_out* truth,
                   uint64_t n_reads, int paired, uint64_t* total_bytes) {
  return record_plan<SamFormat>(e, names, reads, truth, n_reads, paired, total_bytes);
}

int simmr_sam_emit(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* truth, uint8_t* dst, uint64_t dst_capacity) {
  return record_emit<SamFormat>(e, reads, truth, dst, dst_capacity, nullptr, nullptr, nullptr);
}

int simmr_last_sam_ms(simmr_engine* e, float* ms) { return record_ms<SamFormat>(e, ms); }

}  // extern "C"
