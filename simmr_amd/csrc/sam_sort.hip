// sam_sort.hip — the true alignments in coordinate order (include/simmr_hip.h: simmr_sam_sort_*): the entry points over
// sam_sort_kernels.hip.  The seventh translation unit of libsimmr_hip.so; like sam.hip it sees an engine through
// engine_internal.hpp only and keeps its state in a slot of its own (ENG_EXT_SAM_SORT), so a sorted plan and an unsorted one
// on one engine do not disturb each other.  The names table and the argument checks are sam.hip's (sam_names.hpp); the plan, the
// emit and the timer are the shared ones of record_stream_host.hpp, given this unit's traits (SamSortFormat).  The sort itself
// (samsort_sort_pairs) is defined here, for that plan, for bam_index.hip's and for overlap.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "sam_sort_kernels.hip"
#include "record_stream_host.hpp"
#include "scorer_host.hpp"

using namespace simmr;

namespace {

struct SamSortFormat : RecordFormat {
  static constexpr bool SORTED = true;
  static constexpr const char *PLAN = "simmr_sam_sort_plan", *EMIT = "simmr_sam_sort_emit", *NOUN = "sorted SAM", *TIMER = "sorted sam";
  static constexpr const char *SYNC_PLAN = "sorted SAM plan", *SYNC_SIZE = "sorted SAM size and sort passes", *SYNC_WRITE = "sorted SAM write pass";
  static constexpr const char* PLAN_REFUSAL =
      "a read's bytes leave seq[], it is longer than %u bases, its edit_off decreases or leaves edits_capacity, or its edit_pos do not ascend inside "
      "the read";
  static RecordStreamState* state(simmr_engine* e, bool create) { return unit_state<RecordStreamState, ENG_EXT_SAM_SORT>(e, create); }
  static void size(hipStream_t st, uint32_t grid, RecordStreamState& s, const SamReads& rd, const SamEdits& ed, uint64_t n, uint32_t paired, uint32_t pos_bits) {
    hipLaunchKernelGGL(k_samsort_size, dim3(grid), dim3(256), 0, st, rd, ed, s.nt.names(), s.nt.c_bases.as<const uint64_t>(), n, paired, pos_bits,
                       s.len.as<uint32_t>(), s.key[0].as<uint64_t>(), s.err_p());
  }
  static void gather(hipStream_t st, uint32_t grid, RecordStreamState& s, uint64_t n, uint32_t pos_bits, int cur) {
    hipLaunchKernelGGL(k_samsort_gather, dim3(grid), dim3(256), 0, st, s.len.as<const uint32_t>(), s.key[cur].as<const uint64_t>(), s.perm, n, pos_bits,
                       s.idx[cur ^ 1].as<uint32_t>(), s.key[cur ^ 1].as<uint64_t>(), s.chunk_sum.as<uint64_t>());
  }
  static void scan(hipStream_t st, RecordStreamState& s, uint64_t n_chunks) {
    hipLaunchKernelGGL(k_samsort_scan, dim3(1), dim3(256), 0, st, s.chunk_sum.as<const uint64_t>(), s.chunk_prefix.as<uint64_t>(), n_chunks);
  }
  static void offsets(hipStream_t st, uint32_t grid, RecordStreamState& s, const uint32_t* slen, uint64_t n) {
    hipLaunchKernelGGL(k_samsort_offsets, dim3(grid), dim3(256), 0, st, slen, s.chunk_prefix.as<const uint64_t>(), n, s.off.as<uint64_t>());
  }
  static void write(hipStream_t st, uint32_t grid, RecordStreamState& s, uint8_t* dst) {
    hipLaunchKernelGGL(k_samsort_write, dim3(grid), dim3(256), 0, st, s.reads, s.edits, s.nt.names(), s.n_reads, s.paired, s.perm,
                       s.off.as<const uint64_t>(), dst, s.err_p());
  }
};

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
  return record_plan<SamSortFormat>(e, names, reads, truth, n_reads, paired, total_bytes);
}

int simmr_sam_sort_emit(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* truth, uint8_t* dst, uint64_t dst_capacity,
                        uint64_t* key_out, uint64_t* line_off_out) {
  return record_emit<SamSortFormat>(e, reads, truth, dst, dst_capacity, key_out, line_off_out, nullptr);
}

int simmr_last_sam_sort_ms(simmr_engine* e, float* ms) { return record_ms<SamSortFormat>(e, ms); }

}  // extern "C"
