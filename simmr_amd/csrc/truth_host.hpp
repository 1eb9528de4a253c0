// truth_host.hpp — what the two units that walk the reads a row of 16 lanes at a time share on the host (truth.hip, and
// stats.hip, whose kernel batches its reads as k_truth does and says so with a static_assert): the kernels' view of the columns,
// their grid, and the check of the columns they read.  Internal to the library; k_truth is a template, so a unit that includes
// this file and launches none of it holds no truth kernel.
#pragma once
#include <algorithm>

#include "truth_kernels.hip"
#include "host_support.hpp"

namespace simmr {
namespace {

TruthReads truth_reads(const simmr_reads_out* reads) {
  return TruthReads{reads->seq, reads->qual, reads->seq_off, reads->start, reads->end, reads->contig, reads->genome,
                    reads->flags, reads->seq_capacity, reads->slot_bytes == SIMMR_SLOT16 ? 1u : 0u};
}
// the grid of the kernels that walk the reads, a row of 16 lanes per read and 16 reads per workgroup and batch
uint32_t row_grid(const simmr_engine* e, uint64_t n_reads, uint32_t wgs_per_cu) {
  const uint64_t n_batches = (n_reads + TRUTH_WG_READS - 1) / TRUTH_WG_READS;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_batches, (uint64_t)eng_cu_count(e) * wgs_per_cu));
}
// the columns those kernels read: all of them, seq and qual once there is a read (n_reads > 0), and, where the call
// takes the layout from `reads` (check_slot), a slot_bytes it knows
int check_read_columns(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads, const char* who, bool check_slot = true) {
  if (!reads->seq_off || !reads->start || !reads->end || !reads->contig || !reads->genome || !reads->flags ||
      (n_reads > 0 && (!reads->seq || !reads->qual)))
    return eng_fail(e, SIMMR_EINVAL, "%s needs seq, qual, seq_off, start, end, contig, genome and flags", who);
  if (check_slot && reads->slot_bytes > 1u && reads->slot_bytes != SIMMR_SLOT16) return eng_fail(e, SIMMR_EINVAL, "reads->slot_bytes is 0 (compact) or 16");
  return SIMMR_OK;
}

}  // namespace
}  // namespace simmr
