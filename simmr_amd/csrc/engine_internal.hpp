// engine_internal.hpp — what another translation unit of libsimmr_hip.so (truth.hip, stats.hip, depth.hip, strain.hip, regions.hip,
// pileup.hip, sam.hip, sam_sort.hip, overlap.hip, fit.hip, fit_sam.hip, bam.hip, bam_index.hip, mapeval.hip, ovleval.hip, vcfeval.hip) may
// ask of an engine.
// simmr_engine is defined in engine.hip alone; these accessors are defined there and hidden, so the library exports nothing but the
// C ABI.  The host plumbing over these accessors that every unit uses, engine.hip too (the owning DevBuf and Events, the Spans that
// time a unit's calls, HIP_TRY, sync_check, unit_state, staged_rows), is host_support.hpp, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#include "device_types.hpp"

namespace simmr {

#define SIMMR_HIDDEN __attribute__((visibility("hidden")))

SIMMR_HIDDEN int eng_device(const simmr_engine* e);
SIMMR_HIDDEN hipStream_t eng_stream(const simmr_engine* e);
SIMMR_HIDDEN int eng_cu_count(const simmr_engine* e);
// the genome slots and the contigs staged in them (host copies of what the device table holds)
SIMMR_HIDDEN uint32_t eng_genome_slots(const simmr_engine* e);
SIMMR_HIDDEN uint32_t eng_contig_count(const simmr_engine* e, uint32_t slot);  // 0: the slot is not staged
SIMMR_HIDDEN uint64_t eng_contig_len(const simmr_engine* e, uint32_t slot, uint32_t contig);
// counts the simmr_stage_* calls: a state that records a layout of the staged genomes keeps the value it saw
SIMMR_HIDDEN uint64_t eng_staging_epoch(const simmr_engine* e);
// simmr_engine::fail: stores the message for simmr_last_error and returns `code`
SIMMR_HIDDEN int eng_fail(simmr_engine* e, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
// The planes of a staged slot (the caller has seen eng_contig_count(e, slot) > 0): the 2-bit plane and the exception plane
// from their word 0 (*mask = nullptr for a genome of pure ACGT), the device copy of the contig table, the plane's bases.
SIMMR_HIDDEN void eng_genome_planes(const simmr_engine* e, uint32_t slot, uint32_t** packed, const uint32_t** mask,
                                    const ContigDev** contigs_device, uint64_t* plane_bases);
// The device table of the genome slots (GenomeDev[*n_slots], what the read walker of read_walk.hpp takes); rewritten by every
// simmr_stage_* call on the engine's stream, so a kernel enqueued there sees the table of its own moment.
SIMMR_HIDDEN const GenomeDev* eng_genome_table(const simmr_engine* e, uint32_t* n_slots);
// What a call that rewrites staged bases owes the engine: what every simmr_stage_* call does (the staging epoch counts on:
// a truth plan, like every state that kept the epoch it saw, is no longer in force), and the plan in force is dropped with the
// direct FASTQ plan made from it.
SIMMR_HIDDEN void eng_planes_rewritten(simmr_engine* e);
// The stable radix sort of sam_sort_kernels.hip (defined in sam_sort.hip, whose kernels cannot be included into a second unit):
// sorts the n pairs (key[0][i], i) over the low key_bits bits of the keys on `st`, in 8-bit digits, least significant first.
// key[0] / key[1] and idx[0] / idx[1] are the ping and the pong (n entries each), hist holds SAMSORT_PAIRS_DIGITS words per tile of
// SAMSORT_PAIRS_TILE pairs, digit_total SAMSORT_PAIRS_DIGITS words.  Returns the side that holds the sorted pairs; with key_bits == 0
// nothing is launched, the answer is 0 and no index buffer is written (the order is the identity).  Only enqueues.
constexpr uint64_t SAMSORT_PAIRS_TILE = 2048, SAMSORT_PAIRS_DIGITS = 256;
SIMMR_HIDDEN int samsort_sort_pairs(hipStream_t st, uint64_t* const key[2], uint32_t* const idx[2], uint32_t* hist, uint32_t* digit_total,
                                    uint64_t n, uint32_t key_bits);
// The engine's scan (defined in engine.hip, whose k_scan_* kernels cannot be included into a second unit): the exclusive prefix
// sums of in[0 .. n) into out[0 .. n] (device pointers; the caller made room for the n + 1 entries) on the engine's stream, over the
// engine's scan scratch; *total = out[n].  Synchronises the stream.  n == 0: out[0] = 0, total 0, nothing launched.
SIMMR_HIDDEN int eng_scan_u32(simmr_engine* e, const uint32_t* in, uint64_t n, uint64_t* out, uint64_t* total);
// One opaque slot per engine and translation unit for that unit's state; simmr_engine_destroy calls `destroy` on a non-null
// slot (on the engine's device, after the device has been synchronised).  Units reach their slot through unit_state of
// host_support.hpp, whose hook deletes the state.
enum EngExt { ENG_EXT_DEPTH = 0, ENG_EXT_STRAIN = 1, ENG_EXT_REGIONS = 2, ENG_EXT_PILEUP = 3, ENG_EXT_SAM = 4, ENG_EXT_SAM_SORT = 5, ENG_EXT_OVERLAP = 6, ENG_EXT_FIT = 7, ENG_EXT_FIT_SAM = 8, ENG_EXT_BAM = 9, ENG_EXT_TRUTH = 10, ENG_EXT_STATS = 11, ENG_EXT_COUNT = 12 };
SIMMR_HIDDEN void** eng_ext_slot(simmr_engine* e, EngExt which, void (*destroy)(void*));
// The layout of depth[] that the last simmr_depth_reset recorded (defined in depth.hip): tracked contig k is entries
// cfirst[k] .. cfirst[k + 1] - 1 (n_contigs + 1 entries, on the host and on the device) and contig c_contig[k] of genome slot
// c_genome[k].  epoch: the staging epoch the reset saw; resets: counts the resets of this engine.  The host pointers hold
// until the next reset.  false: no reset yet.
struct DepthLayout {
  const uint64_t* cfirst;
  const uint64_t* cfirst_device;
  const uint32_t* c_genome;
  const uint32_t* c_contig;
  uint64_t n_contigs, n_positions, epoch, resets;
};
SIMMR_HIDDEN bool depth_layout(simmr_engine* e, DepthLayout* out);

}  // namespace simmr
