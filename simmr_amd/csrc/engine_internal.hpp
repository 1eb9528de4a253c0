// engine_internal.hpp — what another translation unit of libsimmr_hip.so (depth.hip) may ask of an engine.  simmr_engine is
// defined in engine.hip alone; these accessors are defined there and hidden, so the library exports nothing but the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"

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
// One opaque slot per engine for that translation unit's state; simmr_engine_destroy calls `destroy` on a non-null slot
// (on the engine's device, after the device has been synchronised).
SIMMR_HIDDEN void** eng_ext_slot(simmr_engine* e, void (*destroy)(void*));

}  // namespace simmr
