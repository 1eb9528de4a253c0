// fit_sam.hip — the model fit's SAM route (include/simmr_hip.h: simmr_fit_add_sam, simmr_fit_sam_counts_read): the entry
// points over fit_sam_kernels.hip.  A translation unit of its own beside fit.hip: it adds into fit.hip's tables, which it gets
// through fit_share (fit_device.hpp), and keeps only its side buffers in an engine slot of its own (ENG_EXT_FIT_SAM), grown on
// demand and freed with the state (host_support.hpp).
//
// add:  enqueue-only, so nothing is sized from what the text holds.  The buffers are sized from n_bytes alone: a line start per
//       two bytes (empty lines never enter the index), a descriptor per FSAM_MIN_TAKEN bytes (no shorter line is a taken
//       alignment), a row byte and a side byte per byte of text (an alignment has fewer columns than its line has bytes).
//       index (count) -> scan -> index (write) -> record -> md -> expand -> windows, between fit.hip's two events.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fit_sam_kernels.hip"
#include "host_support.hpp"

using namespace simmr;

namespace {

struct FitSamState {
  DevBuf tile_sum, tile_prefix, starts, recs, rows, side, cursor;
};

// a side buffer that has to grow takes a quarter more than it is asked for (the free waits for the work enqueued on it)
bool side_room(DevBuf& b, size_t bytes) { return b.ensure(bytes, bytes + bytes / 4); }

}  // namespace

extern "C" {

int simmr_fit_add_sam(simmr_engine* e, const uint8_t* text, uint64_t n_bytes, uint32_t n_sets) {
  if (!e) return SIMMR_EINVAL;
  if (n_sets != 1u && n_sets != 2u) return eng_fail(e, SIMMR_EINVAL, "simmr_fit_add_sam: n_sets is 1 or 2");
  if (!text && n_bytes > 0) return eng_fail(e, SIMMR_EINVAL, "simmr_fit_add_sam: NULL text");
  if (n_bytes > SIMMR_FIT_SAM_MAX_BYTES)
    return eng_fail(e, SIMMR_ENOTSUP, "simmr_fit_add_sam: %llu bytes in one add (at most %llu: cut the text at a line's end)",
                    (unsigned long long)n_bytes, (unsigned long long)SIMMR_FIT_SAM_MAX_BYTES);
  FitShare sh;
  if (!fit_share(e, &sh)) return eng_fail(e, SIMMR_ESTATE, "simmr_fit_add_sam called before simmr_fit_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  FitSamState* s = unit_state<FitSamState, ENG_EXT_FIT_SAM>(e, true);
  hipStream_t st = eng_stream(e);
  const uint64_t n_tiles = (n_bytes + FSAM_TILE - 1) / FSAM_TILE, start_cap = n_bytes / 2 + 1, rec_cap = n_bytes / FSAM_MIN_TAKEN + 1;
  if (n_bytes > 0 &&
      (!side_room(s->tile_sum, n_tiles * 8) || !side_room(s->tile_prefix, (n_tiles + 1) * 8) || !side_room(s->starts, start_cap * 4) ||
       !side_room(s->recs, rec_cap * sizeof(FsamRec)) || !side_room(s->rows, n_bytes + 16) || !side_room(s->side, n_bytes) || !side_room(s->cursor, 16)))
    return eng_fail(e, SIMMR_ENOMEM, "fit SAM side buffers: allocation failed for %llu bytes of text", (unsigned long long)n_bytes);
  HIP_TRY(e, hipEventRecord(sh.ev[0], st));
  if (n_bytes > 0) {
    const uint32_t cus = (uint32_t)std::max(eng_cu_count(e), 1);
    const uint32_t tile_grid = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)cus * 16u);
    const uint32_t rec_grid = (uint32_t)std::min<uint64_t>(n_bytes / (FSAM_WG_RECS * FSAM_MIN_TAKEN) + 1, (uint64_t)cus * 8u);
    HIP_TRY(e, hipMemsetAsync(s->cursor.p, 0, 16, st));
    HIP_TRY(e, hipMemsetAsync(s->side.p, 0, n_bytes, st));
    hipLaunchKernelGGL(k_fsam_index, dim3(tile_grid), dim3(FSAM_WG), 0, st, text, n_bytes, n_tiles, s->tile_sum.as<uint64_t>(),
                       (const uint64_t*)nullptr, (uint32_t*)nullptr, 0ull);
    hipLaunchKernelGGL(k_fsam_scan, dim3(1), dim3(256), 0, st, s->tile_sum.as<const uint64_t>(), s->tile_prefix.as<uint64_t>(), n_tiles);
    hipLaunchKernelGGL(k_fsam_index, dim3(tile_grid), dim3(FSAM_WG), 0, st, text, n_bytes, n_tiles, s->tile_sum.as<uint64_t>(),
                       s->tile_prefix.as<const uint64_t>(), s->starts.as<uint32_t>(), start_cap);
    const FsamWork W{text, n_bytes, s->tile_prefix.as<const uint64_t>() + n_tiles, s->starts.as<const uint32_t>(), s->recs.as<FsamRec>(), rec_cap,
                     s->rows.as<uint8_t>(), s->side.as<uint8_t>(), n_bytes, s->cursor.as<unsigned long long>()};
    hipLaunchKernelGGL(k_fsam_record, dim3(rec_grid), dim3(FSAM_WG), 0, st, W, n_sets, sh.T, sh.counts);
    hipLaunchKernelGGL(k_fsam_md, dim3(rec_grid), dim3(FSAM_WG), 0, st, W);
    hipLaunchKernelGGL(k_fsam_expand, dim3(rec_grid), dim3(FSAM_WG), 0, st, W);
    // the windows kernel keeps 64 KB of LDS: two workgroups a CU
    hipLaunchKernelGGL(k_fsam_windows, dim3(std::min(rec_grid, cus * 2u)), dim3(FSAM_WG), 0, st, W, sh.T);
  }
  HIP_TRY(e, hipEventRecord(sh.ev[1], st));
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "fit SAM launch failed: %s", hipGetErrorString(rc));
  fit_share_added(e);
  return SIMMR_OK;
}

int simmr_fit_sam_counts_read(simmr_engine* e, simmr_fit_sam_counts* out) {
  if (!e) return SIMMR_EINVAL;
  if (!out) return eng_fail(e, SIMMR_EINVAL, "simmr_fit_sam_counts_read: NULL argument");
  FitShare sh;
  if (!fit_share(e, &sh)) return eng_fail(e, SIMMR_ESTATE, "simmr_fit_sam_counts_read called before simmr_fit_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemcpyAsync(out, sh.counts, sizeof(*out), hipMemcpyDeviceToHost, st));
  return sync_check(e, "fit SAM counts");
}

}  // extern "C"
