// depth.hip — coverage depth (include/simmr_hip.h: simmr_depth_*): the entry points over depth_kernels.hip.  The second
// translation unit of libsimmr_hip.so; it sees an engine through engine_internal.hpp only and keeps its state in the
// engine's opaque slot (host_support.hpp: unit_state; simmr_engine_destroy deletes it, and its members free what they own).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "depth_kernels.hip"
#include "host_support.hpp"

using namespace simmr;

namespace {

struct DepthState {
  // the layout recorded by the last reset: genome slots -> contigs -> first position (host copies and their device tables)
  std::vector<DepthSlot> slots;
  std::vector<uint64_t> cfirst;           // n_contigs + 1
  std::vector<uint32_t> c_genome, c_contig;
  std::vector<uint64_t> fwin;             // n_contigs + 1, of the last summarize
  uint64_t n_positions = 0, n_tiles = 0, epoch = 0, added = 0, resets = 0;
  bool ready = false;
  DevBuf diff, tile_sum, d_slots, d_cfirst, d_fwin, d_out;
  Spans<3> sp;                            // add, emit, summarize

  size_t diff_bytes() const { return (size_t)n_tiles * DEPTH_TILE * 4u; }  // n_positions + 1 entries, padded to whole tiles
  int32_t* diff_p() const { return diff.as<int32_t>(); }
  uint32_t* err_p() const { return (uint32_t*)(diff.as<char>() + diff_bytes()); }  // the sticky error word, behind the array
};

constexpr auto depth_state = unit_state<DepthState, ENG_EXT_DEPTH>;

}  // namespace

// engine_internal.hpp: what regions.hip reads of the layout
namespace simmr {
bool depth_layout(simmr_engine* e, DepthLayout* out) {
  DepthState* s = depth_state(e, false);
  if (!s || !s->ready) return false;
  *out = DepthLayout{s->cfirst.data(), (const uint64_t*)s->d_cfirst.p, s->c_genome.data(), s->c_contig.data(), s->c_genome.size(),
                     s->n_positions, s->epoch, s->resets};
  return true;
}
}  // namespace simmr

extern "C" {

int simmr_depth_reset(simmr_engine* e, uint64_t* n_positions, uint64_t* n_contigs) {
  if (!e) return SIMMR_EINVAL;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  DepthState* s = depth_state(e, true);
  s->ready = false;
  if (int rc = s->sp.create_missing(e)) return rc;
  StagedRows rows = staged_rows(e, true);
  const uint32_t n_slots = rows.n_slots();
  s->slots.assign(n_slots, DepthSlot{0u, 0u});
  for (uint32_t g = 0; g < n_slots; g++) s->slots[g] = DepthSlot{rows.cbase[g], rows.ncontig[g]};
  s->cfirst = std::move(rows.first);
  s->c_genome = std::move(rows.genome);
  s->c_contig = std::move(rows.contig);
  s->n_positions = s->cfirst.back();
  s->n_tiles = (s->n_positions + 1 + DEPTH_TILE - 1) / DEPTH_TILE;
  const uint64_t tops = (s->n_tiles + DEPTH_TOPS_WIDTH - 1) / DEPTH_TOPS_WIDTH * DEPTH_TOPS_WIDTH;
  if (!s->diff.ensure(s->diff_bytes() + 16) || !s->tile_sum.ensure(tops * 4) ||
      !s->d_slots.ensure(std::max<size_t>(n_slots, 1) * sizeof(DepthSlot)) ||
      !s->d_cfirst.ensure(s->cfirst.size() * 8) || !s->d_fwin.ensure(s->cfirst.size() * 8) ||
      !s->d_out.ensure((3 * s->c_genome.size() + SIMMR_DEPTH_HIST_BINS) * 8))
    return eng_fail(e, SIMMR_ENOMEM, "depth array allocation failed (%llu positions)", (unsigned long long)s->n_positions);
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemsetAsync(s->diff.p, 0, s->diff_bytes() + 16, st));
  HIP_TRY(e, hipMemsetAsync(s->tile_sum.p, 0, tops * 4, st));
  if (n_slots) HIP_TRY(e, hipMemcpyAsync(s->d_slots.p, s->slots.data(), n_slots * sizeof(DepthSlot), hipMemcpyHostToDevice, st));
  HIP_TRY(e, hipMemcpyAsync(s->d_cfirst.p, s->cfirst.data(), s->cfirst.size() * 8, hipMemcpyHostToDevice, st));
  s->epoch = eng_staging_epoch(e);
  s->added = 0;
  s->sp.invalidate_from(0);
  if (int rc = sync_check(e, "depth reset")) return rc;  // (the tables were copied from vectors the next reset rewrites)
  s->ready = true;
  s->resets++;
  if (n_positions) *n_positions = s->n_positions;
  if (n_contigs) *n_contigs = s->c_genome.size();
  return SIMMR_OK;
}

int simmr_depth_add(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads) {
  if (!e) return SIMMR_EINVAL;
  if (!reads) return eng_fail(e, SIMMR_EINVAL, "simmr_depth_add: NULL argument");
  if (!reads->start || !reads->end || !reads->contig || !reads->genome)
    return eng_fail(e, SIMMR_EINVAL, "simmr_depth_add needs start, end, contig and genome");
  DepthState* s = depth_state(e, false);
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_depth_add called before simmr_depth_reset");
  if (s->epoch != eng_staging_epoch(e))
    return eng_fail(e, SIMMR_ESTATE, "a genome was staged since simmr_depth_reset: the layout of depth[] is the reset's");
  if (n_reads >= (1ull << 31) || s->added + n_reads >= (1ull << 31))
    return eng_fail(e, SIMMR_ERANGE, "the reads added since simmr_depth_reset would reach 2^31");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, s->sp.begin(0, st));
  if (n_reads > 0)
    hipLaunchKernelGGL(k_depth_mark, dim3((uint32_t)((n_reads + DEPTH_WG - 1) / DEPTH_WG)), dim3(DEPTH_WG), 0, st, reads->start, reads->end,
                       reads->contig, reads->genome, n_reads, (const DepthSlot*)s->d_slots.p, (uint32_t)s->slots.size(),
                       (const uint64_t*)s->d_cfirst.p, s->diff_p(), s->err_p());
  HIP_TRY(e, s->sp.end(0, st));
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "depth launch failed: %s", hipGetErrorString(rc));
  s->added += n_reads;
  s->sp.mark(0);
  s->sp.invalidate_from(1);
  return SIMMR_OK;
}

int simmr_depth_emit(simmr_engine* e, uint32_t* depth_device, uint64_t capacity) {
  if (!e) return SIMMR_EINVAL;
  DepthState* s = depth_state(e, false);
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_depth_emit called before simmr_depth_reset");
  if (capacity < s->n_positions)
    return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu positions", (unsigned long long)capacity, (unsigned long long)s->n_positions);
  if (s->n_positions > 0 && (!depth_device || ((uintptr_t)depth_device & 15u)))
    return eng_fail(e, SIMMR_EINVAL, "simmr_depth_emit: depth_device must be a 16-byte aligned device pointer");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, s->sp.begin(1, st));
  if (s->n_positions > 0) {
    const uint32_t grid = (uint32_t)s->n_tiles;
    hipLaunchKernelGGL(k_depth_tile_sums, dim3(grid), dim3(DEPTH_WG), 0, st, (const depth_v4i*)s->diff.p, (int32_t*)s->tile_sum.p);
    hipLaunchKernelGGL(k_depth_scan_tiles, dim3(1), dim3(DEPTH_WG), 0, st, (int32_t*)s->tile_sum.p, s->n_tiles);
    // (the tile that holds only the extra last slot has nothing to write)
    hipLaunchKernelGGL(k_depth_apply, dim3((uint32_t)((s->n_positions + DEPTH_TILE - 1) / DEPTH_TILE)), dim3(DEPTH_WG), 0, st,
                       (const depth_v4i*)s->diff.p, (const int32_t*)s->tile_sum.p, depth_device, s->n_positions);
  }
  HIP_TRY(e, s->sp.end(1, st));
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "depth scan")) return rc;
  if (s->sp.valid[0]) s->sp.mark(1);
  if (errw)
    return eng_fail(e, SIMMR_EINVAL, "a read added since the last simmr_depth_reset names a genome slot that is not tracked or a "
                                     "contig that does not exist, or its window leaves its contig");
  return SIMMR_OK;
}

int simmr_depth_contig_first(simmr_engine* e, uint32_t genome_idx, uint32_t contig, uint64_t* first) {
  if (!e) return SIMMR_EINVAL;
  if (!first) return eng_fail(e, SIMMR_EINVAL, "simmr_depth_contig_first: NULL argument");
  DepthState* s = depth_state(e, false);
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_depth_contig_first called before simmr_depth_reset");
  if (genome_idx >= s->slots.size() || contig >= s->slots[genome_idx].n_contigs)
    return eng_fail(e, SIMMR_EINVAL, "genome %u contig %u is not tracked", genome_idx, contig);
  *first = s->cfirst[s->slots[genome_idx].cbase + contig];
  return SIMMR_OK;
}

int simmr_depth_summarize(simmr_engine* e, const uint32_t* depth_device, uint32_t window, simmr_depth_contig* rows_host,
                          uint64_t rows_capacity, uint64_t* hist_host, simmr_depth_windows* win) {
  if (!e) return SIMMR_EINVAL;
  DepthState* s = depth_state(e, false);
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_depth_summarize called before simmr_depth_reset");
  if (window >= (1u << 30)) return eng_fail(e, SIMMR_EINVAL, "simmr_depth_summarize: window must be below 2^30");
  const uint64_t n_contigs = s->c_genome.size();
  const bool windows = window > 0 && win;
  const uint32_t unit = windows ? window : DEPTH_TILE;  // positions of a unit of work: a window, or a fixed chunk
  s->fwin.assign(n_contigs + 1, 0ull);
  for (uint64_t k = 0; k < n_contigs; k++) s->fwin[k + 1] = s->fwin[k] + (s->cfirst[k + 1] - s->cfirst[k] + unit - 1) / unit;
  const uint64_t n_units = s->fwin[n_contigs];
  if (windows) {
    win->n_windows = n_units;
    if (win->capacity < n_units)
      return eng_fail(e, SIMMR_ERANGE, "win->capacity %llu < %llu windows", (unsigned long long)win->capacity, (unsigned long long)n_units);
    if (n_units > 0 && (!win->sum || !win->covered || !win->max)) return eng_fail(e, SIMMR_EINVAL, "simmr_depth_summarize: NULL window column");
  }
  if (rows_host && rows_capacity < n_contigs)
    return eng_fail(e, SIMMR_ERANGE, "rows_capacity %llu < %llu contigs", (unsigned long long)rows_capacity, (unsigned long long)n_contigs);
  if (s->n_positions > 0 && !depth_device) return eng_fail(e, SIMMR_EINVAL, "simmr_depth_summarize: NULL depth array");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  // d_out: three words per contig (sum, covered, max), the histogram behind them
  std::vector<unsigned long long> host(3 * n_contigs + SIMMR_DEPTH_HIST_BINS, 0ull);
  void* const d_out = s->d_out.p;
  HIP_TRY(e, hipMemsetAsync(d_out, 0, host.size() * 8, st));
  HIP_TRY(e, hipMemcpyAsync(s->d_fwin.p, s->fwin.data(), s->fwin.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(e, s->sp.begin(2, st));
  if (n_units > 0) {
    // consecutive units per wave: enough waves to fill the device, and fewer than 2^30 positions per wave (unit < 2^30): an
    // LDS bin of the workgroup's four waves stays below 2^32
    const uint64_t waves = (uint64_t)eng_cu_count(e) * 32u;
    uint64_t per_wave = std::max<uint64_t>((n_units + waves - 1) / waves, 1);
    per_wave = std::max<uint64_t>(std::min<uint64_t>(per_wave, ((1ull << 30) - 1) / unit), 1);
    const uint64_t n_waves = (n_units + per_wave - 1) / per_wave;
    const uint64_t grid = (n_waves + DEPTH_WG / 64 - 1) / (DEPTH_WG / 64);
    if (grid >= (1ull << 31)) return eng_fail(e, SIMMR_ERANGE, "simmr_depth_summarize: too many windows for one launch");
    unsigned long long* rows = (unsigned long long*)d_out;
    hipLaunchKernelGGL(k_depth_summarize, dim3((uint32_t)grid), dim3(DEPTH_WG), 0, st, depth_device, (const uint64_t*)s->d_cfirst.p,
                       (const uint64_t*)s->d_fwin.p, (uint32_t)n_contigs, unit, n_units, per_wave,
                       windows ? (unsigned long long*)win->sum : nullptr, windows ? win->covered : nullptr, windows ? win->max : nullptr,
                       rows, rows + 3 * n_contigs);
  }
  HIP_TRY(e, s->sp.end(2, st));
  HIP_TRY(e, hipMemcpyAsync(host.data(), d_out, host.size() * 8, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "depth summary")) return rc;
  if (s->sp.valid[0]) s->sp.mark(2);
  for (uint64_t k = 0; rows_host && k < n_contigs; k++) {
    simmr_depth_contig& r = rows_host[k];
    memset(&r, 0, sizeof r);
    r.genome = s->c_genome[k];
    r.contig = s->c_contig[k];
    r.first = s->cfirst[k];
    r.len = s->cfirst[k + 1] - s->cfirst[k];
    r.depth_sum = host[3 * k];
    r.covered = host[3 * k + 1];
    r.depth_max = (uint32_t)host[3 * k + 2];
    r.first_window = windows ? s->fwin[k] : 0;
  }
  if (hist_host) memcpy(hist_host, host.data() + 3 * n_contigs, SIMMR_DEPTH_HIST_BINS * 8);
  return SIMMR_OK;
}

int simmr_last_depth_ms(simmr_engine* e, float* ms) {
  if (!e || !ms) return SIMMR_EINVAL;
  DepthState* s = depth_state(e, false);
  if (!s || !s->sp.valid[0]) return eng_fail(e, SIMMR_ESTATE, "no simmr_depth_add yet");
  return s->sp.total_ms(e, "depth", ms);
}

}  // extern "C"
