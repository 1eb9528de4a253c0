// regions.hip — the gold-standard assembly (include/simmr_hip.h: simmr_regions_*): the entry points over
// regions_kernels.hip.  The fourth translation unit of libsimmr_hip.so; it sees an engine through engine_internal.hpp only,
// the layout of depth[] through depth.hip's accessor, and keeps its state in the engine's opaque slot (host_support.hpp:
// unit_state; simmr_engine_destroy deletes it, and its members free what they own).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "regions_kernels.hip"
#include "host_support.hpp"

using namespace simmr;

namespace {

struct RegionsState {
  // the plan in force: made for which layout of depth[] (staging epoch and reset), with which thresholds
  bool planned = false;
  uint64_t epoch = 0, resets = 0, min_len = 0;
  uint32_t min_depth = 0, n_contigs = 0;
  uint64_t n_positions = 0, n_runs = 0, n_regions = 0, n_bases = 0;
  // per tile of positions / per workgroup of runs: two arrays of counts and their prefixes, padded to whole scan iterations
  DevBuf tile_count, tile_prefix, run_count, run_prefix;
  DevBuf run_start, run_end;  // sized from the counted runs
  DevBuf r_x, r_c, r_off;     // the region table, sized from the counted regions
  DevBuf table;               // RegionContig per tracked contig
  Spans<2> sp;                // plan, emit
};

constexpr auto regions_state = unit_state<RegionsState, ENG_EXT_REGIONS>;

uint64_t pad_tops(uint64_t n) { return std::max<uint64_t>((n + REGIONS_TOPS_WIDTH - 1) / REGIONS_TOPS_WIDTH, 1) * REGIONS_TOPS_WIDTH; }

// the layout in force, or the refusal: the epoch check of simmr_depth_add
int layout_of(simmr_engine* e, const char* who, DepthLayout* L) {
  if (!depth_layout(e, L)) return eng_fail(e, SIMMR_ESTATE, "%s called before simmr_depth_reset", who);
  if (L->epoch != eng_staging_epoch(e))
    return eng_fail(e, SIMMR_ESTATE, "a genome was staged since simmr_depth_reset: the layout of depth[] is the reset's");
  return SIMMR_OK;
}

}  // namespace

extern "C" {

int simmr_regions_plan(simmr_engine* e, const uint32_t* depth_device, uint32_t min_depth, uint64_t min_len, uint64_t* n_regions,
                       uint64_t* n_bases) {
  if (!e) return SIMMR_EINVAL;
  if (!n_regions || !n_bases) return eng_fail(e, SIMMR_EINVAL, "simmr_regions_plan: NULL argument");
  RegionsState* s = regions_state(e, true);
  s->planned = false;
  DepthLayout L{};
  if (int rc = layout_of(e, "simmr_regions_plan", &L)) return rc;
  if (min_depth == 0 || min_len == 0) return eng_fail(e, SIMMR_EINVAL, "simmr_regions_plan: min_depth and min_len are at least 1");
  if (L.n_positions > 0 && (!depth_device || ((uintptr_t)depth_device & 15u)))
    return eng_fail(e, SIMMR_EINVAL, "simmr_regions_plan: depth_device must be a 16-byte aligned device pointer");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = s->sp.create_missing(e)) return rc;
  hipStream_t st = eng_stream(e);
  const uint64_t n = L.n_positions, n_contigs = L.n_contigs;
  // the tracked contigs as the kernels see them (the slots are staged: the reset tracked them and nothing was staged since)
  std::vector<RegionContig> table(std::max<uint64_t>(n_contigs, 1));
  for (uint64_t k = 0; k < n_contigs; k++) {
    uint32_t* packed = nullptr;
    const uint32_t* mask = nullptr;
    const ContigDev* contigs = nullptr;
    uint64_t bases = 0;
    eng_genome_planes(e, L.c_genome[k], &packed, &mask, &contigs, &bases);
    table[k] = RegionContig{packed, mask, contigs + L.c_contig[k], L.cfirst[k], L.c_genome[k], L.c_contig[k]};
  }
  const uint64_t n_tiles = (n + 1 + REGIONS_TILE - 1) / REGIONS_TILE;  // (one position more: a run that reaches the end ends there)
  if (n_tiles >= (1ull << 31)) return eng_fail(e, SIMMR_ENOTSUP, "simmr_regions_plan: too many tiles for one launch");
  const uint64_t tops = pad_tops(n_tiles);
  if (!s->table.ensure(table.size() * sizeof(RegionContig)) || !s->tile_count.ensure(2 * tops * 8) || !s->tile_prefix.ensure(2 * (tops + 1) * 8))
    return eng_fail(e, SIMMR_ENOMEM, "region tile allocation failed (%llu tiles)", (unsigned long long)n_tiles);
  HIP_TRY(e, hipMemcpyAsync(s->table.p, table.data(), table.size() * sizeof(RegionContig), hipMemcpyHostToDevice, st));
  HIP_TRY(e, hipMemsetAsync(s->tile_count.p, 0, 2 * tops * 8, st));
  HIP_TRY(e, s->sp.begin(0, st));
  if (n > 0)
    hipLaunchKernelGGL(k_regions_count, dim3((uint32_t)n_tiles), dim3(REGIONS_WG), 0, st, depth_device, n, min_depth, L.cfirst_device,
                       (uint32_t)n_contigs, s->tile_count.as<uint64_t>(), tops);
  hipLaunchKernelGGL(k_regions_scan, dim3(2), dim3(REGIONS_WG), 0, st, s->tile_count.as<const uint64_t>(), s->tile_prefix.as<uint64_t>(),
                     n_tiles, tops);
  uint64_t totals[2] = {0, 0};  // starts, ends: equal
  HIP_TRY(e, hipMemcpyAsync(&totals[0], s->tile_prefix.as<uint64_t>() + tops, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&totals[1], s->tile_prefix.as<uint64_t>() + 2 * tops + 1, 8, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "region count")) return rc;  // (the table was copied from a vector that goes with this call)
  if (totals[0] != totals[1]) return eng_fail(e, SIMMR_ENODEV, "simmr_regions_plan: run starts and ends differ in number");
  const uint64_t n_runs = totals[0];
  // the run buffers, from the counted runs
  const uint64_t run_tiles = (n_runs + REGIONS_RUN_TILE - 1) / REGIONS_RUN_TILE, rtops = pad_tops(run_tiles);
  if (run_tiles >= (1ull << 31)) return eng_fail(e, SIMMR_ENOTSUP, "simmr_regions_plan: too many runs for one launch");
  if (!s->run_start.ensure(std::max<uint64_t>(n_runs, 1) * 8) || !s->run_end.ensure(std::max<uint64_t>(n_runs, 1) * 8) ||
      !s->run_count.ensure(2 * rtops * 8) || !s->run_prefix.ensure(2 * (rtops + 1) * 8))
    return eng_fail(e, SIMMR_ENOMEM, "run buffer allocation failed (%llu runs)", (unsigned long long)n_runs);
  HIP_TRY(e, hipMemsetAsync(s->run_count.p, 0, 2 * rtops * 8, st));
  if (n_runs > 0) {
    hipLaunchKernelGGL(k_regions_runs, dim3((uint32_t)n_tiles), dim3(REGIONS_WG), 0, st, depth_device, n, min_depth, L.cfirst_device,
                       (uint32_t)n_contigs, s->tile_prefix.as<const uint64_t>(), tops, n_runs, s->run_start.as<uint64_t>(),
                       s->run_end.as<uint64_t>());
    hipLaunchKernelGGL(k_regions_flag, dim3((uint32_t)run_tiles), dim3(REGIONS_WG), 0, st, s->run_start.as<const uint64_t>(),
                       s->run_end.as<const uint64_t>(), n_runs, min_len, s->run_count.as<uint64_t>(), rtops);
  }
  hipLaunchKernelGGL(k_regions_scan, dim3(2), dim3(REGIONS_WG), 0, st, s->run_count.as<const uint64_t>(), s->run_prefix.as<uint64_t>(),
                     run_tiles, rtops);
  HIP_TRY(e, hipMemcpyAsync(&totals[0], s->run_prefix.as<uint64_t>() + rtops, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&totals[1], s->run_prefix.as<uint64_t>() + 2 * rtops + 1, 8, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "region scan")) return rc;
  const uint64_t nr = totals[0], nb = totals[1];
  // the region table, from the counted regions
  if (!s->r_x.ensure(std::max<uint64_t>(nr, 1) * 8) || !s->r_c.ensure(std::max<uint64_t>(nr, 1) * 4) || !s->r_off.ensure((nr + 1) * 8))
    return eng_fail(e, SIMMR_ENOMEM, "region table allocation failed (%llu regions)", (unsigned long long)nr);
  if (nr > 0)
    hipLaunchKernelGGL(k_regions_compact, dim3((uint32_t)run_tiles), dim3(REGIONS_WG), 0, st, s->run_start.as<const uint64_t>(),
                       s->run_end.as<const uint64_t>(), n_runs, min_len, s->run_prefix.as<const uint64_t>(), rtops, L.cfirst_device,
                       (uint32_t)n_contigs, nr, nb, s->r_x.as<uint64_t>(), s->r_c.as<uint32_t>(), s->r_off.as<uint64_t>());
  else
    HIP_TRY(e, hipMemsetAsync(s->r_off.p, 0, 8, st));
  HIP_TRY(e, s->sp.end(0, st));
  if (int rc = sync_check(e, "region table")) return rc;
  s->epoch = L.epoch;
  s->resets = L.resets;
  s->min_depth = min_depth;
  s->min_len = min_len;
  s->n_contigs = (uint32_t)n_contigs;
  s->n_positions = n;
  s->n_runs = n_runs;
  s->n_regions = *n_regions = nr;
  s->n_bases = *n_bases = nb;
  s->planned = true;
  s->sp.mark(0);
  s->sp.invalidate_from(1);
  return SIMMR_OK;
}

int simmr_regions_emit(simmr_engine* e, const uint32_t* depth_device, const simmr_regions_out* out) {
  if (!e) return SIMMR_EINVAL;
  if (!out) return eng_fail(e, SIMMR_EINVAL, "simmr_regions_emit: NULL argument");
  RegionsState* s = regions_state(e, false);
  DepthLayout L{};
  if (!s || !s->planned || !depth_layout(e, &L) || L.epoch != eng_staging_epoch(e) || s->epoch != L.epoch || s->resets != L.resets) {
    if (s) s->planned = false;
    return eng_fail(e, SIMMR_ESTATE, "simmr_regions_emit called without a simmr_regions_plan for the staged genomes and the last simmr_depth_reset");
  }
  const bool columns = out->genome || out->contig || out->start || out->len || out->depth_sum || out->seq_off;
  if (columns && out->capacity < s->n_regions)
    return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu regions", (unsigned long long)out->capacity, (unsigned long long)s->n_regions);
  if (out->seq && out->seq_capacity < s->n_bases)
    return eng_fail(e, SIMMR_ERANGE, "seq_capacity %llu < %llu bases", (unsigned long long)out->seq_capacity, (unsigned long long)s->n_bases);
  if (out->seq && ((uintptr_t)out->seq & 15u)) return eng_fail(e, SIMMR_EINVAL, "simmr_regions_emit: seq must be 16-byte aligned");
  if (out->depth_sum && s->n_positions > 0 && (!depth_device || ((uintptr_t)depth_device & 3u)))
    return eng_fail(e, SIMMR_EINVAL, "simmr_regions_emit: depth_sum needs the depth array");
  const uint64_t chunks = (s->n_bases + REGIONS_CHUNK - 1) / REGIONS_CHUNK, grid = (chunks + REGIONS_WG - 1) / REGIONS_WG;
  if (grid >= (1ull << 31) || s->n_regions / REGIONS_WG + 1 >= (1ull << 31))
    return eng_fail(e, SIMMR_ENOTSUP, "simmr_regions_emit: too many bases for one launch");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (out->depth_sum && s->n_regions > 0) HIP_TRY(e, hipMemsetAsync(out->depth_sum, 0, s->n_regions * 8, st));
  HIP_TRY(e, s->sp.begin(1, st));
  if (out->genome || out->contig || out->start || out->len || out->seq_off)
    hipLaunchKernelGGL(k_regions_columns, dim3((uint32_t)(s->n_regions / REGIONS_WG + 1)), dim3(REGIONS_WG), 0, st, s->r_x.as<const uint64_t>(),
                       s->r_c.as<const uint32_t>(), s->r_off.as<const uint64_t>(), s->table.as<const RegionContig>(), s->n_regions,
                       RegionCols{out->genome, out->contig, out->start, out->len, out->seq_off});
  if (s->n_bases > 0 && (out->seq || out->depth_sum))
    hipLaunchKernelGGL(k_regions_bases, dim3((uint32_t)grid), dim3(REGIONS_WG), 0, st, depth_device, s->r_x.as<const uint64_t>(),
                       s->r_c.as<const uint32_t>(), s->r_off.as<const uint64_t>(), s->table.as<const RegionContig>(), s->n_regions, s->n_bases,
                       out->seq, (unsigned long long*)out->depth_sum);
  HIP_TRY(e, s->sp.end(1, st));
  s->sp.mark(1);
  return sync_check(e, "region emit");
}

int simmr_last_regions_ms(simmr_engine* e, float* ms) {
  if (!e || !ms) return SIMMR_EINVAL;
  RegionsState* s = regions_state(e, false);
  if (!s || !s->sp.valid[0]) return eng_fail(e, SIMMR_ESTATE, "no simmr_regions_plan yet");
  return s->sp.total_ms(e, "regions", ms);
}

}  // extern "C"
