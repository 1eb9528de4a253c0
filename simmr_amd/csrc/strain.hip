// strain.hip — strain divergence (include/simmr_hip.h: simmr_strain_*): the entry points over strain_kernels.hip.  The third
// translation unit of libsimmr_hip.so; it sees an engine through engine_internal.hpp only and keeps its state in the
// engine's opaque slot (host_support.hpp: unit_state; simmr_engine_destroy deletes it, and its members free what they own).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "strain_kernels.hip"
#include "host_support.hpp"

using namespace simmr;

namespace {

struct StrainState {
  // the plan in force: which genome, at which staging epoch, with which draw
  bool planned = false;
  uint32_t genome = 0;
  uint64_t epoch = 0, n_sites = 0, n_tiles = 0;
  StrainDraw draw{};
  DevBuf tile_count, tile_prefix;  // u32 per tile; u64 per tile and the total, both padded to whole scan iterations
  Spans<2> sp;                     // plan, apply
};

constexpr auto strain_state = unit_state<StrainState, ENG_EXT_STRAIN>;

// what the kernels take of a staged slot
struct Planes {
  uint32_t* packed;
  const uint32_t* mask;
  const ContigDev* contigs;
  uint32_t n_contigs;
  uint64_t plane_words;
};
Planes planes_of(const simmr_engine* e, uint32_t slot) {
  Planes p{};
  uint64_t bases = 0;
  eng_genome_planes(e, slot, &p.packed, &p.mask, &p.contigs, &bases);
  p.n_contigs = eng_contig_count(e, slot);
  p.plane_words = bases / STRAIN_WORD_BASES;
  return p;
}

}  // namespace

extern "C" {

int simmr_strain_plan(simmr_engine* e, uint32_t genome_idx, double identity, uint64_t seed, uint64_t* n_sites) {
  if (!e) return SIMMR_EINVAL;
  if (!n_sites) return eng_fail(e, SIMMR_EINVAL, "simmr_strain_plan: NULL argument");
  if (!(identity >= 0.25 && identity <= 1.0)) return eng_fail(e, SIMMR_EINVAL, "simmr_strain_plan: identity must be in [0.25, 1]");
  const uint32_t n_contigs = eng_contig_count(e, genome_idx);
  if (n_contigs == 0) return eng_fail(e, SIMMR_EINVAL, "genome %u is not staged", genome_idx);
  for (uint32_t c = 0; c < n_contigs; c++)
    if (eng_contig_len(e, genome_idx, c) >= (1ull << 34))
      return eng_fail(e, SIMMR_ENOTSUP, "contig %u has 2^34 bases or more: its positions do not fit the draws' counter", c);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  StrainState* s = strain_state(e, true);
  s->planned = false;
  if (int rc = s->sp.create_missing(e)) return rc;
  // strain sites, version 1: the thresholds in integer arithmetic
  const uint64_t t32 = (uint64_t)((1.0 - identity) * 4294967296.0 + 0.5);  // at most 3 * 2^30
  s->draw = StrainDraw{(uint32_t)t32, (uint32_t)((t32 + 2) / 3), (uint32_t)((2 * t32 + 2) / 3), (uint32_t)seed, (uint32_t)(seed >> 32)};
  const Planes p = planes_of(e, genome_idx);
  s->n_tiles = (p.plane_words + STRAIN_WG - 1) / STRAIN_WG;
  if (s->n_tiles >= (1ull << 31)) return eng_fail(e, SIMMR_ENOTSUP, "simmr_strain_plan: too many tiles for one launch");
  const uint64_t tops = (s->n_tiles + STRAIN_TOPS_WIDTH - 1) / STRAIN_TOPS_WIDTH * STRAIN_TOPS_WIDTH;
  if (!s->tile_count.ensure(std::max<uint64_t>(tops, 1) * 4) || !s->tile_prefix.ensure((tops + 1) * 8))
    return eng_fail(e, SIMMR_ENOMEM, "strain tile allocation failed (%llu tiles)", (unsigned long long)s->n_tiles);
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemsetAsync(s->tile_count.p, 0, std::max<uint64_t>(tops, 1) * 4, st));
  HIP_TRY(e, s->sp.begin(0, st));
  if (s->n_tiles > 0)
    hipLaunchKernelGGL(k_strain_count, dim3((uint32_t)s->n_tiles), dim3(STRAIN_WG), 0, st, p.mask, p.contigs, p.n_contigs, p.plane_words,
                       s->draw, s->tile_count.as<uint32_t>());
  hipLaunchKernelGGL(k_strain_scan_tiles, dim3(1), dim3(STRAIN_WG), 0, st, s->tile_count.as<const uint32_t>(), s->tile_prefix.as<uint64_t>(),
                     s->n_tiles);
  HIP_TRY(e, s->sp.end(0, st));
  uint64_t total = 0;
  HIP_TRY(e, hipMemcpyAsync(&total, (const uint64_t*)s->tile_prefix.p + tops, 8, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "strain count")) return rc;
  s->genome = genome_idx;
  s->epoch = eng_staging_epoch(e);
  s->n_sites = *n_sites = total;
  s->planned = true;
  s->sp.mark(0);
  s->sp.invalidate_from(1);
  return SIMMR_OK;
}

int simmr_strain_apply(simmr_engine* e, uint32_t genome_idx, const simmr_strain_out* out) {
  if (!e) return SIMMR_EINVAL;
  if (eng_contig_count(e, genome_idx) == 0) return eng_fail(e, SIMMR_EINVAL, "genome %u is not staged", genome_idx);
  StrainState* s = strain_state(e, false);
  if (!s || !s->planned || s->genome != genome_idx)
    return eng_fail(e, SIMMR_ESTATE, "simmr_strain_apply called without a simmr_strain_plan for genome %u", genome_idx);
  if (s->epoch != eng_staging_epoch(e)) {
    s->planned = false;
    return eng_fail(e, SIMMR_ESTATE, "a genome was staged since simmr_strain_plan: the plan counted other planes");
  }
  const bool columns = out && (out->contig || out->pos || out->ref || out->alt);
  if (columns && out->capacity < s->n_sites)
    return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu sites", (unsigned long long)out->capacity, (unsigned long long)s->n_sites);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  const Planes p = planes_of(e, genome_idx);
  hipStream_t st = eng_stream(e);
  s->planned = false;  // consumed: the planes are about to change
  HIP_TRY(e, s->sp.begin(1, st));
  if (s->n_sites > 0)
    hipLaunchKernelGGL(k_strain_apply, dim3((uint32_t)s->n_tiles), dim3(STRAIN_WG), 0, st, p.packed, p.mask, p.contigs, p.n_contigs,
                       p.plane_words, s->draw, s->tile_prefix.as<const uint64_t>(), columns ? out->contig : nullptr,
                       columns ? out->pos : nullptr, columns ? out->ref : nullptr, columns ? out->alt : nullptr);
  HIP_TRY(e, s->sp.end(1, st));
  eng_planes_rewritten(e);
  s->sp.mark(1);
  return sync_check(e, "strain apply");
}

int simmr_last_strain_ms(simmr_engine* e, float* ms) {
  if (!e || !ms) return SIMMR_EINVAL;
  StrainState* s = strain_state(e, false);
  if (!s || !s->sp.valid[0]) return eng_fail(e, SIMMR_ESTATE, "no simmr_strain_plan yet");
  return s->sp.total_ms(e, "strain", ms);
}

}  // extern "C"
