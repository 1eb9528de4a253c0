// pileup.hip — allele counts at listed sites (include/simmr_hip.h: simmr_pileup_*): the entry points over
// pileup_kernels.hip.  The fifth translation unit of libsimmr_hip.so; it sees an engine through engine_internal.hpp only,
// records the dense layout of the staged genomes itself (as depth.hip does: it needs no simmr_depth_reset) and keeps its
// state in the engine's opaque slot (host_support.hpp: unit_state; simmr_engine_destroy deletes it, and its members free what they own).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "pileup_kernels.hip"
#include "host_support.hpp"

using namespace simmr;

namespace {

struct PileupState {
  // the layout recorded by the last reset: genome slots -> contigs -> first position
  std::vector<PileupSlot> slots;
  std::vector<uint64_t> cfirst;  // n_contigs + 1
  uint64_t n = 0, epoch = 0, added = 0;
  bool ready = false;
  DevBuf d_slots, d_cfirst, keys;
  DevBuf table;  // counts[n][2][5], then the first bad site of the reset (64 bits), then the adds' sticky error word
  Spans<1> sp;  // the last add

  size_t table_bytes() const { return (size_t)n * PILEUP_CELLS * 4u; }
  uint32_t* counts_p() const { return table.as<uint32_t>(); }
  unsigned long long* bad_p() const { return (unsigned long long*)(table.as<char>() + table_bytes()); }
  uint32_t* err_p() const { return (uint32_t*)(table.as<char>() + table_bytes() + 8); }
};

constexpr auto pileup_state = unit_state<PileupState, ENG_EXT_PILEUP>;

}  // namespace

extern "C" {

int simmr_pileup_reset(simmr_engine* e, const simmr_pileup_sites* sites) {
  if (!e) return SIMMR_EINVAL;
  if (!sites) return eng_fail(e, SIMMR_EINVAL, "simmr_pileup_reset: NULL argument");
  const uint64_t n = sites->n;
  if (n > 0 && (!sites->genome || !sites->contig || !sites->pos)) return eng_fail(e, SIMMR_EINVAL, "simmr_pileup_reset: NULL site column");
  if ((n + PILEUP_WG - 1) / PILEUP_WG >= (1ull << 31)) return eng_fail(e, SIMMR_ENOTSUP, "simmr_pileup_reset: too many sites for one launch");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  PileupState* s = pileup_state(e, true);
  s->ready = false;
  s->sp.invalidate_from(0);
  if (int rc = s->sp.create_missing(e)) return rc;
  // the dense layout of the genomes staged now: contig firsts, no padding (depth[]'s order)
  StagedRows rows = staged_rows(e);
  const uint32_t n_slots = rows.n_slots();
  s->slots.assign(n_slots, PileupSlot{0u, 0u});
  for (uint32_t g = 0; g < n_slots; g++) s->slots[g] = PileupSlot{rows.cbase[g], rows.ncontig[g]};
  s->cfirst = std::move(rows.first);
  s->n = n;
  if (!s->d_slots.ensure(std::max<size_t>(n_slots, 1) * sizeof(PileupSlot)) || !s->d_cfirst.ensure(s->cfirst.size() * 8) ||
      !s->keys.ensure(std::max<uint64_t>(n, 1) * 8) || !s->table.ensure(s->table_bytes() + 16))
    return eng_fail(e, SIMMR_ENOMEM, "pileup table allocation failed (%llu sites)", (unsigned long long)n);
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemsetAsync(s->table.p, 0, s->table_bytes() + 16, st));
  HIP_TRY(e, hipMemsetAsync(s->bad_p(), 0xff, 8, st));
  if (n_slots) HIP_TRY(e, hipMemcpyAsync(s->d_slots.p, s->slots.data(), n_slots * sizeof(PileupSlot), hipMemcpyHostToDevice, st));
  HIP_TRY(e, hipMemcpyAsync(s->d_cfirst.p, s->cfirst.data(), s->cfirst.size() * 8, hipMemcpyHostToDevice, st));
  if (n > 0)
    hipLaunchKernelGGL(k_pileup_keys, dim3((uint32_t)((n + PILEUP_WG - 1) / PILEUP_WG)), dim3(PILEUP_WG), 0, st, sites->genome, sites->contig,
                       sites->pos, n, s->d_slots.as<const PileupSlot>(), n_slots, s->d_cfirst.as<const uint64_t>(), s->keys.as<uint64_t>(),
                       s->bad_p());
  unsigned long long bad = ~0ull;
  HIP_TRY(e, hipMemcpyAsync(&bad, s->bad_p(), 8, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "pileup reset")) return rc;  // (the tables were copied from vectors the next reset rewrites)
  if (bad != ~0ull)
    return eng_fail(e, SIMMR_EINVAL, "site %llu: its genome slot is not staged, its contig does not exist, its position is not inside the "
                                     "contig, or it does not come after site %llu in (slot, contig, pos) order",
                    bad, bad ? bad - 1 : 0ull);
  s->epoch = eng_staging_epoch(e);
  s->added = 0;
  s->ready = true;
  return SIMMR_OK;
}

int simmr_pileup_add(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads) {
  if (!e) return SIMMR_EINVAL;
  if (!reads) return eng_fail(e, SIMMR_EINVAL, "simmr_pileup_add: NULL argument");
  if (!reads->seq || !reads->seq_off || !reads->start || !reads->end || !reads->contig || !reads->genome || !reads->flags)
    return eng_fail(e, SIMMR_EINVAL, "simmr_pileup_add needs seq, seq_off, start, end, contig, genome and flags");
  PileupState* s = pileup_state(e, false);
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_pileup_add called before simmr_pileup_reset");
  if (s->epoch != eng_staging_epoch(e))
    return eng_fail(e, SIMMR_ESTATE, "a genome was staged since simmr_pileup_reset: the sites' keys are the reset's");
  if (n_reads >= (1ull << 31) || s->added + n_reads >= (1ull << 31))
    return eng_fail(e, SIMMR_ERANGE, "the reads added since simmr_pileup_reset would reach 2^31");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, s->sp.begin(0, st));
  if (n_reads > 0 && s->n > 0) {
    // persistent: eight waves per SIMD's worth of waves, each looping over its share of the 64-read batches
    const uint64_t batches = (n_reads + 63) / 64, wgs = (batches + PILEUP_WG / 64 - 1) / (PILEUP_WG / 64);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)eng_cu_count(e) * PILEUP_WGS_PER_CU);
    const PileupReads rd{reads->seq, reads->seq_off, reads->start, reads->end, reads->contig, reads->genome, reads->flags, reads->seq_capacity};
    hipLaunchKernelGGL(k_pileup_add, dim3(grid), dim3(PILEUP_WG), 0, st, rd, n_reads, s->d_slots.as<const PileupSlot>(),
                       (uint32_t)s->slots.size(), s->d_cfirst.as<const uint64_t>(), s->keys.as<const uint64_t>(), s->n, s->counts_p(), s->err_p());
  }
  HIP_TRY(e, s->sp.end(0, st));
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "pileup launch failed: %s", hipGetErrorString(rc));
  s->added += n_reads;
  s->sp.mark(0);
  return SIMMR_OK;
}

int simmr_pileup_read(simmr_engine* e, uint32_t* counts_device, uint64_t capacity_sites) {
  if (!e) return SIMMR_EINVAL;
  PileupState* s = pileup_state(e, false);
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_pileup_read called before simmr_pileup_reset");
  if (capacity_sites < s->n)
    return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu sites", (unsigned long long)capacity_sites, (unsigned long long)s->n);
  if (s->n > 0 && !counts_device) return eng_fail(e, SIMMR_EINVAL, "simmr_pileup_read: NULL argument");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "pileup add")) return rc;
  if (errw)
    return eng_fail(e, SIMMR_EINVAL, "a read added since the last simmr_pileup_reset names a genome slot that is not tracked or a contig "
                                     "that does not exist, or its window leaves its contig or its bytes leave seq[]");
  if (s->n > 0) HIP_TRY(e, hipMemcpyAsync(counts_device, s->counts_p(), s->table_bytes(), hipMemcpyDeviceToDevice, st));
  return sync_check(e, "pileup read");
}

int simmr_last_pileup_ms(simmr_engine* e, float* ms) {
  if (!e || !ms) return SIMMR_EINVAL;
  PileupState* s = pileup_state(e, false);
  if (!s || !s->sp.valid[0]) return eng_fail(e, SIMMR_ESTATE, "no simmr_pileup_add yet");
  return s->sp.total_ms(e, "pileup", ms);
}

}  // extern "C"
