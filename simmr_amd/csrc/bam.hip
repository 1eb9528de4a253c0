// bam.hip — the true alignments as BAM records and BGZF framing of a device buffer (include/simmr_hip.h: simmr_bam_*,
// simmr_bgzf_*): the entry points over bam_kernels.hip, the state, and the host tables of the CRC (bgzf_tables.hpp).  A
// translation unit of libsimmr_hip.so of its own; like sam.hip it sees an engine through engine_internal.hpp only and keeps its
// state in a slot of its own (ENG_EXT_BAM), so a BAM plan and a SAM plan on one engine do not disturb each other.  The names
// table and the argument checks are sam.hip's (sam_names.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "bam_kernels.hip"
#include "bgzf_tables.hpp"
#include "sam_names.hpp"

using namespace simmr;

static_assert(bgzf::SEG == BGZF_SEG && bgzf::LANES == BGZF_LANES && bgzf::BLOCK == BGZF_BLOCK && bgzf::POLY == BGZF_POLY,
              "bgzf_tables.hpp states the kernel's geometry");

namespace {

struct BamState {
  SamNameTable nt;  // the names of the last plan (sam_names.hpp)
  DevBuf len, off, chunk_sum, chunk_prefix;
  DevBuf word;  // the total (64 bits), then the error word
  // what the plan was made for: every column and both capacities, as the kernels read them
  SamReads reads{};
  SamEdits edits{};
  uint32_t paired = 0;
  uint64_t n_reads = 0, total = 0, epoch = 0;
  bool ready = false, planned_once = false, emitted = false;
  hipEvent_t ev[4] = {};
  // BGZF: the CRC tables, made and uploaded by the first simmr_bgzf_frame
  DevBuf tables;
  std::unique_ptr<bgzf::Tables> h_tables;
  bool tables_ready = false;

  uint32_t* err_p() const { return (uint32_t*)(word.as<char>() + 8); }
  BgzfTables bgzf_tables() const {
    const uint32_t* p = tables.as<const uint32_t>();
    return BgzfTables{p, p + 4 * 256, p + 4 * 256 + (BGZF_LANES - 1u)};
  }
};

void bam_destroy(void* q) {
  BamState* s = (BamState*)q;
  s->nt.release();
  for (DevBuf* b : {&s->len, &s->off, &s->chunk_sum, &s->chunk_prefix, &s->word, &s->tables}) b->release();
  for (hipEvent_t ev : s->ev)
    if (ev) (void)hipEventDestroy(ev);
  delete s;
}

BamState* state_of(simmr_engine* e, bool create) {
  void** slot = eng_ext_slot(e, ENG_EXT_BAM, bam_destroy);
  if (!*slot && create) *slot = new BamState();
  return (BamState*)*slot;
}

}  // namespace

extern "C" {

int simmr_bam_plan(simmr_engine* e, const simmr_sam_names* names, const simmr_reads_out* reads, const simmr_truth_out* truth,
                   uint64_t n_reads, int paired, uint64_t* record_bytes) {
  if (!e) return SIMMR_EINVAL;
  if (BamState* old = state_of(e, false)) old->ready = old->emitted = false;
  if (int rc = check_plan_args(e, names, reads, truth, n_reads, paired, record_bytes, "simmr_bam_plan")) return rc;
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  BamState* s = state_of(e, true);
  if (int rc = sam_sync_check(e, "BAM plan")) return rc;  // (an upload of an earlier plan that failed may still read the host copies)
  if (int rc = s->nt.build(e, names)) return rc;
  if (s->nt.n_rows > 0x7fffffffull)
    return eng_fail(e, SIMMR_ERANGE, "simmr_bam_plan: %llu named contigs: refID is an int32", (unsigned long long)s->nt.n_rows);
  for (hipEvent_t& ev : s->ev)
    if (!ev) SAM_TRY(e, hipEventCreate(&ev));
  const uint64_t n_chunks = (n_reads + SAM_CHUNK - 1) / SAM_CHUNK;
  if (!s->nt.ensure(false) || !s->len.ensure(std::max<uint64_t>(n_reads, 1) * 4) || !s->off.ensure((n_reads + 1) * 8) ||
      !s->chunk_sum.ensure(std::max<uint64_t>(n_chunks, 1) * 8) || !s->chunk_prefix.ensure((n_chunks + 1) * 8) || !s->word.ensure(16))
    return eng_fail(e, SIMMR_ENOMEM, "BAM plan allocation failed (%llu reads)", (unsigned long long)n_reads);
  hipStream_t st = eng_stream(e);
  SAM_TRY(e, s->nt.upload(st, false));
  SAM_TRY(e, hipMemsetAsync(s->word.p, 0, 16, st));
  SAM_TRY(e, hipEventRecord(s->ev[0], st));
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_chunks, (uint64_t)eng_cu_count(e) * SAM_WGS_PER_CU));
  if (n_reads > 0)
    hipLaunchKernelGGL(k_bam_size, dim3(grid), dim3(256), 0, st, sam_reads(reads), sam_edits(truth), s->nt.names(), n_reads, paired ? 1u : 0u,
                       s->len.as<uint32_t>(), s->chunk_sum.as<uint64_t>(), s->err_p());
  hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(256), 0, st, s->chunk_sum.as<const uint64_t>(), s->chunk_prefix.as<uint64_t>(), n_chunks);
  hipLaunchKernelGGL(k_bam_offsets, dim3(grid), dim3(256), 0, st, s->len.as<const uint32_t>(), s->chunk_prefix.as<const uint64_t>(), n_reads,
                     s->off.as<uint64_t>());
  SAM_TRY(e, hipEventRecord(s->ev[1], st));
  uint64_t total = 0;
  uint32_t errw = 0;
  SAM_TRY(e, hipMemcpyAsync(&total, s->off.as<uint64_t>() + n_reads, 8, hipMemcpyDeviceToHost, st));
  SAM_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sam_sync_check(e, "BAM size pass")) return rc;
  s->planned_once = true;
  if (errw)
    return eng_fail(e, SIMMR_EINVAL, "a read's genome / contig has no name, its bytes leave seq[], it is longer than %u bases, it ends at 2^31 or "
                                     "beyond, its edit_off decreases or leaves edits_capacity, or its edit_pos do not ascend inside the read", SAM_MAX_L);
  s->reads = sam_reads(reads);
  s->edits = sam_edits(truth);
  s->paired = paired ? 1u : 0u;
  s->n_reads = n_reads;
  s->total = total;
  s->epoch = eng_staging_epoch(e);
  s->ready = true;
  *record_bytes = total;
  return SIMMR_OK;
}

int simmr_bam_emit(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* truth, uint8_t* dst, uint64_t dst_capacity) {
  if (!e) return SIMMR_EINVAL;
  if (!reads || !truth) return eng_fail(e, SIMMR_EINVAL, "simmr_bam_emit: NULL argument");
  BamState* s = state_of(e, false);
  if (s) s->emitted = false;
  SamReads now_r{};  // (zeroed first: the structs are compared as bytes, padding included)
  SamEdits now_e{};
  std::memset(&now_r, 0, sizeof now_r);
  std::memset(&now_e, 0, sizeof now_e);
  assign_reads(&now_r, reads);
  assign_edits(&now_e, truth);
  if (!s || !s->ready || std::memcmp(&now_r, &s->reads, sizeof now_r) != 0 || std::memcmp(&now_e, &s->edits, sizeof now_e) != 0)
    return eng_fail(e, SIMMR_ESTATE, "simmr_bam_emit called without a simmr_bam_plan for these columns");
  if (s->epoch != eng_staging_epoch(e)) return eng_fail(e, SIMMR_ESTATE, "a genome was staged since simmr_bam_plan: plan again");
  if (int rc = check_columns(e, reads, truth, "simmr_bam_emit")) return rc;
  if (dst_capacity < s->total)
    return eng_fail(e, SIMMR_ERANGE, "dst_capacity %llu < %llu bytes planned", (unsigned long long)dst_capacity, (unsigned long long)s->total);
  if (s->total > 0 && !dst) return eng_fail(e, SIMMR_EINVAL, "simmr_bam_emit: NULL dst");
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  SAM_TRY(e, hipEventRecord(s->ev[2], st));
  if (s->n_reads > 0) {
    const uint64_t n_batches = (s->n_reads + SAM_WG_READS - 1) / SAM_WG_READS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_batches, (uint64_t)eng_cu_count(e) * SAM_WGS_PER_CU);
    hipLaunchKernelGGL(k_bam_write, dim3(grid), dim3(256), 0, st, s->reads, s->edits, s->nt.names(), s->n_reads, s->paired,
                       s->off.as<const uint64_t>(), dst, s->err_p());
  }
  SAM_TRY(e, hipEventRecord(s->ev[3], st));
  uint32_t errw = 0;
  SAM_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sam_sync_check(e, "BAM write pass")) return rc;
  s->emitted = true;
  if (errw) {
    s->ready = false;
    return eng_fail(e, SIMMR_EINVAL, "the columns changed since simmr_bam_plan: a read failed the bounds check of the write pass (no store "
                                     "left its record)");
  }
  return SIMMR_OK;
}

int simmr_last_bam_ms(simmr_engine* e, float* ms) {
  if (!e || !ms) return SIMMR_EINVAL;
  BamState* s = state_of(e, false);
  if (!s || !s->planned_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_bam_plan yet");
  if (int rc = sam_sync_check(e, "bam")) return rc;
  float a = 0.f, b = 0.f;
  SAM_TRY(e, hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
  if (s->emitted) SAM_TRY(e, hipEventElapsedTime(&b, s->ev[2], s->ev[3]));
  *ms = a + b;
  return SIMMR_OK;
}

uint64_t simmr_bgzf_bound(uint64_t n_bytes) {
  return n_bytes + (uint64_t)BGZF_OVERHEAD * (n_bytes / BGZF_BLOCK + (n_bytes % BGZF_BLOCK ? 1u : 0u));
}

int simmr_bgzf_frame(simmr_engine* e, const uint8_t* src, uint64_t n_bytes, uint8_t* dst, uint64_t dst_capacity, uint64_t* written) {
  if (!e) return SIMMR_EINVAL;
  if (!written) return eng_fail(e, SIMMR_EINVAL, "simmr_bgzf_frame: NULL written");
  *written = 0;
  if (n_bytes == 0) return SIMMR_OK;
  if (n_bytes > (1ull << 62)) return eng_fail(e, SIMMR_ERANGE, "simmr_bgzf_frame: %llu bytes", (unsigned long long)n_bytes);
  const uint64_t bound = simmr_bgzf_bound(n_bytes);
  if (dst_capacity < bound)
    return eng_fail(e, SIMMR_ERANGE, "dst_capacity %llu < %llu bytes of blocks", (unsigned long long)dst_capacity, (unsigned long long)bound);
  if (!src || !dst) return eng_fail(e, SIMMR_EINVAL, "simmr_bgzf_frame: NULL buffer");
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
  if (s0 < d0 + bound && d0 < s0 + n_bytes) return eng_fail(e, SIMMR_EINVAL, "simmr_bgzf_frame: src and dst overlap");
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  BamState* s = state_of(e, true);
  hipStream_t st = eng_stream(e);
  if (!s->tables_ready) {
    if (!s->h_tables) {
      s->h_tables = std::make_unique<bgzf::Tables>();
      bgzf::make_tables(s->h_tables.get());
    }
    if (!s->tables.ensure(sizeof(bgzf::Tables))) return eng_fail(e, SIMMR_ENOMEM, "BGZF table allocation failed");
    SAM_TRY(e, hipMemcpyAsync(s->tables.p, s->h_tables.get(), sizeof(bgzf::Tables), hipMemcpyHostToDevice, st));
    if (int rc = sam_sync_check(e, "BGZF tables")) return rc;
    s->tables_ready = true;
  }
  const uint64_t n_blocks = (n_bytes + BGZF_BLOCK - 1) / BGZF_BLOCK;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(n_blocks, (uint64_t)eng_cu_count(e) * 8u);
  hipLaunchKernelGGL(k_bgzf_frame, dim3(grid), dim3(BGZF_LANES), 0, st, src, n_bytes, dst, s->bgzf_tables());
  if (int rc = sam_sync_check(e, "BGZF framing")) return rc;
  *written = bound;
  return SIMMR_OK;
}

}  // extern "C"
