// bam.hip — the true alignments as BAM records and BGZF framing of a device buffer (include/simmr_hip.h: simmr_bam_*,
// simmr_bgzf_*): the entry points over bam_kernels.hip, the state, and the host tables of the CRC (bgzf_tables.hpp).  A
// translation unit of libsimmr_hip.so of its own; like sam.hip it sees an engine through engine_internal.hpp only and keeps its
// state in a slot of its own (ENG_EXT_BAM), so a BAM plan and a SAM plan on one engine do not disturb each other.  The names
// table and the argument checks are sam.hip's (sam_names.hpp); the plan, the emit and the timer of the records are the shared ones
// of record_stream_host.hpp, given this unit's traits (BamFormat).  simmr_bgzf_* and the CRC tables are this unit's alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "bam_kernels.hip"
#include "bgzf_tables.hpp"
#include "record_stream_host.hpp"

using namespace simmr;

static_assert(bgzf::SEG == BGZF_SEG && bgzf::LANES == BGZF_LANES && bgzf::BLOCK == BGZF_BLOCK && bgzf::POLY == BGZF_POLY,
              "bgzf_tables.hpp states the kernel's geometry");

namespace {

// the CRC tables of BGZF framing, made and uploaded by the first simmr_bgzf_frame, beside the record writer's state
struct BamState {
  RecordStreamState rec;
  DevBuf tables;
  std::unique_ptr<bgzf::Tables> h_tables;
  bool tables_ready = false;

  BgzfTables bgzf_tables() const {
    const uint32_t* p = tables.as<const uint32_t>();
    return BgzfTables{p, p + 4 * 256, p + 4 * 256 + (BGZF_LANES - 1u)};
  }
};

constexpr auto bam_state = unit_state<BamState, ENG_EXT_BAM>;

struct BamFormat : RecordFormat {
  static constexpr const char *PLAN = "simmr_bam_plan", *EMIT = "simmr_bam_emit", *NOUN = "BAM", *TIMER = "bam";
  static constexpr const char *SYNC_PLAN = "BAM plan", *SYNC_SIZE = "BAM size pass", *SYNC_WRITE = "BAM write pass";
  static constexpr const char* PLAN_REFUSAL =
      "a read's genome / contig has no name, its bytes leave seq[], it is longer than %u bases, it ends at 2^31 or beyond, its edit_off decreases or "
      "leaves edits_capacity, or its edit_pos do not ascend inside the read";
  static int check_names(simmr_engine* e, const SamNameTable& nt) {
    if (nt.n_rows > 0x7fffffffull) return eng_fail(e, SIMMR_ERANGE, "simmr_bam_plan: %llu named contigs: refID is an int32", (unsigned long long)nt.n_rows);
    return SIMMR_OK;
  }
  static RecordStreamState* state(simmr_engine* e, bool create) {
    BamState* s = bam_state(e, create);
    return s ? &s->rec : nullptr;
  }
  static void size(hipStream_t st, uint32_t grid, RecordStreamState& s, const SamReads& rd, const SamEdits& ed, uint64_t n, uint32_t paired, uint32_t) {
    hipLaunchKernelGGL(k_bam_size, dim3(grid), dim3(256), 0, st, rd, ed, s.nt.names(), n, paired, s.len.as<uint32_t>(), s.chunk_sum.as<uint64_t>(), s.err_p());
  }
  static void scan(hipStream_t st, RecordStreamState& s, uint64_t n_chunks) {
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(256), 0, st, s.chunk_sum.as<const uint64_t>(), s.chunk_prefix.as<uint64_t>(), n_chunks);
  }
  static void offsets(hipStream_t st, uint32_t grid, RecordStreamState& s, const uint32_t* len, uint64_t n) {
    hipLaunchKernelGGL(k_bam_offsets, dim3(grid), dim3(256), 0, st, len, s.chunk_prefix.as<const uint64_t>(), n, s.off.as<uint64_t>());
  }
  static void write(hipStream_t st, uint32_t grid, RecordStreamState& s, uint8_t* dst) {
    hipLaunchKernelGGL(k_bam_write, dim3(grid), dim3(256), 0, st, s.reads, s.edits, s.nt.names(), s.n_reads, s.paired, s.off.as<const uint64_t>(), dst, s.err_p());
  }
};

}  // namespace

extern "C" {

int simmr_bam_plan(simmr_engine* e, const simmr_sam_names* names, const simmr_reads_out* reads, const simmr_truth_out* truth,
                   uint64_t n_reads, int paired, uint64_t* record_bytes) {
  return record_plan<BamFormat>(e, names, reads, truth, n_reads, paired, record_bytes);
}

int simmr_bam_emit(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* truth, uint8_t* dst, uint64_t dst_capacity) {
  return record_emit<BamFormat>(e, reads, truth, dst, dst_capacity, nullptr, nullptr, nullptr);
}

int simmr_last_bam_ms(simmr_engine* e, float* ms) { return record_ms<BamFormat>(e, ms); }

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
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  BamState* s = bam_state(e, true);
  hipStream_t st = eng_stream(e);
  if (!s->tables_ready) {
    if (!s->h_tables) {
      s->h_tables = std::make_unique<bgzf::Tables>();
      bgzf::make_tables(s->h_tables.get());
    }
    if (!s->tables.ensure(sizeof(bgzf::Tables))) return eng_fail(e, SIMMR_ENOMEM, "BGZF table allocation failed");
    HIP_TRY(e, hipMemcpyAsync(s->tables.p, s->h_tables.get(), sizeof(bgzf::Tables), hipMemcpyHostToDevice, st));
    if (int rc = sync_check(e, "BGZF tables")) return rc;
    s->tables_ready = true;
  }
  const uint64_t n_blocks = (n_bytes + BGZF_BLOCK - 1) / BGZF_BLOCK;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(n_blocks, (uint64_t)eng_cu_count(e) * 8u);
  hipLaunchKernelGGL(k_bgzf_frame, dim3(grid), dim3(BGZF_LANES), 0, st, src, n_bytes, dst, s->bgzf_tables());
  if (int rc = sync_check(e, "BGZF framing")) return rc;
  *written = bound;
  return SIMMR_OK;
}

}  // extern "C"
