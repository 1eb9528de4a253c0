// stats.hip — run statistics (include/simmr_hip.h: simmr_stats_*): the entry points over stats_kernels.hip.  A translation
// unit of its own; it sees an engine through engine_internal.hpp only and keeps its state in the engine's opaque slot
// (host_support.hpp: unit_state; simmr_engine_destroy deletes it, and its members free what they own).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "truth_host.hpp"  // the read walker and the columns, grid and checks shared with truth.hip
#include "stats_kernels.hip"

using namespace simmr;

namespace {

static_assert(TRUTH_WG_READS == STATS_WG_READS, "k_truth and k_read_stats batch their reads alike");  // (row_grid)
const size_t STATS_BYTES = sizeof(simmr_run_stats) + 8;  // the tables and the error word behind them

struct StatsState {
  DevBuf tab;   // the simmr_run_stats the kernel adds to, followed by its sticky error word
  Spans<1> sp;  // the last add
  bool ready = false;
};

constexpr auto stats_state = unit_state<StatsState, ENG_EXT_STATS>;

}  // namespace

extern "C" {

int simmr_stats_reset(simmr_engine* e) {
  if (!e) return SIMMR_EINVAL;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  StatsState* s = stats_state(e, true);
  if (int rc = s->sp.create_missing(e)) return rc;
  if (!s->tab.ensure_slack(STATS_BYTES)) return eng_fail(e, SIMMR_ENOMEM, "statistics allocation failed");
  HIP_TRY(e, hipMemsetAsync(s->tab.p, 0, STATS_BYTES, eng_stream(e)));
  s->ready = true;
  s->sp.invalidate_from(0);
  return SIMMR_OK;
}

int simmr_stats_add(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads, uint32_t n_sets) {
  if (!e) return SIMMR_EINVAL;
  if (!reads) return eng_fail(e, SIMMR_EINVAL, "simmr_stats_add: NULL argument");
  if (n_sets != 1u && n_sets != 2u) return eng_fail(e, SIMMR_EINVAL, "simmr_stats_add: n_sets is 1 or 2");
  // (seq and qual are asked for even of no reads)
  if (int rc = check_read_columns(e, reads, std::max<uint64_t>(n_reads, 1), "simmr_stats_add")) return rc;
  StatsState* s = stats_state(e, false);
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_stats_add called before simmr_stats_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, s->sp.begin(0, st));
  if (n_reads > 0) {
    uint32_t n_genomes = 0;
    const GenomeDev* genomes = eng_genome_table(e, &n_genomes);
    unsigned long long* tab = s->tab.as<unsigned long long>();
    hipLaunchKernelGGL(k_read_stats, dim3(row_grid(e, n_reads, STATS_WGS_PER_CU)), dim3(256), 0, st, genomes, n_genomes, truth_reads(reads), n_reads,
                       n_sets, reads->qual_offset, tab, (uint32_t*)(tab + STATS_TABLE_WORDS));
  }
  HIP_TRY(e, s->sp.end(0, st));
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "statistics launch failed: %s", hipGetErrorString(rc));
  s->sp.mark(0);
  return SIMMR_OK;
}

int simmr_stats_read(simmr_engine* e, simmr_run_stats* dst_host) {
  if (!e) return SIMMR_EINVAL;
  if (!dst_host) return eng_fail(e, SIMMR_EINVAL, "simmr_stats_read: NULL argument");
  StatsState* s = stats_state(e, false);
  if (!s || !s->ready) return eng_fail(e, SIMMR_ESTATE, "simmr_stats_read called before simmr_stats_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  std::vector<uint64_t> host(STATS_BYTES / 8);
  HIP_TRY(e, hipMemcpyAsync(host.data(), s->tab.p, STATS_BYTES, hipMemcpyDeviceToHost, eng_stream(e)));
  if (int rc = sync_check(e, "statistics readback")) return rc;
  if (host[STATS_TABLE_WORDS] != 0)
    return eng_fail(e, SIMMR_EINVAL, "a read added since the last simmr_stats_reset names a genome or contig that is not staged, "
                                     "its coordinates leave the contig or seq[], or it is longer than 65535 bases");
  memcpy(dst_host, host.data(), sizeof(simmr_run_stats));
  return SIMMR_OK;
}

int simmr_last_stats_ms(simmr_engine* e, float* ms) {
  if (!e || !ms) return SIMMR_EINVAL;
  StatsState* s = stats_state(e, false);
  if (!s || !s->sp.valid[0]) return eng_fail(e, SIMMR_ESTATE, "no simmr_stats_add yet");
  return s->sp.total_ms(e, "statistics", ms);
}

}  // extern "C"
