// asmmap.hip — an assembler's contigs placed on the gold-standard assembly (include/simmr_hip.h: simmr_asmmap_*): the entry points
// over asmmap_kernels.hip, on the scaffold of scorer_host.hpp.  The text-to-planes stage is asmeval's (asmeval_front.hpp), every
// scan is the engine's (eng_scan_u32).
//
// truth_add:  the front, the genome of every record, the truth rows (genome, length), the roll; the occurrences (key, t << 1 | o, p)
//             are appended through a cursor, their columns sized from the bytes of every truth add since the reset and the truth
//             rows from their lines.  Only enqueues.
// truth_plan: reads the cursor, sorts over 2k bits, marks anchors and repeat heads, scans both marks (each scan synchronises and
//             gives a total), compacts the two indexes, builds their prefix tables, sums by_genome's truth columns and empties
//             the candidate side.
// add:        the front, then SYNCHRONISES for the add's bases and records; count pass, scan (hits), write pass, run heads, scan
//             (runs), run columns, kept marks, scan (kept runs), their compaction, block heads, scan (blocks), block columns,
//             spans, joins.  Five waits: each total sizes what the next stage writes.
// Time: the adds' span and the plan's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_support.hpp"
#include "asmmap_kernels.hip"
#include "asmeval_front.hpp"
#include "sam_names.hpp"
#include "scorer_host.hpp"

using namespace simmr;

namespace {

enum { SPAN_ADDS = 0, SPAN_PLAN = 1, SPAN_COUNT = 2 };
constexpr uint32_t TABLE_MAX_BITS = 24;  // the prefix table: min(24, bit length of the entries) bits of the key's top

const char* const MALFORMED_TRUTH =
    "a sequence line in front of the add's first header, a header with no '|' in its first word, or a prefix that is not among the genome names";
const char* const MALFORMED_CAND = "a sequence line in front of the add's first header";

}  // namespace

struct simmr_asmmap {
  simmr_engine* e = nullptr;
  DeviceNames genomes;
  uint32_t n_genomes = 0, k = 0, band = 0, relocation = 0, min_anchors = 0;
  AsmFront front;
  DevBuf rec_row;
  // the truth: the rows, the occurrences as appended, the sort's buffers, the two indexes
  DevBuf t_genome, t_len, u_key, u_to, u_p, mark_a, mark_r, before_a, before_r;
  PairSort order;
  DevBuf a_key, a_t, a_p, a_o, a_table, r_key, r_table, g_truth;
  DevBuf cursor, counts, word;
  // one add: the hits, the runs, the kept runs and their scans
  DevBuf lane_hits, lane_off, h_c, h_q, h_ts, h_d, run_head, run_before, r_first, r_last, kept, kept_before, k_first, k_last, blk_head, blk_before;
  // since the plan: the contig and block columns; the tables of a read
  DevBuf c_len, c_hits, c_blocks, c_first, c_bb, c_worst, b_col[9], b_dfirst, b_dlast, g_blocks;
  uint64_t occ_cap = 0, truth_cap = 0;
  uint64_t n_truth = 0, n_anchors = 0, n_repeats = 0, n_contigs = 0, contig_cap = 0, n_blocks = 0, block_cap = 0, n_runs = 0;
  uint32_t a_bits = 0, r_bits = 0;
  uint32_t max_wgs = 0;  // SIMMR_ASMMAP_MAX_WGS; 0: no cap
  bool reset_once = false, planned = false;
  FoldedSpans<SPAN_COUNT> sp;

  MevNames names() const { return genomes.names(n_genomes); }
  AmapAnchors anchors() const {
    return AmapAnchors{AsmEntries{a_key.as<const uint64_t>(), nullptr, a_table.as<const uint32_t>(), (uint32_t)n_anchors, a_bits, 2u * k - a_bits},
                       AsmEntries{r_key.as<const uint64_t>(), nullptr, r_table.as<const uint32_t>(), (uint32_t)n_repeats, r_bits, 2u * k - r_bits},
                       a_t.as<const uint32_t>(), a_p.as<const uint32_t>(), a_o.as<const uint32_t>()};
  }
  AmapHits hits() const { return AmapHits{h_c.as<uint32_t>(), h_q.as<uint32_t>(), h_ts.as<uint32_t>(), h_d.as<long long>()}; }
  AmapBlocks blocks() const {
    return AmapBlocks{b_col[0].as<uint32_t>(), b_col[1].as<uint32_t>(), b_col[2].as<uint32_t>(), b_col[3].as<uint32_t>(), b_col[4].as<uint32_t>(),
                      b_col[5].as<uint32_t>(), b_col[6].as<uint32_t>(), b_col[7].as<uint32_t>(), b_col[8].as<uint32_t>(), b_dfirst.as<long long>(),
                      b_dlast.as<long long>()};
  }
  AmapContigs contigs() const {
    return AmapContigs{c_len.as<uint64_t>(), c_hits.as<uint32_t>(), c_blocks.as<uint32_t>(), c_first.as<uint32_t>(), c_bb.as<unsigned long long>(),
                       c_worst.as<uint32_t>()};
  }
  unsigned long long* counts_p() const { return counts.as<unsigned long long>(); }
  unsigned long long* cursor_p() const { return cursor.as<unsigned long long>(); }
};

namespace {

int check_add(simmr_asmmap* h, const uint8_t* text, uint64_t n_bytes, const char* who) {
  return check_add_text(h->e, h->reset_once, text, n_bytes, SIMMR_ASMEVAL_MAX_BYTES, who, "simmr_asmmap_reset", "cut the text in front of a header");
}

// the workgroups of a launch of one of this unit's kernels over `items`; SIMMR_ASMMAP_MAX_WGS (read at create, include/simmr_hip.h)
// caps them, so that a test reaches a grid's second trip with a small text: every answer is the same for any value.  The front's
// launches are asmeval's (asm_front_launch) and are not capped.
uint32_t grid_for(const simmr_asmmap* h, uint64_t items, uint32_t per_wg, uint32_t wgs_per_cu) {
  const uint64_t cus = (uint64_t)std::max(eng_cu_count(h->e), 1);
  return grid_capped(items, per_wg, h->max_wgs ? std::min<uint64_t>(cus * wgs_per_cu, h->max_wgs) : cus * wgs_per_cu);
}

int enqueue_front(simmr_asmmap* h, const uint8_t* text, uint64_t n_bytes, hipStream_t st, bool truth, MevText* W) {
  if (!h->front.ensure(n_bytes)) return eng_fail(h->e, SIMMR_ENOMEM, "asmmap: allocation failed for %llu bytes of text", (unsigned long long)n_bytes);
  const AsmFrontSums sums{h->counts_p(), (uint32_t)(truth ? AM_T_RECORDS : AM_RECORDS), (uint32_t)(truth ? AM_T_BASES : AM_BASES),
                          (uint32_t)(truth ? AM_T_INVALID : AM_INVALID), h->word.as<uint32_t>(), truth ? ASM_ERR_TRUTH : ASM_ERR_CAND};
  asm_front_launch(h->e, st, text, n_bytes, h->front.bufs(), sums, W);
  return SIMMR_OK;
}

// the prefix table over n sorted keys: its bits, and the launch
int build_table(simmr_asmmap* h, hipStream_t st, const DevBuf& keys, uint64_t n, DevBuf* table, uint32_t* bits_out) {
  const uint32_t bits = std::min(TABLE_MAX_BITS, bits_of(n));
  *bits_out = n > 0 ? bits : 0u;
  if (!table->ensure(((1ull << bits) + 1) * 4)) return eng_fail(h->e, SIMMR_ENOMEM, "asmmap truth plan: allocation failed (%llu entries)", (unsigned long long)n);
  if (n > 0)
    hipLaunchKernelGGL(k_amap_table, dim3(grid_for(h, (1ull << bits) + 1, AMAP_WG, 32)), dim3(AMAP_WG), 0, st, keys.as<const uint64_t>(), (uint32_t)n, bits,
                       2u * h->k - bits, table->as<uint32_t>());
  return SIMMR_OK;
}

}  // namespace

extern "C" {

int simmr_asmmap_create(simmr_engine* e, simmr_asmmap** out) {
  if (int rc = scorer_create(e, out, "simmr_asmmap_create")) return rc;
  if (const char* v = std::getenv("SIMMR_ASMMAP_MAX_WGS")) (*out)->max_wgs = (uint32_t)std::max(std::atoi(v), 0);
  return SIMMR_OK;
}

void simmr_asmmap_destroy(simmr_asmmap* h) { scorer_destroy(h); }

int simmr_asmmap_reset(simmr_asmmap* h, const simmr_asmmap_config* cfg) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!cfg || (cfg->n_genomes > 0 && !cfg->genome)) return eng_fail(e, SIMMR_EINVAL, "simmr_asmmap_reset: NULL argument");
  if (cfg->k < 15u || cfg->k > 31u || cfg->k % 2u == 0u) return eng_fail(e, SIMMR_EINVAL, "simmr_asmmap_reset: k = %u (an odd number of 15 to 31)", cfg->k);
  if (cfg->relocation >= (1u << 31)) return eng_fail(e, SIMMR_EINVAL, "simmr_asmmap_reset: relocation = %u (below 2^31)", cfg->relocation);
  if (cfg->band > cfg->relocation) return eng_fail(e, SIMMR_EINVAL, "simmr_asmmap_reset: band = %u above relocation = %u", cfg->band, cfg->relocation);
  if (cfg->min_anchors == 0u) return eng_fail(e, SIMMR_EINVAL, "simmr_asmmap_reset: min_anchors = 0 (at least 1)");
  if (cfg->n_genomes > (1u << 24) - 1u) return eng_fail(e, SIMMR_ERANGE, "simmr_asmmap_reset: %u genome names (fewer than 2^24)", cfg->n_genomes);
  SortedNames sorted;
  if (int rc = sorted_names(e, cfg->genome, cfg->n_genomes, SAM_RNAME_MAX, rname_legal, "genome name", nullptr, &sorted)) return rc;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = sync_check(e, "asmmap reset")) return rc;
  h->planned = false;
  h->reset_once = false;
  if (int rc = h->sp.reset(e)) return rc;
  if (!h->genomes.room(sorted) || !h->cursor.ensure(16) || !h->counts.ensure(AM_COUNT * 8) || !h->word.ensure(16))
    return eng_fail(e, SIMMR_ENOMEM, "asmmap reset: allocation failed");
  hipStream_t st = eng_stream(e);
  if (int rc = h->genomes.upload(e, sorted, st)) return rc;
  HIP_TRY(e, hipMemsetAsync(h->cursor.p, 0, 16, st));
  HIP_TRY(e, hipMemsetAsync(h->counts.p, 0, AM_COUNT * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->word.p, 0, 16, st));
  if (int rc = sync_check(e, "asmmap reset")) return rc;  // (the uploads read host vectors that end here)
  h->n_genomes = cfg->n_genomes;
  h->k = cfg->k;
  h->band = cfg->band;
  h->relocation = cfg->relocation;
  h->min_anchors = cfg->min_anchors;
  h->occ_cap = h->truth_cap = 0;
  h->n_truth = h->n_anchors = h->n_repeats = h->n_contigs = h->contig_cap = h->n_blocks = h->block_cap = h->n_runs = 0;
  h->a_bits = h->r_bits = 0;
  h->reset_once = true;
  return SIMMR_OK;
}

int simmr_asmmap_truth_add(simmr_asmmap* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_asmmap_truth_add")) return rc;
  h->planned = false;
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t cap = h->occ_cap + n_bytes, held = h->occ_cap, rows = h->truth_cap + n_bytes / 2 + 1, rows_held = h->truth_cap;
  if (!h->u_key.grow_keep(cap * 8, held * 8, st) || !h->u_to.grow_keep(cap * 4, held * 4, st) || !h->u_p.grow_keep(cap * 4, held * 4, st) ||
      !h->t_genome.grow_keep(rows * 4, rows_held * 4, st) || !h->t_len.grow_keep(rows * 4, rows_held * 4, st) || !h->rec_row.ensure((n_bytes / 2 + 1) * 4))
    return eng_fail(e, SIMMR_ENOMEM, "asmmap truth: allocation failed for %llu k-mer occurrences", (unsigned long long)cap);
  h->occ_cap = cap;
  h->truth_cap = rows;
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  if (int rc = enqueue_front(h, text, n_bytes, st, true, &W)) return rc;
  asm_front_genomes(e, st, W, h->front.lines(), h->names(), h->rec_row.as<uint32_t>(), h->word.as<uint32_t>());
  hipLaunchKernelGGL(k_amap_truth_records, dim3(grid_for(h, n_bytes / 2 + 1, AMAP_WG, 8)), dim3(AMAP_WG), 0, st, h->front.rec_start.as<const uint32_t>(),
                     h->front.tot.as<const uint32_t>(), h->rec_row.as<const uint32_t>(), (const unsigned long long*)h->counts_p(), rows, h->t_genome.as<uint32_t>(),
                     h->t_len.as<uint32_t>());
  hipLaunchKernelGGL(k_amap_roll_truth, dim3(grid_for(h, n_bytes / ASM_WORD + 1, AMAP_WG, 32)), dim3(AMAP_WG), 0, st, h->front.plane(), h->k,
                     (const unsigned long long*)h->counts_p(), h->u_key.as<uint64_t>(), h->u_to.as<uint32_t>(), h->u_p.as<uint32_t>(), cap, h->cursor_p());
  return h->sp.end(e, SPAN_ADDS, st, "asmmap truth add");
}

int simmr_asmmap_truth_plan(simmr_asmmap* h, uint64_t* n_anchors) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_asmmap_truth_plan called before simmr_asmmap_reset");
  h->planned = false;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  uint64_t cur = 0, n_truth = 0;
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(&cur, h->cursor.p, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&n_truth, h->counts_p() + AM_T_RECORDS, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "asmmap truth adds")) return rc;
  if (int rc = h->sp.fold(e, "asmmap")) return rc;
  if (errw & ASM_ERR_TRUTH) return eng_fail(e, SIMMR_EINVAL, "a malformed truth text: %s", MALFORMED_TRUTH);
  const uint64_t n = std::min(cur, h->occ_cap);
  n_truth = std::min(n_truth, h->truth_cap);
  if (n >= (1ull << 31))
    return eng_fail(e, SIMMR_ERANGE, "simmr_asmmap_truth_plan takes fewer than 2^31 k-mer occurrences (%llu given)", (unsigned long long)n);
  if (n_truth >= (1ull << 31))
    return eng_fail(e, SIMMR_ERANGE, "simmr_asmmap_truth_plan takes fewer than 2^31 truth records (%llu given)", (unsigned long long)n_truth);
  const uint64_t n1 = std::max<uint64_t>(n, 1);
  const uint64_t g2 = (uint64_t)std::max(h->n_genomes, 1u) * 2;
  if (!h->order.room(n1) || !h->mark_a.ensure(n1 * 4) || !h->mark_r.ensure(n1 * 4) || !h->before_a.ensure((n1 + 1) * 8) ||
      !h->before_r.ensure((n1 + 1) * 8) || !h->g_truth.ensure(g2 * 8))
    return eng_fail(e, SIMMR_ENOMEM, "asmmap truth plan: allocation failed (%llu k-mer occurrences)", (unsigned long long)n);
  if (int rc = h->sp.begin(e, SPAN_PLAN, st)) return rc;
  // the candidate side starts over
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + AM_RECORDS, 0, (AM_COUNT - AM_RECORDS) * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->g_truth.p, 0, g2 * 8, st));
  h->n_contigs = h->contig_cap = h->n_blocks = h->block_cap = h->n_runs = 0;
  uint64_t na = 0, nr = 0;
  const uint32_t grid = grid_for(h, n1, AMAP_WG, 32);
  PairSort::Sorted by_key{};
  if (n > 0) {
    HIP_TRY(e, hipMemcpyAsync(h->order.key[0].p, h->u_key.p, n * 8, hipMemcpyDeviceToDevice, st));
    by_key = h->order.sort(st, n, 2u * h->k);
    hipLaunchKernelGGL(k_amap_marks, dim3(grid), dim3(AMAP_WG), 0, st, by_key.keys, n, h->mark_a.as<uint32_t>(), h->mark_r.as<uint32_t>());
    if (int rc = eng_scan_u32(e, h->mark_a.as<const uint32_t>(), n, h->before_a.as<uint64_t>(), &na)) return rc;  // (synchronises)
    if (int rc = eng_scan_u32(e, h->mark_r.as<const uint32_t>(), n, h->before_r.as<uint64_t>(), &nr)) return rc;  // (synchronises)
  }
  const uint64_t na1 = std::max<uint64_t>(na, 1), nr1 = std::max<uint64_t>(nr, 1);
  if (!h->a_key.ensure(na1 * 8) || !h->a_t.ensure(na1 * 4) || !h->a_p.ensure(na1 * 4) || !h->a_o.ensure(na1 * 4) || !h->r_key.ensure(nr1 * 8))
    return eng_fail(e, SIMMR_ENOMEM, "asmmap truth plan: allocation failed (%llu anchors, %llu repeats)", (unsigned long long)na, (unsigned long long)nr);
  if (n > 0)
    hipLaunchKernelGGL(k_amap_index, dim3(grid), dim3(AMAP_WG), 0, st, by_key.keys, by_key.perm,
                       h->mark_a.as<const uint32_t>(), h->mark_r.as<const uint32_t>(), h->before_a.as<const uint64_t>(), h->before_r.as<const uint64_t>(),
                       h->u_to.as<const uint32_t>(), h->u_p.as<const uint32_t>(), n, na, nr, h->a_key.as<uint64_t>(), h->a_t.as<uint32_t>(), h->a_p.as<uint32_t>(),
                       h->a_o.as<uint32_t>(), h->r_key.as<uint64_t>());
  uint32_t a_bits = 0, r_bits = 0;
  if (int rc = build_table(h, st, h->a_key, na, &h->a_table, &a_bits)) return rc;
  if (int rc = build_table(h, st, h->r_key, nr, &h->r_table, &r_bits)) return rc;
  if (n_truth > 0)
    hipLaunchKernelGGL(k_amap_reduce_truth, dim3(grid_for(h, std::max(n_truth, na), AMAP_WG, 8)), dim3(AMAP_WG), 0, st, h->t_genome.as<const uint32_t>(),
                       h->t_len.as<const uint32_t>(), n_truth, h->a_t.as<const uint32_t>(), na, h->n_genomes, h->g_truth.as<unsigned long long>());
  if (int rc = h->sp.end(e, SPAN_PLAN, st, "asmmap truth plan")) return rc;
  if (int rc = sync_check(e, "asmmap truth plan")) return rc;
  h->n_truth = n_truth;
  h->n_anchors = na;
  h->n_repeats = nr;
  h->a_bits = a_bits;
  h->r_bits = r_bits;
  h->planned = true;
  if (int rc = h->sp.fold(e, "asmmap")) return rc;
  if (n_anchors) *n_anchors = na;
  return SIMMR_OK;
}

int simmr_asmmap_add(simmr_asmmap* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_asmmap_add")) return rc;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_asmmap_add called without a simmr_asmmap_truth_plan in force");
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  if (int rc = enqueue_front(h, text, n_bytes, st, false, &W)) return rc;
  uint32_t tot[3] = {0, 0, 0};
  HIP_TRY(e, hipMemcpyAsync(tot, h->front.tot.p, 12, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "asmmap add")) return rc;
  const uint64_t n_bases = tot[1], n_rec = tot[2], c0 = h->n_contigs, want = c0 + n_rec;
  if (want >= (1ull << 31)) return eng_fail(e, SIMMR_ERANGE, "simmr_asmmap_add takes fewer than 2^31 contigs since the plan (%llu given)", (unsigned long long)want);
  const uint64_t n_words = (n_bases + ASM_WORD - 1) / ASM_WORD;
  bool room = true;
  if (want > h->contig_cap) {
    const uint64_t cap = want + want / 2, held = h->contig_cap;
    room = grow_zero(&h->c_len, cap, held, 8, st) && grow_zero(&h->c_bb, cap, held, 8, st) && grow_zero(&h->c_hits, cap, held, 4, st) &&
           grow_zero(&h->c_blocks, cap, held, 4, st) && grow_zero(&h->c_first, cap, held, 4, st) && grow_zero(&h->c_worst, cap, held, 4, st);
    if (room) h->contig_cap = cap;
  }
  room = room && h->lane_hits.ensure(std::max<uint64_t>(n_words, 1) * 4) && h->lane_off.ensure((n_words + 1) * 8);
  if (!room) return eng_fail(e, SIMMR_ENOMEM, "asmmap add: allocation failed (%llu contigs, %llu bases)", (unsigned long long)want, (unsigned long long)n_bases);
  h->n_contigs = want;
  if (n_rec > 0)
    hipLaunchKernelGGL(k_amap_contig_len, dim3(grid_for(h, n_rec, AMAP_WG, 32)), dim3(AMAP_WG), 0, st, h->front.rec_start.as<const uint32_t>(), (uint32_t)n_rec, c0,
                       h->c_len.as<uint64_t>());
  if (n_words == 0) return h->sp.end(e, SPAN_ADDS, st, "asmmap add");
  // the hits: count, scan, write (without an anchor the k-mers and the repeat hits still count)
  hipLaunchKernelGGL(k_amap_roll_count, dim3(grid_for(h, n_words, AMAP_WG, 32)), dim3(AMAP_WG), 0, st, h->front.plane(), h->k, h->anchors(), c0,
                     h->c_hits.as<uint32_t>(), h->lane_hits.as<uint32_t>(), h->counts_p());
  uint64_t nh = 0;
  if (int rc = eng_scan_u32(e, h->lane_hits.as<const uint32_t>(), n_words, h->lane_off.as<uint64_t>(), &nh)) return rc;  // (synchronises)
  if (nh == 0) return h->sp.end(e, SPAN_ADDS, st, "asmmap add");
  if (!h->h_c.ensure(nh * 4) || !h->h_q.ensure(nh * 4) || !h->h_ts.ensure(nh * 4) || !h->h_d.ensure(nh * 8) || !h->run_head.ensure(nh * 4) ||
      !h->run_before.ensure((nh + 1) * 8))
    return eng_fail(e, SIMMR_ENOMEM, "asmmap add: allocation failed (%llu anchor hits)", (unsigned long long)nh);
  const uint32_t hit_grid = grid_for(h, nh, AMAP_WG, 32);
  hipLaunchKernelGGL(k_amap_roll_write, dim3(grid_for(h, n_words, AMAP_WG, 32)), dim3(AMAP_WG), 0, st, h->front.plane(), h->k, h->anchors(),
                     h->lane_hits.as<const uint32_t>(), h->lane_off.as<const uint64_t>(), nh, h->hits());
  // the runs
  hipLaunchKernelGGL(k_amap_run_heads, dim3(hit_grid), dim3(AMAP_WG), 0, st, h->hits(), nh, (uint64_t)h->band, h->run_head.as<uint32_t>());
  uint64_t nr = 0;
  if (int rc = eng_scan_u32(e, h->run_head.as<const uint32_t>(), nh, h->run_before.as<uint64_t>(), &nr)) return rc;  // (synchronises)
  if (!h->r_first.ensure(nr * 4) || !h->r_last.ensure(nr * 4) || !h->kept.ensure(nr * 4) || !h->kept_before.ensure((nr + 1) * 8))
    return eng_fail(e, SIMMR_ENOMEM, "asmmap add: allocation failed (%llu runs)", (unsigned long long)nr);
  h->n_runs += nr;
  const uint32_t run_grid = grid_for(h, nr, AMAP_WG, 32);
  hipLaunchKernelGGL(k_amap_runs, dim3(hit_grid), dim3(AMAP_WG), 0, st, h->run_head.as<const uint32_t>(), h->run_before.as<const uint64_t>(), nh, nr,
                     h->r_first.as<uint32_t>(), h->r_last.as<uint32_t>());
  hipLaunchKernelGGL(k_amap_kept, dim3(run_grid), dim3(AMAP_WG), 0, st, h->r_first.as<const uint32_t>(), h->r_last.as<const uint32_t>(), nr, h->min_anchors,
                     h->kept.as<uint32_t>(), h->counts_p());
  uint64_t nk = 0;
  if (int rc = eng_scan_u32(e, h->kept.as<const uint32_t>(), nr, h->kept_before.as<uint64_t>(), &nk)) return rc;  // (synchronises)
  if (nk == 0) return h->sp.end(e, SPAN_ADDS, st, "asmmap add");
  if (!h->k_first.ensure(nk * 4) || !h->k_last.ensure(nk * 4) || !h->blk_head.ensure(nk * 4) || !h->blk_before.ensure((nk + 1) * 8))
    return eng_fail(e, SIMMR_ENOMEM, "asmmap add: allocation failed (%llu kept runs)", (unsigned long long)nk);
  const uint32_t kept_grid = grid_for(h, nk, AMAP_WG, 32);
  hipLaunchKernelGGL(k_amap_kept_runs, dim3(run_grid), dim3(AMAP_WG), 0, st, h->kept.as<const uint32_t>(), h->kept_before.as<const uint64_t>(),
                     h->r_first.as<const uint32_t>(), h->r_last.as<const uint32_t>(), nr, nk, h->k_first.as<uint32_t>(), h->k_last.as<uint32_t>());
  // the blocks
  hipLaunchKernelGGL(k_amap_block_heads, dim3(kept_grid), dim3(AMAP_WG), 0, st, h->hits(), h->k_first.as<const uint32_t>(), h->k_last.as<const uint32_t>(), nk,
                     (uint64_t)h->band, h->blk_head.as<uint32_t>());
  uint64_t nb = 0;
  if (int rc = eng_scan_u32(e, h->blk_head.as<const uint32_t>(), nk, h->blk_before.as<uint64_t>(), &nb)) return rc;  // (synchronises)
  const uint64_t b0 = h->n_blocks, b_want = b0 + nb;
  if (b_want >= 0xffffffffull) return eng_fail(e, SIMMR_ERANGE, "simmr_asmmap_add takes fewer than 2^32 - 1 blocks since the plan (%llu given)", (unsigned long long)b_want);
  if (b_want > h->block_cap) {
    const uint64_t cap = b_want + b_want / 2, held = h->block_cap;
    for (DevBuf& col : h->b_col) room = room && grow_zero(&col, cap, held, 4, st);
    room = room && grow_zero(&h->b_dfirst, cap, held, 8, st) && grow_zero(&h->b_dlast, cap, held, 8, st);
    if (!room) return eng_fail(e, SIMMR_ENOMEM, "asmmap add: allocation failed (%llu blocks)", (unsigned long long)b_want);
    h->block_cap = cap;
  }
  h->n_blocks = b_want;
  const AmapBlocks B = h->blocks();
  HIP_TRY(e, hipMemsetAsync(B.p_start + b0, 0xff, nb * 4, st));  // (hits and p_end are zero: grow_zero, and nothing wrote behind n_blocks)
  hipLaunchKernelGGL(k_amap_blocks, dim3(kept_grid), dim3(AMAP_WG), 0, st, h->hits(), h->k_first.as<const uint32_t>(), h->k_last.as<const uint32_t>(),
                     h->blk_head.as<const uint32_t>(), h->blk_before.as<const uint64_t>(), nk, nb, b0, c0, h->k, B);
  hipLaunchKernelGGL(k_amap_block_span, dim3(hit_grid), dim3(AMAP_WG), 0, st, h->hits(), h->run_head.as<const uint32_t>(), h->run_before.as<const uint64_t>(),
                     h->kept.as<const uint32_t>(), h->kept_before.as<const uint64_t>(), h->blk_head.as<const uint32_t>(), h->blk_before.as<const uint64_t>(), nh, nb,
                     b0, h->k, B);
  hipLaunchKernelGGL(k_amap_joins, dim3(grid_for(h, nb, AMAP_WG, 32)), dim3(AMAP_WG), 0, st, B, b0, nb, h->t_genome.as<const uint32_t>(), (uint64_t)h->band,
                     (uint64_t)h->relocation, h->contigs());
  return h->sp.end(e, SPAN_ADDS, st, "asmmap add");
}

int simmr_asmmap_read(simmr_asmmap* h, simmr_asmmap_counts* counts, uint64_t* by_genome_host) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_asmmap_read called before simmr_asmmap_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t g1 = std::max(h->n_genomes, 1u);
  if (!h->g_blocks.ensure(g1 * 3 * 8) || !h->g_truth.ensure(g1 * 2 * 8)) return eng_fail(e, SIMMR_ENOMEM, "asmmap read: allocation failed");
  HIP_TRY(e, hipMemsetAsync(h->g_blocks.p, 0, g1 * 3 * 8, st));
  // what the reductions make starts over: blocks .. breaks_local, and the contig classes .. misassembled_bases
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + AM_BLOCKS, 0, (AM_COUNT - AM_BLOCKS) * 8, st));
  if (h->planned && h->n_blocks > 0)
    hipLaunchKernelGGL(k_amap_reduce_blocks, dim3(grid_for(h, h->n_blocks, AMAP_WG, 16)), dim3(AMAP_WG), 0, st, h->blocks(), h->n_blocks,
                       h->t_genome.as<const uint32_t>(), h->n_genomes, h->g_blocks.as<unsigned long long>(), h->counts_p());
  if (h->planned && h->n_contigs > 0)
    hipLaunchKernelGGL(k_amap_reduce_contigs, dim3(grid_for(h, h->n_contigs, AMAP_WG, 16)), dim3(AMAP_WG), 0, st, h->contigs(), h->n_contigs, h->counts_p());
  std::vector<uint64_t> host(AM_COUNT), gb(g1 * 3), gt(g1 * 2, 0);
  uint64_t cur = 0;
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(host.data(), h->counts.p, AM_COUNT * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(gb.data(), h->g_blocks.p, g1 * 3 * 8, hipMemcpyDeviceToHost, st));
  if (h->planned) HIP_TRY(e, hipMemcpyAsync(gt.data(), h->g_truth.p, g1 * 2 * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&cur, h->cursor.p, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "asmmap read")) return rc;
  if (errw & ASM_ERR_TRUTH) return eng_fail(e, SIMMR_EINVAL, "a malformed truth text: %s", MALFORMED_TRUTH);
  if (errw & ASM_ERR_CAND) return eng_fail(e, SIMMR_EINVAL, "a malformed candidate text: %s", MALFORMED_CAND);
  host[AM_T_KMERS] = std::min(cur, h->occ_cap);
  host[AM_T_ANCHORS] = h->planned ? h->n_anchors : 0;
  host[AM_T_REPEATS] = h->planned ? h->n_repeats : 0;
  host[AM_RUNS] = h->planned ? h->n_runs : 0;
  if (!h->planned) std::fill(host.begin() + AM_RECORDS, host.end(), 0ull);  // (a truth add has dropped the plan: the candidate side went with it)
  if (counts) std::memcpy(counts, host.data(), sizeof(*counts));
  if (by_genome_host)
    for (uint32_t g = 0; g < h->n_genomes; g++) {
      uint64_t* row = by_genome_host + (uint64_t)g * AMAP_GENOME_COLS;
      row[0] = gt[g * 2];
      row[1] = gt[g * 2 + 1];
      row[2] = gb[g * 3];
      row[3] = gb[g * 3 + 1];
      row[4] = gb[g * 3 + 2];
    }
  return SIMMR_OK;
}

int simmr_asmmap_anchors(simmr_asmmap* h, uint64_t* key_dev, uint32_t* t_dev, uint32_t* p_dev, uint32_t* o_dev, uint64_t capacity) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_asmmap_anchors called without a simmr_asmmap_truth_plan in force");
  if (capacity < h->n_anchors)
    return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu anchors", (unsigned long long)capacity, (unsigned long long)h->n_anchors);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t n = h->n_anchors;
  if (n > 0) {
    if (key_dev) HIP_TRY(e, hipMemcpyAsync(key_dev, h->a_key.p, n * 8, hipMemcpyDeviceToDevice, st));
    if (t_dev) HIP_TRY(e, hipMemcpyAsync(t_dev, h->a_t.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (p_dev) HIP_TRY(e, hipMemcpyAsync(p_dev, h->a_p.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (o_dev) HIP_TRY(e, hipMemcpyAsync(o_dev, h->a_o.p, n * 4, hipMemcpyDeviceToDevice, st));
  }
  return sync_check(e, "asmmap anchors");
}

int simmr_asmmap_blocks(simmr_asmmap* h, uint32_t* const* cols_dev, uint64_t capacity, uint64_t* n_blocks) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_asmmap_blocks called without a simmr_asmmap_truth_plan in force");
  const uint64_t n = h->n_blocks;
  if (n_blocks) *n_blocks = n;
  if (capacity < n) return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu blocks", (unsigned long long)capacity, (unsigned long long)n);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (n > 0 && cols_dev)
    for (uint32_t j = 0; j < SIMMR_ASMMAP_BLOCK_COLS; j++)
      if (cols_dev[j]) HIP_TRY(e, hipMemcpyAsync(cols_dev[j], h->b_col[j].p, n * 4, hipMemcpyDeviceToDevice, st));
  return sync_check(e, "asmmap blocks");
}

int simmr_asmmap_contigs(simmr_asmmap* h, uint64_t* length_dev, uint32_t* hits_dev, uint32_t* blocks_dev, uint32_t* first_block_dev, uint64_t* block_bases_dev,
                         uint32_t* worst_join_dev, uint64_t capacity, uint64_t* n_contigs) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_asmmap_contigs called without a simmr_asmmap_truth_plan in force");
  const uint64_t n = h->n_contigs;
  if (n_contigs) *n_contigs = n;
  if (capacity < n) return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu contigs", (unsigned long long)capacity, (unsigned long long)n);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (n > 0) {
    if (length_dev) HIP_TRY(e, hipMemcpyAsync(length_dev, h->c_len.p, n * 8, hipMemcpyDeviceToDevice, st));
    if (hits_dev) HIP_TRY(e, hipMemcpyAsync(hits_dev, h->c_hits.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (blocks_dev) HIP_TRY(e, hipMemcpyAsync(blocks_dev, h->c_blocks.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (block_bases_dev) HIP_TRY(e, hipMemcpyAsync(block_bases_dev, h->c_bb.p, n * 8, hipMemcpyDeviceToDevice, st));
    if (first_block_dev || worst_join_dev)
      hipLaunchKernelGGL(k_amap_contig_cols, dim3(grid_for(h, n, AMAP_WG, 32)), dim3(AMAP_WG), 0, st, h->c_first.as<const uint32_t>(), h->c_worst.as<const uint32_t>(), n,
                         first_block_dev, worst_join_dev);
  }
  return sync_check(e, "asmmap contigs");
}

int simmr_last_asmmap_ms(simmr_asmmap* h, float* ms) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!ms) return eng_fail(e, SIMMR_EINVAL, "simmr_last_asmmap_ms: NULL ms");
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_asmmap_reset yet");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  return h->sp.last_ms(e, "asmmap", ms);
}

}  // extern "C"
