// asmeval.hip — an assembler's contigs scored against the gold-standard assembly (include/simmr_hip.h: simmr_asmeval_*): the
// entry points over asmeval_kernels.hip, on the scaffold of scorer_host.hpp.  The front (asmeval_front.hpp) is this unit's and
// asmmap.hip's; the scan of the run heads is the engine's (eng_scan_u32).
//
// The front of an add of either side (enqueue_front) only enqueues and sizes everything from n_bytes: a line per two bytes, a
// record per line, a base per byte.  index (count) -> scan -> index (write) -> lines (count) -> chunks -> lines (write) -> pack.
// truth_add:  the front, the genome of every record, the roll; the occurrences (key, genome row) are appended through a cursor,
//             their columns sized from the bytes of every truth add since the reset (a column that has to grow keeps what it holds).
// truth_plan: reads the cursor, copies the keys to the sort's ping, sorts over 2k bits, marks the run heads, scans them (which
//             synchronises and gives the number of entries), compacts the runs into the entries, builds the prefix table
//             (bits = min(24, bit length of the entries)) and empties the candidate side.
// add:        the front, then SYNCHRONISES for the add's bases and records (room for the contig columns), the roll with the lookups,
//             synchronises for the number of vote pairs, sorts them, scans their heads (synchronises) and takes every contig's top.
// Time: the adds' span and the plan's, and the sort inside the plan in a `Spans` of one beside them (it counts once, inside the
// plan).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "host_support.hpp"
#include "asmeval_kernels.hip"
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

struct simmr_asmeval {
  simmr_engine* e = nullptr;
  DeviceNames genomes;
  uint32_t n_genomes = 0, k = 0, plain_search = 0;
  // the front of one add: the line index, the lines, the planes (asmeval_front.hpp)
  AsmFront front;
  DevBuf rec_row;
  // the truth: the occurrences as appended, the sort's buffers, the entries
  DevBuf u_key, u_row, head, before;
  PairSort occ_sort, pair_sort;  // the plan's over the occurrences, an add's over its vote pairs (their keys go into pair_sort.key[0])
  DevBuf e_key, e_start, e_genome, e_mult, hits, table;
  DevBuf cursor;   // [0] occurrences, [1] the vote pairs of the add
  DevBuf counts;   // AC_COUNT words
  DevBuf word;     // the error word
  // the candidates: the contig columns, the pairs and votes of one add, the per-genome table of a read
  DevBuf c_len, c_kmers, c_found, c_shared, c_top, c_voted, p_count, v_key, v_count, g_table;
  uint64_t occ_cap = 0;     // occurrences the truth adds since the reset may have appended
  uint64_t n_entries = 0, n_contigs = 0, contig_cap = 0;
  uint32_t table_bits = 0;
  bool reset_once = false, planned = false;
  FoldedSpans<SPAN_COUNT> sp;
  Spans<1> sort_sp;  // the sort inside the last plan: beside the spans above, so that it counts once, inside the plan

  MevNames names() const { return genomes.names(n_genomes); }
  AsmLines lines() const { return front.lines(); }
  AsmPlane plane() const { return front.plane(); }
  AsmContigs contigs() const {
    return AsmContigs{c_len.as<uint64_t>(), c_kmers.as<uint32_t>(), c_found.as<uint32_t>(), c_shared.as<uint32_t>(), c_top.as<unsigned long long>(),
                      c_voted.as<uint32_t>()};
  }
  AsmEntries entries() const {
    const uint32_t bits = plain_search ? 0u : table_bits;
    return AsmEntries{e_key.as<const uint64_t>(), e_genome.as<const uint32_t>(), table.as<const uint32_t>(), (uint32_t)n_entries, bits, 2u * k - bits};
  }
  unsigned long long* counts_p() const { return counts.as<unsigned long long>(); }
  unsigned long long* cursor_p() const { return cursor.as<unsigned long long>(); }
};

namespace {

int check_add(simmr_asmeval* h, const uint8_t* text, uint64_t n_bytes, const char* who) {
  return check_add_text(h->e, h->reset_once, text, n_bytes, SIMMR_ASMEVAL_MAX_BYTES, who, "simmr_asmeval_reset", "cut the text in front of a header");
}

// text[0, n_bytes) (n_bytes > 0) to the object's line entries and planes; `truth`: the side whose counts and error bit it feeds
int enqueue_front(simmr_asmeval* h, const uint8_t* text, uint64_t n_bytes, hipStream_t st, bool truth, MevText* W) {
  simmr_engine* e = h->e;
  if (!h->front.ensure(n_bytes)) return eng_fail(e, SIMMR_ENOMEM, "asmeval: allocation failed for %llu bytes of text", (unsigned long long)n_bytes);
  const AsmFrontSums sums{h->counts_p(), (uint32_t)(truth ? AC_T_RECORDS : AC_RECORDS), (uint32_t)(truth ? AC_T_BASES : AC_BASES),
                          (uint32_t)(truth ? AC_T_INVALID : AC_INVALID), h->word.as<uint32_t>(), truth ? ASM_ERR_TRUTH : ASM_ERR_CAND};
  asm_front_launch(e, st, text, n_bytes, h->front.bufs(), sums, W);
  return SIMMR_OK;
}

}  // namespace

namespace simmr {

void asm_front_launch(simmr_engine* e, hipStream_t st, const uint8_t* text, uint64_t n_bytes, const AsmFrontBufs& B, const AsmFrontSums& S, MevText* W) {
  const uint64_t n_tiles = (n_bytes + FSAM_TILE - 1) / FSAM_TILE, line_cap = n_bytes / 2 + 1, chunk_cap = line_cap / ASM_CHUNK + 1;
  const uint64_t word_cap = n_bytes / ASM_WORD + 1;
  const uint32_t tile_grid = grid_for(e, n_tiles, 1, 16), line_grid = grid_for(e, chunk_cap, 1, 8), word_grid = grid_for(e, word_cap, ASM_WG, 16);
  hipLaunchKernelGGL(k_asm_index, dim3(tile_grid), dim3(FSAM_WG), 0, st, text, n_bytes, n_tiles, B.tile_sum, (const uint64_t*)nullptr, (uint32_t*)nullptr, 0ull);
  hipLaunchKernelGGL(k_asm_scan, dim3(1), dim3(256), 0, st, (const uint64_t*)B.tile_sum, B.tile_prefix, n_tiles);
  hipLaunchKernelGGL(k_asm_index, dim3(tile_grid), dim3(FSAM_WG), 0, st, text, n_bytes, n_tiles, B.tile_sum, (const uint64_t*)B.tile_prefix, B.starts, line_cap);
  *W = MevText{text, n_bytes, (const uint64_t*)B.tile_prefix + n_tiles, (const uint32_t*)B.starts};
  hipLaunchKernelGGL(k_asm_lines, dim3(line_grid), dim3(ASM_WG), 0, st, *W, line_cap, B.chunk_sum, (const uint64_t*)nullptr, B.lines, S.err, S.err_bit);
  hipLaunchKernelGGL(k_asm_chunks, dim3(1), dim3(256), 0, st, W->n_lines, line_cap, (const uint64_t*)B.chunk_sum, B.chunk_prefix, B.lines, S.counts, S.records_at,
                     S.bases_at);
  hipLaunchKernelGGL(k_asm_lines, dim3(line_grid), dim3(ASM_WG), 0, st, *W, line_cap, B.chunk_sum, (const uint64_t*)B.chunk_prefix, B.lines, S.err, S.err_bit);
  hipLaunchKernelGGL(k_asm_pack, dim3(word_grid), dim3(ASM_WG), 0, st, *W, B.lines, B.code, B.valid, S.counts, S.invalid_at);
}

void asm_front_genomes(simmr_engine* e, hipStream_t st, const MevText& W, const AsmLines& L, const MevNames& N, uint32_t* rec_row, uint32_t* err) {
  hipLaunchKernelGGL(k_asm_genomes, dim3(grid_for(e, W.n_bytes / 2 + 1, ASM_WG_RECS, 8)), dim3(ASM_WG), 0, st, W, L, N, rec_row, err);
}

}  // namespace simmr

extern "C" {

int simmr_asmeval_create(simmr_engine* e, simmr_asmeval** out) { return scorer_create(e, out, "simmr_asmeval_create"); }

void simmr_asmeval_destroy(simmr_asmeval* h) { scorer_destroy(h); }

int simmr_asmeval_reset(simmr_asmeval* h, const simmr_asmeval_config* cfg) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!cfg || (cfg->n_genomes > 0 && !cfg->genome)) return eng_fail(e, SIMMR_EINVAL, "simmr_asmeval_reset: NULL argument");
  if (cfg->k < 15u || cfg->k > 31u || cfg->k % 2u == 0u) return eng_fail(e, SIMMR_EINVAL, "simmr_asmeval_reset: k = %u (an odd number of 15 to 31)", cfg->k);
  if (cfg->n_genomes > (1u << 24) - 1u) return eng_fail(e, SIMMR_ERANGE, "simmr_asmeval_reset: %u genome names (fewer than 2^24)", cfg->n_genomes);
  SortedNames sorted;
  if (int rc = sorted_names(e, cfg->genome, cfg->n_genomes, SAM_RNAME_MAX, rname_legal, "genome name", nullptr, &sorted)) return rc;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = sync_check(e, "asmeval reset")) return rc;
  h->planned = false;
  h->reset_once = false;
  h->sort_sp.invalidate_from(0);
  if (int rc = h->sp.reset(e)) return rc;
  if (int rc = h->sort_sp.create_missing(e)) return rc;
  if (!h->genomes.room(sorted) || !h->cursor.ensure(16) || !h->counts.ensure(AC_COUNT * 8) || !h->word.ensure(16))
    return eng_fail(e, SIMMR_ENOMEM, "asmeval reset: allocation failed");
  hipStream_t st = eng_stream(e);
  if (int rc = h->genomes.upload(e, sorted, st)) return rc;
  HIP_TRY(e, hipMemsetAsync(h->cursor.p, 0, 16, st));
  HIP_TRY(e, hipMemsetAsync(h->counts.p, 0, AC_COUNT * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->word.p, 0, 16, st));
  if (int rc = sync_check(e, "asmeval reset")) return rc;  // (the uploads read host vectors that end here)
  h->n_genomes = cfg->n_genomes;
  h->k = cfg->k;
  h->plain_search = cfg->plain_search ? 1u : 0u;
  h->occ_cap = 0;
  h->n_entries = 0;
  h->n_contigs = 0;
  h->table_bits = 0;
  h->reset_once = true;
  return SIMMR_OK;
}

int simmr_asmeval_truth_add(simmr_asmeval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_asmeval_truth_add")) return rc;
  h->planned = false;
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t cap = h->occ_cap + n_bytes, held = h->occ_cap;
  if (!h->u_key.grow_keep(cap * 8, held * 8, st) || !h->u_row.grow_keep(cap * 4, held * 4, st) || !h->rec_row.ensure((n_bytes / 2 + 1) * 4))
    return eng_fail(e, SIMMR_ENOMEM, "asmeval truth: allocation failed for %llu k-mer occurrences", (unsigned long long)cap);
  h->occ_cap = cap;
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  if (int rc = enqueue_front(h, text, n_bytes, st, true, &W)) return rc;
  asm_front_genomes(e, st, W, h->lines(), h->names(), h->rec_row.as<uint32_t>(), h->word.as<uint32_t>());
  hipLaunchKernelGGL(k_asm_roll_truth, dim3(grid_for(e, n_bytes / ASM_WORD + 1, ASM_WG, 32)), dim3(ASM_WG), 0, st, h->plane(), h->k,
                     h->rec_row.as<const uint32_t>(), h->u_key.as<uint64_t>(), h->u_row.as<uint32_t>(), cap, h->cursor_p());
  return h->sp.end(e, SPAN_ADDS, st, "asmeval truth add");
}

int simmr_asmeval_truth_plan(simmr_asmeval* h, uint64_t* n_entries) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_asmeval_truth_plan called before simmr_asmeval_reset");
  h->planned = false;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  uint64_t cur = 0;
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(&cur, h->cursor.p, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "asmeval truth adds")) return rc;
  if (int rc = h->sp.fold(e, "asmeval")) return rc;
  if (errw & ASM_ERR_TRUTH) return eng_fail(e, SIMMR_EINVAL, "a malformed truth text: %s", MALFORMED_TRUTH);
  const uint64_t n = std::min(cur, h->occ_cap);
  if (n >= (1ull << 31))
    return eng_fail(e, SIMMR_ERANGE, "simmr_asmeval_truth_plan takes fewer than 2^31 k-mer occurrences (%llu given)", (unsigned long long)n);
  const uint64_t n1 = std::max<uint64_t>(n, 1);
  if (!h->occ_sort.room(n1) || !h->head.ensure(n1 * 4) || !h->before.ensure((n1 + 1) * 8))
    return eng_fail(e, SIMMR_ENOMEM, "asmeval truth plan: allocation failed (%llu k-mer occurrences)", (unsigned long long)n);
  if (int rc = h->sp.begin(e, SPAN_PLAN, st)) return rc;
  // the candidate side starts over
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + AC_RECORDS, 0, (AC_COUNT - AC_RECORDS) * 8, st));
  h->n_contigs = 0;
  h->contig_cap = 0;
  h->sort_sp.invalidate_from(0);
  uint64_t nd = 0;
  const uint64_t* skey = h->occ_sort.key[0].as<const uint64_t>();
  const uint32_t* sidx = nullptr;
  const uint32_t grid = grid_for(e, n1, 256, 32);
  if (n > 0) {
    HIP_TRY(e, hipMemcpyAsync(h->occ_sort.key[0].p, h->u_key.p, n * 8, hipMemcpyDeviceToDevice, st));
    HIP_TRY(e, h->sort_sp.begin(0, st));
    const PairSort::Sorted by_key = h->occ_sort.sort(st, n, 2u * h->k);
    HIP_TRY(e, h->sort_sp.end(0, st));
    h->sort_sp.mark(0);
    skey = by_key.keys;
    sidx = by_key.perm;
    hipLaunchKernelGGL(k_asm_heads, dim3(grid), dim3(256), 0, st, skey, n, h->head.as<uint32_t>());
    if (int rc = eng_scan_u32(e, h->head.as<const uint32_t>(), n, h->before.as<uint64_t>(), &nd)) return rc;  // (synchronises)
  }
  const uint64_t nd1 = std::max<uint64_t>(nd, 1);
  const uint32_t bits = std::min(TABLE_MAX_BITS, bits_of(nd));
  if (!h->e_key.ensure(nd1 * 8) || !h->e_start.ensure((nd1 + 1) * 4) || !h->e_genome.ensure(nd1 * 4) || !h->e_mult.ensure(nd1 * 4) || !h->hits.ensure(nd1 * 4) ||
      !h->table.ensure(((1ull << bits) + 1) * 4))
    return eng_fail(e, SIMMR_ENOMEM, "asmeval truth plan: allocation failed (%llu entries)", (unsigned long long)nd);
  HIP_TRY(e, hipMemsetAsync(h->e_genome.p, 0, nd1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->hits.p, 0, nd1 * 4, st));
  if (nd > 0) {
    hipLaunchKernelGGL(k_asm_entries, dim3(grid), dim3(256), 0, st, skey, sidx, h->u_row.as<const uint32_t>(), h->before.as<const uint64_t>(), n, nd,
                       h->n_genomes, h->e_key.as<uint64_t>(), h->e_start.as<uint32_t>(), h->e_genome.as<uint32_t>());
    hipLaunchKernelGGL(k_asm_mult, dim3(grid_for(e, nd, 256, 32)), dim3(256), 0, st, h->e_start.as<const uint32_t>(), nd, h->e_mult.as<uint32_t>());
    hipLaunchKernelGGL(k_asm_table, dim3(grid_for(e, (1ull << bits) + 1, 256, 32)), dim3(256), 0, st, h->e_key.as<const uint64_t>(), (uint32_t)nd, bits,
                       2u * h->k - bits, h->table.as<uint32_t>());
  }
  if (int rc = h->sp.end(e, SPAN_PLAN, st, "asmeval truth plan")) return rc;
  if (int rc = sync_check(e, "asmeval truth plan")) return rc;
  h->n_entries = nd;
  h->table_bits = nd > 0 ? bits : 0u;
  h->planned = true;
  if (int rc = h->sp.fold(e, "asmeval")) return rc;
  if (n_entries) *n_entries = nd;
  return SIMMR_OK;
}

int simmr_asmeval_add(simmr_asmeval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_asmeval_add")) return rc;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_asmeval_add called without a simmr_asmeval_truth_plan in force");
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  if (int rc = enqueue_front(h, text, n_bytes, st, false, &W)) return rc;
  uint32_t tot[3] = {0, 0, 0};
  HIP_TRY(e, hipMemcpyAsync(tot, h->front.tot.p, 12, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "asmeval add")) return rc;
  const uint64_t n_bases = tot[1], n_rec = tot[2], c0 = h->n_contigs, want = c0 + n_rec;
  if (want >= (1ull << 31)) return eng_fail(e, SIMMR_ERANGE, "simmr_asmeval_add takes fewer than 2^31 contigs since the plan (%llu given)", (unsigned long long)want);
  const uint64_t pair_cap = std::max<uint64_t>(n_bases, 1);
  bool room = true;
  if (want > h->contig_cap) {
    const uint64_t cap = want + want / 2, held = h->contig_cap;
    room = grow_zero(&h->c_len, cap, held, 8, st) && grow_zero(&h->c_top, cap, held, 8, st) && grow_zero(&h->c_kmers, cap, held, 4, st) &&
           grow_zero(&h->c_found, cap, held, 4, st) && grow_zero(&h->c_shared, cap, held, 4, st) && grow_zero(&h->c_voted, cap, held, 4, st);
    if (room) h->contig_cap = cap;
  }
  room = room && h->pair_sort.key[0].ensure(pair_cap * 8) && h->p_count.ensure(pair_cap * 4);
  if (!room) return eng_fail(e, SIMMR_ENOMEM, "asmeval add: allocation failed (%llu contigs, %llu bases)", (unsigned long long)want, (unsigned long long)n_bases);
  h->n_contigs = want;
  HIP_TRY(e, hipMemsetAsync(h->cursor_p() + 1, 0, 8, st));
  if (n_rec > 0)
    hipLaunchKernelGGL(k_asm_contig_len, dim3(grid_for(e, n_rec, 256, 32)), dim3(256), 0, st, h->front.rec_start.as<const uint32_t>(), (uint32_t)n_rec, c0,
                       h->c_len.as<uint64_t>());
  if (n_bases > 0)
    hipLaunchKernelGGL(k_asm_roll_cand, dim3(grid_for(e, n_bases / ASM_WORD + 1, ASM_WG, 32)), dim3(ASM_WG), 0, st, h->plane(), h->k, h->entries(), h->n_genomes,
                       h->hits.as<uint32_t>(), c0, h->contigs(), h->pair_sort.key[0].as<uint64_t>(), h->p_count.as<uint32_t>(), pair_cap, h->cursor_p() + 1);
  uint64_t np = 0;
  HIP_TRY(e, hipMemcpyAsync(&np, h->cursor_p() + 1, 8, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "asmeval add")) return rc;
  np = std::min(np, pair_cap);
  if (np > 0) {
    if (!h->pair_sort.room(np) || !h->head.ensure(np * 4) || !h->before.ensure((np + 1) * 8))
      return eng_fail(e, SIMMR_ENOMEM, "asmeval add: allocation failed (%llu vote pairs)", (unsigned long long)np);
    const PairSort::Sorted by_pair = h->pair_sort.sort(st, np, bits_of((want - 1) << ASM_GENOME_BITS | 0xffffffull));  // (24 bits at least: a permutation)
    const uint32_t grid = grid_for(e, np, 256, 32);
    hipLaunchKernelGGL(k_asm_heads, dim3(grid), dim3(256), 0, st, by_pair.keys, np, h->head.as<uint32_t>());
    uint64_t nv = 0;
    if (int rc = eng_scan_u32(e, h->head.as<const uint32_t>(), np, h->before.as<uint64_t>(), &nv)) return rc;  // (synchronises)
    if (!h->v_key.ensure(nv * 8) || !h->v_count.ensure(nv * 4)) return eng_fail(e, SIMMR_ENOMEM, "asmeval add: allocation failed (%llu votes)", (unsigned long long)nv);
    HIP_TRY(e, hipMemsetAsync(h->v_count.p, 0, nv * 4, st));
    hipLaunchKernelGGL(k_asm_vote_sum, dim3(grid), dim3(256), 0, st, by_pair.keys, by_pair.perm, h->p_count.as<const uint32_t>(),
                       h->before.as<const uint64_t>(), np, nv, h->v_key.as<uint64_t>(), h->v_count.as<uint32_t>());
    hipLaunchKernelGGL(k_asm_vote_top, dim3(grid_for(e, nv, 256, 32)), dim3(256), 0, st, h->v_key.as<const uint64_t>(), h->v_count.as<const uint32_t>(), nv, want,
                       h->contigs());
  }
  return h->sp.end(e, SPAN_ADDS, st, "asmeval add");
}

int simmr_asmeval_read(simmr_asmeval* h, simmr_asmeval_counts* counts, uint64_t* by_genome_host) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_asmeval_read called before simmr_asmeval_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t rows = (uint64_t)h->n_genomes + 1, table_words = rows * ASM_GENOME_COLS;
  if (!h->g_table.ensure(table_words * 8)) return eng_fail(e, SIMMR_ENOMEM, "asmeval read: allocation failed");
  HIP_TRY(e, hipMemsetAsync(h->g_table.p, 0, table_words * 8, st));
  // what the contig reduction makes starts over: records and bases (the adds' own sums are the same numbers), kmers .. shared_only
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + AC_RECORDS, 0, 2 * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + AC_KMERS, 0, (AC_COUNT - AC_KMERS) * 8, st));
  if (h->planned && h->n_entries > 0)
    hipLaunchKernelGGL(k_asm_reduce_entries, dim3(grid_for(e, h->n_entries, 256, 16)), dim3(256), 0, st, h->e_genome.as<const uint32_t>(),
                       h->e_mult.as<const uint32_t>(), h->hits.as<const uint32_t>(), h->n_entries, (uint32_t)rows, h->g_table.as<unsigned long long>());
  if (h->planned && h->n_contigs > 0)
    hipLaunchKernelGGL(k_asm_reduce_contigs, dim3(grid_for(e, h->n_contigs, 256, 16)), dim3(256), 0, st, h->contigs(), h->n_contigs, h->n_genomes,
                       h->g_table.as<unsigned long long>(), h->counts_p());
  std::vector<uint64_t> host(AC_COUNT), table(table_words);
  uint64_t cur = 0;
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(host.data(), h->counts.p, AC_COUNT * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(table.data(), h->g_table.p, table_words * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&cur, h->cursor.p, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "asmeval read")) return rc;
  if (errw & ASM_ERR_TRUTH) return eng_fail(e, SIMMR_EINVAL, "a malformed truth text: %s", MALFORMED_TRUTH);
  if (errw & ASM_ERR_CAND) return eng_fail(e, SIMMR_EINVAL, "a malformed candidate text: %s", MALFORMED_CAND);
  host[AC_T_KMERS] = std::min(cur, h->occ_cap);
  host[AC_T_DISTINCT] = h->planned ? h->n_entries : 0;
  host[AC_T_SHARED_DISTINCT] = table[(rows - 1) * ASM_GENOME_COLS];
  host[AC_NOVEL] = host[AC_KMERS] - host[AC_FOUND];
  if (counts) std::memcpy(counts, host.data(), sizeof(*counts));
  if (by_genome_host) std::memcpy(by_genome_host, table.data(), table_words * 8);
  return SIMMR_OK;
}

int simmr_asmeval_emit(simmr_asmeval* h, uint64_t* key_dev, uint32_t* genome_dev, uint32_t* mult_dev, uint32_t* hits_dev, uint64_t capacity) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_asmeval_emit called without a simmr_asmeval_truth_plan in force");
  if (capacity < h->n_entries)
    return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu truth entries", (unsigned long long)capacity, (unsigned long long)h->n_entries);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (h->n_entries > 0) {
    if (key_dev) HIP_TRY(e, hipMemcpyAsync(key_dev, h->e_key.p, h->n_entries * 8, hipMemcpyDeviceToDevice, st));
    if (genome_dev) HIP_TRY(e, hipMemcpyAsync(genome_dev, h->e_genome.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
    if (mult_dev) HIP_TRY(e, hipMemcpyAsync(mult_dev, h->e_mult.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
    if (hits_dev) HIP_TRY(e, hipMemcpyAsync(hits_dev, h->hits.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
  }
  return sync_check(e, "asmeval emit");
}

int simmr_asmeval_contigs(simmr_asmeval* h, uint64_t* length_dev, uint32_t* kmers_dev, uint32_t* found_dev, uint32_t* shared_dev, uint32_t* top_genome_dev,
                          uint32_t* top_kmers_dev, uint64_t capacity, uint64_t* n_contigs) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_asmeval_contigs called without a simmr_asmeval_truth_plan in force");
  const uint64_t n = h->n_contigs;
  if (n_contigs) *n_contigs = n;
  if (capacity < n) return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu contigs", (unsigned long long)capacity, (unsigned long long)n);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (n > 0) {
    if (length_dev) HIP_TRY(e, hipMemcpyAsync(length_dev, h->c_len.p, n * 8, hipMemcpyDeviceToDevice, st));
    if (kmers_dev) HIP_TRY(e, hipMemcpyAsync(kmers_dev, h->c_kmers.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (found_dev) HIP_TRY(e, hipMemcpyAsync(found_dev, h->c_found.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (shared_dev) HIP_TRY(e, hipMemcpyAsync(shared_dev, h->c_shared.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (top_genome_dev || top_kmers_dev)
      hipLaunchKernelGGL(k_asm_contig_cols, dim3(grid_for(e, n, 256, 32)), dim3(256), 0, st, h->c_top.as<const unsigned long long>(), n, top_genome_dev,
                         top_kmers_dev);
  }
  return sync_check(e, "asmeval contigs");
}

int simmr_last_asmeval_ms(simmr_asmeval* h, float* ms, float* plan_sort_ms) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!ms) return eng_fail(e, SIMMR_EINVAL, "simmr_last_asmeval_ms: NULL ms");
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_asmeval_reset yet");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = h->sp.last_ms(e, "asmeval", ms)) return rc;
  if (plan_sort_ms)
    if (int rc = h->sort_sp.total_ms(e, "asmeval", plan_sort_ms)) return rc;
  return SIMMR_OK;
}

}  // extern "C"
