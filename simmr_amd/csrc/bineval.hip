// bineval.hip — a binner's contig bins scored against each contig's true genome (include/simmr_hip.h: simmr_bineval_*): the entry
// points over bineval_kernels.hip, on the scaffold of scorer_host.hpp.  The scans of the flags are the engine's (eng_scan_u32).
//
// The front of an add of either side (enqueue_front) only enqueues and sizes everything from n_bytes: a line per two bytes.
// index (count) -> scan -> index (write) -> lines -> chunks -> write.
// truth_add:  the front, the rows (name, hash, length) behind the truth's device cursor, the genome of every row.  The columns and
//             the name pool are sized from the bytes of every truth add since the reset (a column that has to grow keeps what it holds).
// truth_plan: reads the cursor, writes the truncated hashes to the sort's ping, sorts over hash_bits bits (none: the identity order), looks
//             for equal names inside the runs, and empties the candidate side.
// add:        the front, the lines and the chunks, then SYNCHRONISES for the add's records and bin-name bytes (room for the record
//             columns), then the write pass with the lookups, the first record and the records of every truth contig.
// read:       sorts the records by the bin name's hash, finds the representatives, scans their flags (synchronises: the bins),
//             assigns, sorts the cell keys, scans the cell heads (synchronises: the cells), sums, and makes the tables.
// Time: the adds' span, the plan's and the read's, and the sort inside the plan in a `Spans` of one beside them (it counts once,
// inside the plan).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "host_support.hpp"
#include "bineval_kernels.hip"
#include "sam_names.hpp"
#include "scorer_host.hpp"

using namespace simmr;

namespace {

// Workgroups a CU of every grid: beyond them the workgroups loop.  Small, so that a text of a few MB takes every kernel past one trip.
constexpr uint32_t WGS_PER_CU = 2;

enum { SPAN_ADDS = 0, SPAN_PLAN = 1, SPAN_READ = 2, SPAN_COUNT = 3 };

const char* const MALFORMED_TRUTH =
    "a line with fewer than eight fields, a field 2 to 7 that is no number, a contig name that is empty, longer than 254 bytes or holds a blank or a "
    "control byte, or a genome that is neither '.' nor among the genome names";
const char* const MALFORMED_DUP = "a contig name occurs twice";
const char* const MALFORMED_CAND = "a record without a second field, or a name that is empty, longer than 254 bytes or holds a blank or a control byte";

}  // namespace

struct simmr_bineval {
  simmr_engine* e = nullptr;
  DeviceNames genomes;
  uint32_t n_genomes = 0, hash_bits = 64;
  // the front of one add: the line index, the chunks, the totals
  LineIndex line_index;
  DevBuf info, chunk_sum, chunk_prefix, tot, rec_field;
  // the truth: the rows as appended, the order of the plan, the assignment
  DevBuf t_pool, t_off, t_len, t_hash, t_length, t_genome, t_first, t_records, t_bin;
  PairSort truth_sort, rec_sort, cell_sort;  // the plan's over the truth's hashes, a read's over the records' hashes and over the cell keys
  DevBuf head, before;
  DevBuf cursor;   // [0] the truth's rows, [1] the bytes of their names
  DevBuf unknown;  // the records of contigs that are not in the truth
  DevBuf counts;   // BC_COUNT words
  DevBuf word;     // the error word
  // the candidate records since the plan
  DevBuf b_pool, b_off, b_len, b_hash, r_contig;
  // a read: the records' order, the bin rows, the cells, the tables
  DevBuf rep, flag, rec_bin;
  DevBuf q_contigs, q_real, q_bases, q_none, q_first, q_top_genome, q_top_bases;
  DevBuf c_bin, c_genome, c_contigs, c_bases;
  DevBuf g_table, best_bin;
  uint64_t row_cap = 0, pool_cap = 0;   // what the truth adds since the reset may have appended
  uint64_t n_truth = 0, n_records = 0, n_bpool = 0, n_bins = 0, n_cells = 0;
  PairSort::Sorted truth_order{};  // the truth's rows in the plan's order
  bool reset_once = false, planned = false, read_holds = false;
  FoldedSpans<SPAN_COUNT> sp;
  Spans<1> sort_sp;

  uint64_t mask() const { return hash_bits >= 64u ? ~0ull : (1ull << hash_bits) - 1ull; }
  MevNames names() const { return genomes.names(n_genomes); }
  BinNames truth_names() const { return BinNames{t_pool.as<uint8_t>(), t_off.as<uint64_t>(), t_len.as<uint32_t>(), t_hash.as<uint64_t>(), row_cap, pool_cap}; }
  BinNames bin_names(uint64_t rows, uint64_t bytes) const {
    return BinNames{b_pool.as<uint8_t>(), b_off.as<uint64_t>(), b_len.as<uint32_t>(), b_hash.as<uint64_t>(), rows, bytes};
  }
  BinIndex index() const {
    return BinIndex{truth_order.keys, truth_order.perm, t_pool.as<const uint8_t>(), t_off.as<const uint64_t>(),
                    t_len.as<const uint32_t>(), t_hash.as<const uint64_t>(), (uint32_t)n_truth, mask()};
  }
  BinBins bins() const {
    return BinBins{q_contigs.as<uint32_t>(), q_real.as<uint32_t>(), q_bases.as<uint64_t>(), q_none.as<uint64_t>(), q_first.as<uint32_t>(),
                   q_top_genome.as<uint32_t>(), q_top_bases.as<unsigned long long>()};
  }
  BinCells cells() const { return BinCells{c_bin.as<uint32_t>(), c_genome.as<uint32_t>(), c_contigs.as<uint32_t>(), c_bases.as<unsigned long long>()}; }
  unsigned long long* counts_p() const { return counts.as<unsigned long long>(); }
};

namespace {

int check_add(simmr_bineval* h, const uint8_t* text, uint64_t n_bytes, const char* who) {
  return check_add_text(h->e, h->reset_once, text, n_bytes, SIMMR_BINEVAL_MAX_BYTES, who, "simmr_bineval_reset", "cut the text behind a line end");
}

// text[0, n_bytes) (n_bytes > 0) to the object's line index
int enqueue_front(simmr_bineval* h, const uint8_t* text, uint64_t n_bytes, hipStream_t st, MevText* W, uint64_t* line_cap_out) {
  simmr_engine* e = h->e;
  const uint64_t n_tiles = (n_bytes + FSAM_TILE - 1) / FSAM_TILE, line_cap = n_bytes / 2 + 1, chunk_cap = line_cap / BIN_CHUNK + 1;
  bool room = h->line_index.room(n_tiles, line_cap) && h->chunk_sum.ensure(chunk_cap * 8) && h->chunk_prefix.ensure((chunk_cap + 1) * 8) &&
              h->tot.ensure(sizeof(BinTot)) && h->rec_field.ensure(line_cap * 8) && h->info.ensure(line_cap * 16);
  if (!room) return eng_fail(e, SIMMR_ENOMEM, "bineval: allocation failed for %llu bytes of text", (unsigned long long)n_bytes);
  h->line_index.enqueue(st, k_bin_index, k_bin_scan, text, n_bytes, FSAM_TILE, grid_for(e, n_tiles, 1, WGS_PER_CU), line_cap, W);
  *line_cap_out = line_cap;
  return SIMMR_OK;
}

// the n pairs (S->key[0][i], i) in the order of the low `bits` bits of the keys.  No bits: the identity, written out.
PairSort::Sorted sort_by(simmr_bineval* h, hipStream_t st, PairSort* S, uint64_t n, uint32_t bits) {
  if (bits > 0u) return S->sort(st, n, bits);
  hipLaunchKernelGGL(k_bin_iota, dim3(grid_for(h->e, n, 256, WGS_PER_CU)), dim3(256), 0, st, S->idx[0].as<uint32_t>(), n);
  return PairSort::Sorted{S->key[0].as<const uint64_t>(), S->idx[0].as<const uint32_t>()};
}

int malformed(simmr_bineval* h, uint32_t errw) {
  simmr_engine* e = h->e;
  if (errw & BIN_ERR_TRUTH) return eng_fail(e, SIMMR_EINVAL, "a malformed truth text: %s", MALFORMED_TRUTH);
  if (errw & BIN_ERR_DUP) return eng_fail(e, SIMMR_EINVAL, "a malformed truth text: %s", MALFORMED_DUP);
  if (errw & BIN_ERR_CAND) return eng_fail(e, SIMMR_EINVAL, "a malformed candidate text: %s", MALFORMED_CAND);
  return SIMMR_OK;
}

// what simmr_bineval_bins, _cells and _contigs share: the state, the count, the capacity
int emit_check(simmr_bineval* h, const char* who, const char* what, uint64_t n, uint64_t capacity, uint64_t* n_out) {
  simmr_engine* e = h->e;
  if (!h->planned || !h->read_holds) return eng_fail(e, SIMMR_ESTATE, "%s called without a simmr_bineval_read since the plan and the last add", who);
  if (n_out) *n_out = n;
  if (capacity < n) return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu %s", (unsigned long long)capacity, (unsigned long long)n, what);
  return SIMMR_OK;
}

}  // namespace

extern "C" {

int simmr_bineval_create(simmr_engine* e, simmr_bineval** out) { return scorer_create(e, out, "simmr_bineval_create"); }

void simmr_bineval_destroy(simmr_bineval* h) { scorer_destroy(h); }

int simmr_bineval_reset(simmr_bineval* h, const simmr_bineval_config* cfg) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!cfg || (cfg->n_genomes > 0 && !cfg->genome)) return eng_fail(e, SIMMR_EINVAL, "simmr_bineval_reset: NULL argument");
  if (cfg->hash_bits > 64u) return eng_fail(e, SIMMR_EINVAL, "simmr_bineval_reset: hash_bits = %u (0 to 64)", cfg->hash_bits);
  if (cfg->n_genomes > (1u << 24) - 1u) return eng_fail(e, SIMMR_ERANGE, "simmr_bineval_reset: %u genome names (fewer than 2^24)", cfg->n_genomes);
  SortedNames sorted;
  if (int rc = sorted_names(e, cfg->genome, cfg->n_genomes, SAM_RNAME_MAX, rname_legal, "genome name", nullptr, &sorted)) return rc;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = sync_check(e, "bineval reset")) return rc;
  h->planned = false;
  h->read_holds = false;
  h->reset_once = false;
  h->sort_sp.invalidate_from(0);
  if (int rc = h->sp.reset(e)) return rc;
  if (int rc = h->sort_sp.create_missing(e)) return rc;
  if (!h->genomes.room(sorted) || !h->cursor.ensure(16) || !h->unknown.ensure(8) ||
      !h->counts.ensure(BC_COUNT * 8) || !h->word.ensure(16))
    return eng_fail(e, SIMMR_ENOMEM, "bineval reset: allocation failed");
  hipStream_t st = eng_stream(e);
  if (int rc = h->genomes.upload(e, sorted, st)) return rc;
  HIP_TRY(e, hipMemsetAsync(h->cursor.p, 0, 16, st));
  HIP_TRY(e, hipMemsetAsync(h->unknown.p, 0, 8, st));
  HIP_TRY(e, hipMemsetAsync(h->counts.p, 0, BC_COUNT * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->word.p, 0, 16, st));
  if (int rc = sync_check(e, "bineval reset")) return rc;  // (the uploads read host vectors that end here)
  h->n_genomes = cfg->n_genomes;
  h->hash_bits = cfg->hash_bits;
  h->row_cap = h->pool_cap = 0;
  h->n_truth = h->n_records = h->n_bpool = h->n_bins = h->n_cells = 0;
  h->reset_once = true;
  return SIMMR_OK;
}

int simmr_bineval_truth_add(simmr_bineval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_bineval_truth_add")) return rc;
  h->planned = false;
  h->read_holds = false;
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  // a record has eight fields and seven tabs: 16 bytes with its line end, 15 without one at the text's end
  const uint64_t rows = h->row_cap + n_bytes / 15 + 1, held = h->row_cap, bytes = h->pool_cap + n_bytes;
  if (!h->t_pool.grow_keep(bytes, h->pool_cap, st) || !h->t_off.grow_keep(rows * 8, held * 8, st) || !h->t_len.grow_keep(rows * 4, held * 4, st) ||
      !h->t_hash.grow_keep(rows * 8, held * 8, st) || !h->t_length.grow_keep(rows * 8, held * 8, st) || !h->t_genome.grow_keep(rows * 4, held * 4, st))
    return eng_fail(e, SIMMR_ENOMEM, "bineval truth: allocation failed for %llu contigs", (unsigned long long)rows);
  h->row_cap = rows;
  h->pool_cap = bytes;
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  uint64_t line_cap = 0;
  if (int rc = enqueue_front(h, text, n_bytes, st, &W, &line_cap)) return rc;
  const uint32_t line_grid = grid_for(e, line_cap / BIN_CHUNK + 1, 1, WGS_PER_CU);
  BinTot* tot = h->tot.as<BinTot>();
  hipLaunchKernelGGL(k_bin_lines, dim3(line_grid), dim3(BIN_WG), 0, st, W, line_cap, 1u, h->chunk_sum.as<uint64_t>(), h->info.as<uint4>(),
                     h->word.as<uint32_t>(), BIN_ERR_TRUTH);
  hipLaunchKernelGGL(k_bin_chunks, dim3(1), dim3(256), 0, st, W.n_lines, line_cap, h->chunk_sum.as<const uint64_t>(), h->chunk_prefix.as<uint64_t>(), tot,
                     h->cursor.as<unsigned long long>(), 0ull, 0ull);
  hipLaunchKernelGGL(k_bin_truth_write, dim3(line_grid), dim3(BIN_WG), 0, st, W, line_cap, h->chunk_prefix.as<const uint64_t>(), h->info.as<const uint4>(),
                     (const BinTot*)tot, h->truth_names(), h->t_length.as<uint64_t>(), h->rec_field.as<uint32_t>());
  hipLaunchKernelGGL(k_bin_genomes, dim3(grid_for(e, line_cap, BIN_WG_RECS, WGS_PER_CU)), dim3(BIN_WG), 0, st, W, (const BinTot*)tot, h->rec_field.as<const uint32_t>(),
                     h->names(), h->t_genome.as<uint32_t>(), h->row_cap, h->word.as<uint32_t>());
  return h->sp.end(e, SPAN_ADDS, st, "bineval truth add");
}

int simmr_bineval_truth_plan(simmr_bineval* h, uint64_t* n_contigs) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_bineval_truth_plan called before simmr_bineval_reset");
  h->planned = false;
  h->read_holds = false;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  uint64_t cur = 0;
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(&cur, h->cursor.p, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "bineval truth adds")) return rc;
  if (int rc = h->sp.fold(e, "bineval")) return rc;
  if (errw & BIN_ERR_TRUTH) return malformed(h, BIN_ERR_TRUTH);
  const uint64_t n = std::min(cur, h->row_cap);
  if (n >= (1ull << 31)) return eng_fail(e, SIMMR_ERANGE, "simmr_bineval_truth_plan takes fewer than 2^31 truth contigs (%llu given)", (unsigned long long)n);
  const uint64_t n1 = std::max<uint64_t>(n, 1);
  if (!h->truth_sort.room(n1) || !h->head.ensure(n1 * 4) || !h->before.ensure((n1 + 1) * 8) || !h->t_first.ensure(n1 * 4) || !h->t_records.ensure(n1 * 4) || !h->t_bin.ensure(n1 * 4))
    return eng_fail(e, SIMMR_ENOMEM, "bineval truth plan: allocation failed (%llu contigs)", (unsigned long long)n);
  if (int rc = h->sp.begin(e, SPAN_PLAN, st)) return rc;
  // the candidate side starts over
  HIP_TRY(e, hipMemsetAsync(h->unknown.p, 0, 8, st));
  HIP_TRY(e, hipMemsetAsync(h->t_first.p, 0xff, n1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->t_records.p, 0, n1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->word.p, 0, 4, st));  // (the truth is well-formed here; a duplicate is looked for below)
  h->n_records = h->n_bpool = h->n_bins = h->n_cells = 0;
  h->n_truth = n;
  h->truth_order = PairSort::Sorted{h->truth_sort.key[0].as<const uint64_t>(), h->truth_sort.idx[0].as<const uint32_t>()};
  h->sort_sp.invalidate_from(0);
  if (n > 0) {
    hipLaunchKernelGGL(k_bin_keys, dim3(grid_for(e, n, 256, WGS_PER_CU)), dim3(256), 0, st, h->t_hash.as<const uint64_t>(), h->mask(), n, h->truth_sort.key[0].as<uint64_t>());
    HIP_TRY(e, h->sort_sp.begin(0, st));
    h->truth_order = sort_by(h, st, &h->truth_sort, n, h->hash_bits);
    HIP_TRY(e, h->sort_sp.end(0, st));
    h->sort_sp.mark(0);
    hipLaunchKernelGGL(k_bin_truth_dups, dim3(grid_for(e, n, 256, WGS_PER_CU)), dim3(256), 0, st, h->index(), h->word.as<uint32_t>());
  }
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = h->sp.end(e, SPAN_PLAN, st, "bineval truth plan")) return rc;
  if (int rc = sync_check(e, "bineval truth plan")) return rc;
  if (int rc = h->sp.fold(e, "bineval")) return rc;
  if (errw & BIN_ERR_DUP) return malformed(h, BIN_ERR_DUP);
  h->planned = true;
  if (n_contigs) *n_contigs = n;
  return SIMMR_OK;
}

int simmr_bineval_add(simmr_bineval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_bineval_add")) return rc;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_bineval_add called without a simmr_bineval_truth_plan in force");
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  uint64_t line_cap = 0;
  if (int rc = enqueue_front(h, text, n_bytes, st, &W, &line_cap)) return rc;
  const uint32_t line_grid = grid_for(e, line_cap / BIN_CHUNK + 1, 1, WGS_PER_CU);
  BinTot* tot = h->tot.as<BinTot>();
  hipLaunchKernelGGL(k_bin_lines, dim3(line_grid), dim3(BIN_WG), 0, st, W, line_cap, 0u, h->chunk_sum.as<uint64_t>(), h->info.as<uint4>(),
                     h->word.as<uint32_t>(), BIN_ERR_CAND);
  hipLaunchKernelGGL(k_bin_chunks, dim3(1), dim3(256), 0, st, W.n_lines, line_cap, h->chunk_sum.as<const uint64_t>(), h->chunk_prefix.as<uint64_t>(), tot,
                     (unsigned long long*)nullptr, (unsigned long long)h->n_records, (unsigned long long)h->n_bpool);
  BinTot got{};
  HIP_TRY(e, hipMemcpyAsync(&got, tot, sizeof(got), hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "bineval add")) return rc;
  const uint64_t held = h->n_records, want = held + got.records, bytes = h->n_bpool + got.bytes;
  if (want >= (1ull << 31)) {
    (void)h->sp.end(e, SPAN_ADDS, st, "bineval add");  // (the front of the refused add has run: the span closes behind it)
    return eng_fail(e, SIMMR_ERANGE, "simmr_bineval_add takes fewer than 2^31 records since the plan (%llu given)", (unsigned long long)want);
  }
  if (!h->b_pool.grow_keep(std::max<uint64_t>(bytes, 1), h->n_bpool, st) || !h->b_off.grow_keep(want * 8 + 8, held * 8, st) ||
      !h->b_len.grow_keep(want * 4 + 4, held * 4, st) || !h->b_hash.grow_keep(want * 8 + 8, held * 8, st) || !h->r_contig.grow_keep(want * 4 + 4, held * 4, st))
  {
    (void)h->sp.end(e, SPAN_ADDS, st, "bineval add");
    return eng_fail(e, SIMMR_ENOMEM, "bineval add: allocation failed (%llu records)", (unsigned long long)want);
  }
  h->read_holds = false;
  if (got.records > 0)
    hipLaunchKernelGGL(k_bin_cand_write, dim3(line_grid), dim3(BIN_WG), 0, st, W, line_cap, h->chunk_prefix.as<const uint64_t>(), h->info.as<const uint4>(),
                       (const BinTot*)tot, h->index(), h->bin_names(want, bytes), h->r_contig.as<uint32_t>(), h->t_first.as<uint32_t>(),
                       h->t_records.as<uint32_t>(), h->unknown.as<unsigned long long>());
  h->n_records = want;
  h->n_bpool = bytes;
  return h->sp.end(e, SPAN_ADDS, st, "bineval add");
}

int simmr_bineval_read(simmr_bineval* h, simmr_bineval_counts* counts, uint64_t* by_genome_host) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_bineval_read called before simmr_bineval_reset");
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_bineval_read called without a simmr_bineval_truth_plan in force");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  h->read_holds = false;
  const uint64_t n = h->n_records, nt = h->n_truth, rows = (uint64_t)h->n_genomes + 1, table_words = rows * BIN_GENOME_COLS;
  if (!h->g_table.ensure(table_words * 8) || !h->best_bin.ensure(rows * 4)) return eng_fail(e, SIMMR_ENOMEM, "bineval read: allocation failed");
  if (int rc = h->sp.fold(e, "bineval")) return rc;  // (the adds' span ends here)
  if (int rc = h->sp.begin(e, SPAN_READ, st)) return rc;
  HIP_TRY(e, hipMemsetAsync(h->counts.p, 0, BC_COUNT * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->g_table.p, 0, table_words * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->best_bin.p, 0xff, rows * 4, st));
  // the bin rows
  uint64_t n_bins = 0;
  if (n > 0) {
    if (!h->rec_sort.room(n) || !h->head.ensure(n * 4) || !h->before.ensure((n + 1) * 8) || !h->rep.ensure(n * 4) || !h->flag.ensure(n * 4) || !h->rec_bin.ensure(n * 4))
      return eng_fail(e, SIMMR_ENOMEM, "bineval read: allocation failed (%llu records)", (unsigned long long)n);
    hipLaunchKernelGGL(k_bin_keys, dim3(grid_for(e, n, 256, WGS_PER_CU)), dim3(256), 0, st, h->b_hash.as<const uint64_t>(), h->mask(), n, h->rec_sort.key[0].as<uint64_t>());
    HIP_TRY(e, hipMemsetAsync(h->flag.p, 0, n * 4, st));
    const PairSort::Sorted by_hash = sort_by(h, st, &h->rec_sort, n, h->hash_bits);
    hipLaunchKernelGGL(k_bin_reps, dim3(grid_for(e, n, 256, WGS_PER_CU)), dim3(256), 0, st, by_hash.keys, by_hash.perm,
                       h->r_contig.as<const uint32_t>(), h->bin_names(n, h->n_bpool), n, h->rep.as<uint32_t>(), h->flag.as<uint32_t>());
    if (int rc = eng_scan_u32(e, h->flag.as<const uint32_t>(), n, h->before.as<uint64_t>(), &n_bins)) return rc;  // (synchronises)
  }
  const uint64_t nb1 = std::max<uint64_t>(n_bins, 1);
  if (!h->q_contigs.ensure(nb1 * 4) || !h->q_real.ensure(nb1 * 4) || !h->q_bases.ensure(nb1 * 8) || !h->q_none.ensure(nb1 * 8) || !h->q_first.ensure(nb1 * 4) ||
      !h->q_top_genome.ensure(nb1 * 4) || !h->q_top_bases.ensure(nb1 * 8))
    return eng_fail(e, SIMMR_ENOMEM, "bineval read: allocation failed (%llu bins)", (unsigned long long)n_bins);
  HIP_TRY(e, hipMemsetAsync(h->q_contigs.p, 0, nb1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->q_real.p, 0, nb1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->q_bases.p, 0, nb1 * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->q_none.p, 0, nb1 * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->q_top_genome.p, 0xff, nb1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->q_top_bases.p, 0, nb1 * 8, st));
  if (n > 0)
    hipLaunchKernelGGL(k_bin_rows, dim3(grid_for(e, n, 256, WGS_PER_CU)), dim3(256), 0, st, h->rep.as<const uint32_t>(), h->before.as<const uint64_t>(), n, n_bins,
                       h->rec_bin.as<uint32_t>(), h->q_first.as<uint32_t>());
  // the cells
  uint64_t n_cells = 0;
  PairSort::Sorted by_cell{};
  if (nt > 0) {
    if (!h->cell_sort.room(nt) || !h->head.ensure(nt * 4) || !h->before.ensure((nt + 1) * 8))
      return eng_fail(e, SIMMR_ENOMEM, "bineval read: allocation failed (%llu contigs)", (unsigned long long)nt);
    const uint32_t grid = grid_for(e, nt, 256, WGS_PER_CU);
    hipLaunchKernelGGL(k_bin_assign, dim3(grid), dim3(256), 0, st, h->t_first.as<const uint32_t>(), h->t_genome.as<const uint32_t>(),
                       h->rec_bin.as<const uint32_t>(), nt, n, (uint32_t)n_bins, h->cell_sort.key[0].as<uint64_t>(), h->t_bin.as<uint32_t>());
    by_cell = sort_by(h, st, &h->cell_sort, nt, BIN_GENOME_BITS + bits_of(n_bins));
    hipLaunchKernelGGL(k_bin_cell_heads, dim3(grid), dim3(256), 0, st, by_cell.keys, nt, (uint32_t)n_bins, h->head.as<uint32_t>());
    if (int rc = eng_scan_u32(e, h->head.as<const uint32_t>(), nt, h->before.as<uint64_t>(), &n_cells)) return rc;  // (synchronises)
  }
  const uint64_t nc1 = std::max<uint64_t>(n_cells, 1);
  if (!h->c_bin.ensure(nc1 * 4) || !h->c_genome.ensure(nc1 * 4) || !h->c_contigs.ensure(nc1 * 4) || !h->c_bases.ensure(nc1 * 8))
    return eng_fail(e, SIMMR_ENOMEM, "bineval read: allocation failed (%llu cells)", (unsigned long long)n_cells);
  HIP_TRY(e, hipMemsetAsync(h->c_contigs.p, 0, nc1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->c_bases.p, 0, nc1 * 8, st));
  if (nt > 0) {
    const uint32_t grid = grid_for(e, nt, 256, WGS_PER_CU);
    if (n_cells > 0)
      hipLaunchKernelGGL(k_bin_cell_sum, dim3(grid), dim3(256), 0, st, by_cell.keys, by_cell.perm,
                         h->t_length.as<const uint64_t>(), h->before.as<const uint64_t>(), nt, (uint32_t)n_bins, n_cells, h->cells());
    hipLaunchKernelGGL(k_bin_truth_rows, dim3(grid), dim3(256), 0, st, h->t_genome.as<const uint32_t>(), h->t_length.as<const uint64_t>(),
                       h->t_first.as<const uint32_t>(), h->t_records.as<const uint32_t>(), nt, h->n_genomes, h->g_table.as<unsigned long long>(), h->counts_p());
  }
  if (n_cells > 0)
    for (uint32_t phase = 0; phase < 2u; phase++)
      hipLaunchKernelGGL(k_bin_cell_tables, dim3(grid_for(e, n_cells, 256, WGS_PER_CU)), dim3(256), 0, st, h->cells(), n_cells, (uint32_t)n_bins, h->n_genomes, phase,
                         h->bins(), h->g_table.as<unsigned long long>(), h->best_bin.as<uint32_t>(), h->counts_p());
  if (n_bins > 0 || h->n_genomes > 0)
    hipLaunchKernelGGL(k_bin_finish, dim3(grid_for(e, std::max<uint64_t>(n_bins, h->n_genomes), 256, WGS_PER_CU)), dim3(256), 0, st, h->bins(), (uint32_t)n_bins,
                       h->n_genomes, h->best_bin.as<const uint32_t>(), h->g_table.as<unsigned long long>(), h->counts_p());
  std::vector<uint64_t> host(BC_COUNT), table(table_words);
  uint64_t unknown = 0;
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(host.data(), h->counts.p, BC_COUNT * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(table.data(), h->g_table.p, table_words * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&unknown, h->unknown.p, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = h->sp.end(e, SPAN_READ, st, "bineval read")) return rc;
  if (int rc = sync_check(e, "bineval read")) return rc;
  if (int rc = h->sp.fold(e, "bineval")) return rc;
  if (errw) return malformed(h, errw);
  h->n_bins = n_bins;
  h->n_cells = n_cells;
  h->read_holds = true;
  host[BC_T_RECORDS] = nt;
  host[BC_RECORDS] = n;
  host[BC_UNKNOWN] = unknown;
  host[BC_BINS] = n_bins;
  host[BC_CELLS] = n_cells;
  if (counts) std::memcpy(counts, host.data(), sizeof(*counts));
  if (by_genome_host) std::memcpy(by_genome_host, table.data(), table_words * 8);
  return SIMMR_OK;
}

int simmr_bineval_bins(simmr_bineval* h, uint32_t* contigs_dev, uint64_t* bases_dev, uint64_t* none_bases_dev, uint32_t* first_record_dev,
                       uint32_t* top_genome_dev, uint64_t* top_bases_dev, uint64_t capacity, uint64_t* n_bins) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  const uint64_t n = h->n_bins;
  if (int rc = emit_check(h, "simmr_bineval_bins", "bins", n, capacity, n_bins)) return rc;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (n > 0) {
    if (contigs_dev) HIP_TRY(e, hipMemcpyAsync(contigs_dev, h->q_contigs.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (bases_dev) HIP_TRY(e, hipMemcpyAsync(bases_dev, h->q_bases.p, n * 8, hipMemcpyDeviceToDevice, st));
    if (none_bases_dev) HIP_TRY(e, hipMemcpyAsync(none_bases_dev, h->q_none.p, n * 8, hipMemcpyDeviceToDevice, st));
    if (first_record_dev) HIP_TRY(e, hipMemcpyAsync(first_record_dev, h->q_first.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (top_genome_dev) HIP_TRY(e, hipMemcpyAsync(top_genome_dev, h->q_top_genome.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (top_bases_dev) HIP_TRY(e, hipMemcpyAsync(top_bases_dev, h->q_top_bases.p, n * 8, hipMemcpyDeviceToDevice, st));
  }
  return sync_check(e, "bineval bins");
}

int simmr_bineval_cells(simmr_bineval* h, uint32_t* bin_dev, uint32_t* genome_dev, uint32_t* contigs_dev, uint64_t* bases_dev, uint64_t capacity,
                        uint64_t* n_cells) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  const uint64_t n = h->n_cells;
  if (int rc = emit_check(h, "simmr_bineval_cells", "cells", n, capacity, n_cells)) return rc;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (n > 0) {
    if (bin_dev) HIP_TRY(e, hipMemcpyAsync(bin_dev, h->c_bin.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (genome_dev) HIP_TRY(e, hipMemcpyAsync(genome_dev, h->c_genome.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (contigs_dev) HIP_TRY(e, hipMemcpyAsync(contigs_dev, h->c_contigs.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (bases_dev) HIP_TRY(e, hipMemcpyAsync(bases_dev, h->c_bases.p, n * 8, hipMemcpyDeviceToDevice, st));
  }
  return sync_check(e, "bineval cells");
}

int simmr_bineval_contigs(simmr_bineval* h, uint32_t* genome_dev, uint64_t* length_dev, uint32_t* bin_dev, uint32_t* records_dev, uint64_t capacity,
                          uint64_t* n_contigs) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  const uint64_t n = h->n_truth;
  if (int rc = emit_check(h, "simmr_bineval_contigs", "contigs", n, capacity, n_contigs)) return rc;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (n > 0) {
    if (genome_dev) HIP_TRY(e, hipMemcpyAsync(genome_dev, h->t_genome.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (length_dev) HIP_TRY(e, hipMemcpyAsync(length_dev, h->t_length.p, n * 8, hipMemcpyDeviceToDevice, st));
    if (bin_dev) HIP_TRY(e, hipMemcpyAsync(bin_dev, h->t_bin.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (records_dev) HIP_TRY(e, hipMemcpyAsync(records_dev, h->t_records.p, n * 4, hipMemcpyDeviceToDevice, st));
  }
  return sync_check(e, "bineval contigs");
}

int simmr_last_bineval_ms(simmr_bineval* h, float* ms, float* plan_sort_ms) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!ms) return eng_fail(e, SIMMR_EINVAL, "simmr_last_bineval_ms: NULL ms");
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_bineval_reset yet");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = h->sp.last_ms(e, "bineval", ms)) return rc;
  if (plan_sort_ms)
    if (int rc = h->sort_sp.total_ms(e, "bineval", plan_sort_ms)) return rc;
  return SIMMR_OK;
}

}  // extern "C"
