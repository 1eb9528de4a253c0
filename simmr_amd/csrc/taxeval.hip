// taxeval.hip — a read classifier's calls scored against each read's true genome (include/simmr_hip.h: simmr_taxeval_*): the entry
// points over taxeval_kernels.hip, on the scaffold of scorer_host.hpp.  The genome ids are a name table under a rule of their own
// (no tab, no newline), and its order carries the taxids along.  The sort is sam_sort.hip's (samsort_sort_pairs), called directly:
// the reset's over the taxids and the plan's over the ids share their histograms.
//
// reset:      uploads the arrays; sort -> nodes (parents and genomes to rows) -> lineage (depths and the ancestor table); reads the
//             error word.  A refusal leaves the object without a tree.
// truth_add:  enqueue-only, so nothing is sized from what the text holds.  The index buffers are sized from n_bytes (a line start
//             per two bytes), the line columns from the bytes of every truth add since the reset (a line per TXE_MIN_LINE bytes);
//             a column that has to grow keeps what it holds.  index (count) -> scan -> index (write) -> truth.
// truth_plan: reads the cursor and the largest id, sorts the lines by id, heads (count) -> scan -> heads (write) collapses equal
//             ids into entries; zeroes the candidate side.
// add:        index (count) -> scan -> index (write) -> record.
// taxa:       zeroes the clade sums, rollup, copies the columns out: the direct counts are only read.
// Time: the adds' span and the plan's.  The reset's work is not timed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "host_support.hpp"
#include "taxeval_kernels.hip"
#include "scorer_host.hpp"

using namespace simmr;

namespace {

enum { SPAN_ADDS = 0, SPAN_PLAN = 1, SPAN_COUNT = 2 };
constexpr size_t COUNT_WORDS = TC_COUNT + 2u * TXE_RANK_WORDS;  // the counts, by_rank, reads_by_rank
constexpr uint64_t MAX_NODES = 1ull << 26, MAX_GENOMES = 1ull << 24;

const char* const TRUTH_MALFORMED = "fewer than 3 fields, a read_id that is no number of 1 to 18 digits, a pair that is not 0, 1 or 2, or a genome_id outside the genomes";
const char* const CAND_MALFORMED = "fewer than 3 fields, a first field that is neither C nor U, or a third field that is neither 1 to 10 digits below 2^32 nor "
                                   "text that ends in '(taxid <such digits>)'";

}  // namespace

struct simmr_taxeval {
  simmr_engine* e = nullptr;
  // the genomes: the names sorted in a blob, and per name row the node of its taxid
  DeviceNames genomes;
  DevBuf g_taxid, g_node;
  uint32_t n_names = 0;
  // the tree: what the caller gave (in_*), the sorted taxids (t_key[t_cur]), and per sorted node its columns
  DevBuf in_parent, in_rank, t_key[2], t_idx[2], taxid, prow, rank, depth, anc;
  DevBuf direct, clade;  // [3][n_nodes] each: true, called, both
  DevBuf look;           // the ten words of k_txe_look
  const uint64_t* tkey = nullptr;
  uint32_t n_nodes = 0;
  LineIndex index;  // of one add
  // the truth: the lines as appended (u_*), the sort's buffers, and the entries in id order (e_*)
  DevBuf u_id, u_genome, key[2], idx[2], hist, digit_total, head_sum, head_prefix, e_id, e_genome, e_mates;
  DevBuf cursor;   // [0] lines, [1] the largest id
  DevBuf counts;   // TC_COUNT words, then by_rank's 40 and reads_by_rank's 40
  DevBuf word;     // the error word
  DevBuf seen, hits;
  uint64_t line_cap = 0;   // lines the truth adds since the reset may have appended
  uint64_t n_entries = 0;
  bool reset_once = false, planned = false;
  FoldedSpans<SPAN_COUNT> sp;

  MevNames names() const { return genomes.names(n_names); }
  TxeTree tree() const { return TxeTree{tkey, prow.as<const uint32_t>(), depth.as<const uint32_t>(), anc.as<const uint32_t>(), n_nodes}; }
  TxeEntries entries() const { return TxeEntries{e_id.as<const uint64_t>(), e_genome.as<const uint32_t>(), e_mates.as<const uint32_t>(), n_entries}; }
  unsigned long long* counts_p() const { return counts.as<unsigned long long>(); }
};

namespace {

int check_add(simmr_taxeval* h, const uint8_t* text, uint64_t n_bytes, const char* who) {
  return check_add_text(h->e, h->reset_once, text, n_bytes, SIMMR_FIT_SAM_MAX_BYTES, who, "simmr_taxeval_reset", "cut the text at a line's end");
}

// the line index of text[0, n_bytes) into the object's buffers (n_bytes > 0)
int enqueue_index(simmr_taxeval* h, const uint8_t* text, uint64_t n_bytes, hipStream_t st, MevText* W, uint32_t* rec_grid) {
  simmr_engine* e = h->e;
  const uint64_t n_tiles = (n_bytes + FSAM_TILE - 1) / FSAM_TILE, start_cap = n_bytes / 2 + 1;
  if (!h->index.room(n_tiles, start_cap))
    return eng_fail(e, SIMMR_ENOMEM, "taxeval line index: allocation failed for %llu bytes of text", (unsigned long long)n_bytes);
  const uint32_t cus = (uint32_t)std::max(eng_cu_count(e), 1);
  *rec_grid = (uint32_t)std::min<uint64_t>(n_bytes / (TXE_WG_RECS * TXE_MIN_LINE) + 1, (uint64_t)cus * 8u);
  h->index.enqueue(st, k_txe_index, k_txe_scan, text, n_bytes, FSAM_TILE, (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)cus * 16u), start_cap, W);
  return SIMMR_OK;
}

int tree_refusal(simmr_engine* e, uint32_t errw) {
  const char* what = errw & TXE_ERR_TAXID0 ? "a node has the taxid 0, which stands for 'unclassified'"
                     : errw & TXE_ERR_TWICE ? "a taxid is given twice"
                     : errw & TXE_ERR_RANK ? "a rank code above 8"
                     : errw & TXE_ERR_PARENT ? "a parent that is no node"
                     : errw & TXE_ERR_DEPTH ? "a walk to the root takes more than 255 steps (a cycle, or a tree deeper than that)"
                     : errw & TXE_ERR_RANK_TWICE ? "a lineage holds one rank twice"
                                                 : "a genome's taxid is no node";
  return eng_fail(e, SIMMR_EINVAL, "simmr_taxeval_reset: %s", what);
}

}  // namespace

extern "C" {

int simmr_taxeval_create(simmr_engine* e, simmr_taxeval** out) { return scorer_create(e, out, "simmr_taxeval_create"); }

void simmr_taxeval_destroy(simmr_taxeval* h) { scorer_destroy(h); }

int simmr_taxeval_reset(simmr_taxeval* h, const simmr_taxeval_config* cfg) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!cfg || (cfg->n_nodes > 0 && (!cfg->taxid || !cfg->parent || !cfg->rank)) || (cfg->n_genomes > 0 && (!cfg->genome_id || !cfg->genome_taxid)))
    return eng_fail(e, SIMMR_EINVAL, "simmr_taxeval_reset: NULL argument");
  if (cfg->n_nodes > MAX_NODES) return eng_fail(e, SIMMR_ERANGE, "simmr_taxeval_reset: %llu nodes (at most 2^26)", (unsigned long long)cfg->n_nodes);
  if (cfg->n_genomes > MAX_GENOMES) return eng_fail(e, SIMMR_ERANGE, "simmr_taxeval_reset: %llu genomes (at most 2^24)", (unsigned long long)cfg->n_genomes);
  const uint32_t n = (uint32_t)cfg->n_nodes, ng = (uint32_t)cfg->n_genomes;
  SortedNames sorted;  // (bytewise, a prefix first, as mev_compare orders them)
  if (int rc = sorted_names(e, cfg->genome_id, ng, SAM_RNAME_MAX, [](const char* s, size_t) { return !std::strchr(s, '\t') && !std::strchr(s, '\n'); },
                            "genome id", "holds a tab or a newline", &sorted))
    return rc;
  std::vector<uint32_t> gtax(std::max(ng, 1u), 0u);
  for (uint32_t i = 0; i < ng; i++) gtax[i] = cfg->genome_taxid[sorted.order[i]];
  uint32_t largest = 0;
  for (uint32_t i = 0; i < n; i++) largest = std::max(largest, cfg->taxid[i]);
  std::vector<uint64_t> keys(std::max(n, 1u), 0ull);
  for (uint32_t i = 0; i < n; i++) keys[i] = cfg->taxid[i];

  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = sync_check(e, "taxeval reset")) return rc;
  h->planned = false;
  h->reset_once = false;
  h->n_entries = 0;
  h->line_cap = 0;
  if (int rc = h->sp.reset(e)) return rc;
  const uint64_t n1 = std::max(n, 1u), g1 = std::max(ng, 1u), n_tiles = (n + SAMSORT_PAIRS_TILE - 1) / SAMSORT_PAIRS_TILE;
  bool room = h->genomes.room(sorted) && h->g_taxid.ensure(g1 * 4) && h->g_node.ensure(g1 * 4) &&
              h->cursor.ensure(16) && h->counts.ensure(COUNT_WORDS * 8) && h->word.ensure(16) && h->look.ensure(64) && h->in_parent.ensure(n1 * 4) &&
              h->in_rank.ensure(n1) && h->rank.ensure(n1) && h->anc.ensure(n1 * TXE_RANKS * 4) && h->direct.ensure(n1 * 24) && h->clade.ensure(n1 * 24) &&
              h->hist.ensure(std::max<uint64_t>(n_tiles, 1) * SAMSORT_PAIRS_DIGITS * 4) && h->digit_total.ensure(SAMSORT_PAIRS_DIGITS * 4);
  for (DevBuf* b : {&h->t_key[0], &h->t_key[1]}) room = room && b->ensure(n1 * 8);
  for (DevBuf* b : {&h->t_idx[0], &h->t_idx[1], &h->taxid, &h->prow, &h->depth}) room = room && b->ensure(n1 * 4);
  if (!room) return eng_fail(e, SIMMR_ENOMEM, "taxeval reset: allocation failed (%u nodes, %u genomes)", n, ng);
  hipStream_t st = eng_stream(e);
  if (int rc = h->genomes.upload(e, sorted, st)) return rc;
  HIP_TRY(e, hipMemcpyAsync(h->g_taxid.p, gtax.data(), g1 * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(e, hipMemcpyAsync(h->t_key[0].p, keys.data(), n1 * 8, hipMemcpyHostToDevice, st));
  if (n > 0) {
    HIP_TRY(e, hipMemcpyAsync(h->in_parent.p, cfg->parent, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(e, hipMemcpyAsync(h->in_rank.p, cfg->rank, n, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(e, hipMemsetAsync(h->cursor.p, 0, 16, st));
  HIP_TRY(e, hipMemsetAsync(h->counts.p, 0, COUNT_WORDS * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->word.p, 0, 16, st));
  HIP_TRY(e, hipMemsetAsync(h->direct.p, 0, n1 * 24, st));
  h->tkey = h->t_key[0].as<const uint64_t>();
  h->n_nodes = n;
  const uint32_t cus = (uint32_t)std::max(eng_cu_count(e), 1);
  const uint32_t* perm = nullptr;
  if (n > 0) {
    uint64_t* const keys2[2] = {h->t_key[0].as<uint64_t>(), h->t_key[1].as<uint64_t>()};
    uint32_t* const idxs[2] = {h->t_idx[0].as<uint32_t>(), h->t_idx[1].as<uint32_t>()};
    const uint32_t key_bits = bits_of(largest);
    const int cur = samsort_sort_pairs(st, keys2, idxs, h->hist.as<uint32_t>(), h->digit_total.as<uint32_t>(), n, key_bits);
    h->tkey = h->t_key[cur].as<const uint64_t>();
    perm = key_bits > 0u ? h->t_idx[cur].as<const uint32_t>() : nullptr;
  }
  if ((uint64_t)n + ng > 0) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n + ng + TXE_WG_RECS - 1) / TXE_WG_RECS, (uint64_t)cus * 8u);
    hipLaunchKernelGGL(k_txe_nodes, dim3(grid), dim3(TXE_WG), 0, st, h->tkey, perm, h->in_parent.as<const uint32_t>(), h->in_rank.as<const uint8_t>(), n,
                       h->g_taxid.as<const uint32_t>(), ng, h->taxid.as<uint32_t>(), h->prow.as<uint32_t>(), h->rank.as<uint8_t>(), h->g_node.as<uint32_t>(),
                       h->word.as<uint32_t>());
  }
  if (n > 0) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + TXE_BUILD_WG - 1) / TXE_BUILD_WG, (uint64_t)cus * TXE_BUILD_TRIP_WGS);
    hipLaunchKernelGGL(k_txe_lineage, dim3(grid), dim3(TXE_BUILD_WG), 0, st, h->prow.as<const uint32_t>(), h->rank.as<const uint8_t>(), n,
                       h->depth.as<uint32_t>(), h->anc.as<uint32_t>(), h->word.as<uint32_t>());
  }
  hipError_t launched = hipGetLastError();
  if (launched != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "taxeval reset launch failed: %s", hipGetErrorString(launched));
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "taxeval reset")) return rc;  // (the uploads read host vectors that end here)
  if (errw & TXE_ERR_TREE) return tree_refusal(e, errw);
  h->n_names = ng;
  h->reset_once = true;
  return SIMMR_OK;
}

int simmr_taxeval_lineage(simmr_taxeval* h, uint32_t taxid, uint32_t* out_taxid, uint32_t* depth) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_taxeval_lineage called before simmr_taxeval_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  uint32_t host[TXE_RANKS + 2u] = {};
  hipLaunchKernelGGL(k_txe_look, dim3(1), dim3(TXE_LANES), 0, st, h->tree(), h->taxid.as<const uint32_t>(), taxid, h->look.as<uint32_t>());
  HIP_TRY(e, hipMemcpyAsync(host, h->look.p, sizeof host, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "taxeval lineage")) return rc;
  if (taxid == 0u || !host[TXE_RANKS + 1u]) return eng_fail(e, SIMMR_EINVAL, "simmr_taxeval_lineage: %u is no node", taxid);
  if (out_taxid) std::memcpy(out_taxid, host, TXE_RANKS * 4);
  if (depth) *depth = host[TXE_RANKS];
  return SIMMR_OK;
}

int simmr_taxeval_truth_add(simmr_taxeval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_taxeval_truth_add")) return rc;
  h->planned = false;
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t cap = h->line_cap + n_bytes / TXE_MIN_LINE + 1, held = h->line_cap;
  if (!h->u_id.grow_keep(cap * 8, held * 8, st) || !h->u_genome.grow_keep(cap * 4, held * 4, st))
    return eng_fail(e, SIMMR_ENOMEM, "taxeval truth: allocation failed for %llu lines", (unsigned long long)cap);
  h->line_cap = cap;
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  uint32_t rec_grid = 1;
  if (int rc = enqueue_index(h, text, n_bytes, st, &W, &rec_grid)) return rc;
  hipLaunchKernelGGL(k_txe_truth, dim3(rec_grid), dim3(TXE_WG), 0, st, W, h->names(), h->u_id.as<uint64_t>(), h->u_genome.as<uint32_t>(), cap,
                     h->cursor.as<unsigned long long>(), h->counts_p(), h->word.as<uint32_t>());
  return h->sp.end(e, SPAN_ADDS, st, "taxeval truth add");
}

int simmr_taxeval_truth_plan(simmr_taxeval* h, uint64_t* n_entries) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_taxeval_truth_plan called before simmr_taxeval_reset");
  h->planned = false;
  h->n_entries = 0;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  uint64_t cur2[2] = {0, 0};
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(cur2, h->cursor.p, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "taxeval truth adds")) return rc;
  if (int rc = h->sp.fold(e, "taxeval")) return rc;
  if (errw & TXE_ERR_TRUTH) return eng_fail(e, SIMMR_EINVAL, "a malformed truth record: %s", TRUTH_MALFORMED);
  const uint64_t n = std::min(cur2[0], h->line_cap);
  if (n >= (1ull << 31)) return eng_fail(e, SIMMR_ERANGE, "simmr_taxeval_truth_plan takes fewer than 2^31 truth lines (%llu given)", (unsigned long long)n);
  const uint64_t n1 = std::max<uint64_t>(n, 1), n_tiles = (n + SAMSORT_PAIRS_TILE - 1) / SAMSORT_PAIRS_TILE;
  const uint64_t head_tiles = (n + TXE_HEAD_TILE - 1) / TXE_HEAD_TILE;
  bool room = h->hist.ensure(std::max<uint64_t>(n_tiles, 1) * SAMSORT_PAIRS_DIGITS * 4) && h->head_sum.ensure(std::max<uint64_t>(head_tiles, 1) * 8) &&
              h->head_prefix.ensure((head_tiles + 1) * 8);
  for (DevBuf* b : {&h->key[0], &h->key[1], &h->e_id}) room = room && b->ensure(n1 * 8);
  for (DevBuf* b : {&h->idx[0], &h->idx[1], &h->e_genome, &h->e_mates, &h->seen, &h->hits}) room = room && b->ensure(n1 * 4);
  if (!room) return eng_fail(e, SIMMR_ENOMEM, "taxeval truth plan: allocation failed (%llu lines)", (unsigned long long)n);
  if (int rc = h->sp.begin(e, SPAN_PLAN, st)) return rc;
  // the candidate side starts over: its counts (the words behind the truth's two), the two rank tables, the node counts, seen and hits
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + TC_T_ENTRIES, 0, (COUNT_WORDS - TC_T_ENTRIES) * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->direct.p, 0, std::max<uint64_t>(h->n_nodes, 1) * 24, st));
  HIP_TRY(e, hipMemsetAsync(h->seen.p, 0, n1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->hits.p, 0, n1 * 4, st));
  HIP_TRY(e, hipMemsetAsync(h->head_prefix.p, 0, (head_tiles + 1) * 8, st));
  if (n > 0) {
    HIP_TRY(e, hipMemcpyAsync(h->key[0].p, h->u_id.p, n * 8, hipMemcpyDeviceToDevice, st));
    uint64_t* const keys[2] = {h->key[0].as<uint64_t>(), h->key[1].as<uint64_t>()};
    uint32_t* const idxs[2] = {h->idx[0].as<uint32_t>(), h->idx[1].as<uint32_t>()};
    const uint32_t key_bits = bits_of(cur2[1]);
    const int cur = samsort_sort_pairs(st, keys, idxs, h->hist.as<uint32_t>(), h->digit_total.as<uint32_t>(), n, key_bits);
    const uint64_t* skey = h->key[cur].as<const uint64_t>();
    const uint32_t* perm = key_bits > 0u ? h->idx[cur].as<const uint32_t>() : (const uint32_t*)nullptr;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(head_tiles, (uint64_t)std::max(eng_cu_count(e), 1) * 16u);
    hipLaunchKernelGGL(k_txe_heads, dim3(grid), dim3(256), 0, st, skey, perm, n, head_tiles, h->head_sum.as<uint64_t>(), (const uint64_t*)nullptr,
                       h->u_genome.as<const uint32_t>(), (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, h->word.as<uint32_t>());
    hipLaunchKernelGGL(k_txe_scan, dim3(1), dim3(256), 0, st, h->head_sum.as<const uint64_t>(), h->head_prefix.as<uint64_t>(), head_tiles);
    hipLaunchKernelGGL(k_txe_heads, dim3(grid), dim3(256), 0, st, skey, perm, n, head_tiles, h->head_sum.as<uint64_t>(), h->head_prefix.as<const uint64_t>(),
                       h->u_genome.as<const uint32_t>(), h->e_id.as<uint64_t>(), h->e_genome.as<uint32_t>(), h->e_mates.as<uint32_t>(), h->word.as<uint32_t>());
  }
  if (int rc = h->sp.end(e, SPAN_PLAN, st, "taxeval truth plan")) return rc;
  uint64_t heads = 0;
  HIP_TRY(e, hipMemcpyAsync(&heads, h->head_prefix.as<uint64_t>() + head_tiles, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "taxeval truth plan")) return rc;
  if (errw & TXE_ERR_PLAN) {
    uint32_t cleared = errw & ~TXE_ERR_PLAN;  // (the lines stay; the flags are the plan's alone)
    HIP_TRY(e, hipMemcpy(h->word.p, &cleared, 4, hipMemcpyHostToDevice));
    return eng_fail(e, SIMMR_EINVAL, errw & TXE_ERR_MATES ? "more than two truth lines have one read id" : "two truth lines of one read id name different genomes");
  }
  h->n_entries = std::min(heads, n);
  HIP_TRY(e, hipMemcpy(h->counts_p() + TC_T_ENTRIES, &h->n_entries, 8, hipMemcpyHostToDevice));
  h->planned = true;
  if (int rc = h->sp.fold(e, "taxeval")) return rc;
  if (n_entries) *n_entries = h->n_entries;
  return SIMMR_OK;
}

int simmr_taxeval_add(simmr_taxeval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_add(h, text, n_bytes, "simmr_taxeval_add")) return rc;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_taxeval_add called without a simmr_taxeval_truth_plan in force");
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (int rc = h->sp.begin(e, SPAN_ADDS, st)) return rc;
  MevText W;
  uint32_t rec_grid = 1;
  if (int rc = enqueue_index(h, text, n_bytes, st, &W, &rec_grid)) return rc;
  hipLaunchKernelGGL(k_txe_record, dim3(rec_grid), dim3(TXE_WG), 0, st, W, h->entries(), h->tree(), h->g_node.as<const uint32_t>(), h->counts_p(),
                     h->counts_p() + TC_COUNT, h->direct.as<unsigned long long>(), h->seen.as<uint32_t>(), h->hits.as<uint32_t>(), h->word.as<uint32_t>());
  return h->sp.end(e, SPAN_ADDS, st, "taxeval add");
}

int simmr_taxeval_read(simmr_taxeval* h, simmr_taxeval_counts* counts, uint64_t* by_rank_host, uint64_t* reads_by_rank_host) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_taxeval_read called before simmr_taxeval_reset");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + TC_T_PAIRED, 0, 8, st));
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + TC_MISSING, 0, (TC_COUNT - TC_MISSING) * 8, st));
  HIP_TRY(e, hipMemsetAsync(h->counts_p() + TC_COUNT + TXE_RANK_WORDS, 0, TXE_RANK_WORDS * 8, st));
  if (h->planned && h->n_entries > 0) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((h->n_entries + 255) / 256, (uint64_t)std::max(eng_cu_count(e), 1) * 16u);
    hipLaunchKernelGGL(k_txe_reduce, dim3(grid), dim3(256), 0, st, h->entries(), h->g_node.as<const uint32_t>(), h->anc.as<const uint32_t>(),
                       h->seen.as<const uint32_t>(), h->hits.as<const uint32_t>(), h->counts_p(), h->counts_p() + TC_COUNT + TXE_RANK_WORDS);
  }
  std::vector<uint64_t> host(COUNT_WORDS);
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(host.data(), h->counts.p, COUNT_WORDS * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, h->word.p, 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "taxeval read")) return rc;
  if (errw & TXE_ERR_TRUTH) return eng_fail(e, SIMMR_EINVAL, "a malformed truth record: %s", TRUTH_MALFORMED);
  if (errw & TXE_ERR_CAND) return eng_fail(e, SIMMR_EINVAL, "a malformed candidate record: %s", CAND_MALFORMED);
  if (counts) std::memcpy(counts, host.data(), sizeof(*counts));
  if (by_rank_host) std::memcpy(by_rank_host, host.data() + TC_COUNT, TXE_RANK_WORDS * 8);
  if (reads_by_rank_host) std::memcpy(reads_by_rank_host, host.data() + TC_COUNT + TXE_RANK_WORDS, TXE_RANK_WORDS * 8);
  return SIMMR_OK;
}

int simmr_taxeval_emit(simmr_taxeval* h, uint64_t* id_dev, uint32_t* genome_row_dev, uint32_t* mates_dev, uint32_t* seen_dev, uint32_t* hits_dev,
                       uint64_t capacity) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_taxeval_emit called without a simmr_taxeval_truth_plan in force");
  if (capacity < h->n_entries)
    return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu truth entries", (unsigned long long)capacity, (unsigned long long)h->n_entries);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (h->n_entries > 0) {
    if (id_dev) HIP_TRY(e, hipMemcpyAsync(id_dev, h->e_id.p, h->n_entries * 8, hipMemcpyDeviceToDevice, st));
    if (genome_row_dev) HIP_TRY(e, hipMemcpyAsync(genome_row_dev, h->e_genome.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
    if (mates_dev) HIP_TRY(e, hipMemcpyAsync(mates_dev, h->e_mates.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
    if (seen_dev) HIP_TRY(e, hipMemcpyAsync(seen_dev, h->seen.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
    if (hits_dev) HIP_TRY(e, hipMemcpyAsync(hits_dev, h->hits.p, h->n_entries * 4, hipMemcpyDeviceToDevice, st));
  }
  return sync_check(e, "taxeval emit");
}

int simmr_taxeval_taxa(simmr_taxeval* h, uint32_t* taxid_dev, uint64_t* true_dev, uint64_t* called_dev, uint64_t* both_dev, uint64_t capacity_nodes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "simmr_taxeval_taxa called before simmr_taxeval_reset");
  const uint64_t n = h->n_nodes;
  if (capacity_nodes < n) return eng_fail(e, SIMMR_ERANGE, "capacity %llu < %llu nodes", (unsigned long long)capacity_nodes, (unsigned long long)n);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (n > 0) {
    HIP_TRY(e, hipMemsetAsync(h->clade.p, 0, n * 24, st));
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + TXE_BUILD_WG - 1) / TXE_BUILD_WG, (uint64_t)std::max(eng_cu_count(e), 1) * TXE_BUILD_TRIP_WGS);
    hipLaunchKernelGGL(k_txe_rollup, dim3(grid), dim3(TXE_BUILD_WG), 0, st, h->direct.as<const unsigned long long>(), h->clade.as<unsigned long long>(),
                       h->prow.as<const uint32_t>(), (uint32_t)n);
    const uint64_t* c = h->clade.as<const uint64_t>();
    if (taxid_dev) HIP_TRY(e, hipMemcpyAsync(taxid_dev, h->taxid.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (true_dev) HIP_TRY(e, hipMemcpyAsync(true_dev, c, n * 8, hipMemcpyDeviceToDevice, st));
    if (called_dev) HIP_TRY(e, hipMemcpyAsync(called_dev, c + n, n * 8, hipMemcpyDeviceToDevice, st));
    if (both_dev) HIP_TRY(e, hipMemcpyAsync(both_dev, c + 2 * n, n * 8, hipMemcpyDeviceToDevice, st));
  }
  return sync_check(e, "taxeval taxa");
}

int simmr_last_taxeval_ms(simmr_taxeval* h, float* ms) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!ms) return eng_fail(e, SIMMR_EINVAL, "simmr_last_taxeval_ms: NULL ms");
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_taxeval_reset yet");
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  return h->sp.last_ms(e, "taxeval", ms);
}

}  // extern "C"
