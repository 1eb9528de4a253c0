// taxeval.hip — a read classifier's calls scored against each read's true genome (include/simmr_hip.h: simmr_taxeval_*): the entry
// points over taxeval_kernels.hip.  A translation unit of libsimmr_hip.so of its own; it sees an engine through engine_internal.hpp
// only.  The engine's slot enum is full, so the state lives in an object of its own that the caller creates on an engine and
// destroys before the engine, as vcfeval.hip's does.  The genome names are kept as mapeval.hip keeps its names (sorted, in a device
// blob), the sort is sam_sort.hip's (samsort_sort_pairs): run once by the reset over the taxids and once by the plan over the ids.
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
// Time: two spans, as vcfeval.hip keeps them: the adds of either side are one span from the first to the last, the plan has one
// of its own, and a call that synchronises anyway folds the spans that count into a sum.  The reset's work is not timed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "host_support.hpp"
#include "taxeval_kernels.hip"

using namespace simmr;

namespace {

uint32_t bits_of(uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }

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
  DevBuf blob, name_off, g_taxid, g_node;
  uint32_t n_names = 0;
  // the tree: what the caller gave (in_*), the sorted taxids (t_key[t_cur]), and per sorted node its columns
  DevBuf in_parent, in_rank, t_key[2], t_idx[2], taxid, prow, rank, depth, anc;
  DevBuf direct, clade;  // [3][n_nodes] each: true, called, both
  DevBuf look;           // the ten words of k_txe_look
  const uint64_t* tkey = nullptr;
  uint32_t n_nodes = 0;
  // the line index of one add
  DevBuf tile_sum, tile_prefix, starts;
  // the truth: the lines as appended (u_*), the sort's buffers, and the entries in id order (e_*)
  DevBuf u_id, u_genome, key[2], idx[2], hist, digit_total, head_sum, head_prefix, e_id, e_genome, e_mates;
  DevBuf cursor;   // [0] lines, [1] the largest id
  DevBuf counts;   // TC_COUNT words, then by_rank's 40 and reads_by_rank's 40
  DevBuf word;     // the error word
  DevBuf seen, hits;
  uint64_t line_cap = 0;   // lines the truth adds since the reset may have appended
  uint64_t n_entries = 0;
  bool reset_once = false, planned = false;
  Spans<SPAN_COUNT> sp;
  bool open = false;  // the span of the adds has begun and is not folded yet
  float done_ms = 0.f;

  MevNames names() const { return MevNames{blob.as<const uint8_t>(), name_off.as<const uint32_t>(), n_names}; }
  TxeTree tree() const { return TxeTree{tkey, prow.as<const uint32_t>(), depth.as<const uint32_t>(), anc.as<const uint32_t>(), n_nodes}; }
  TxeEntries entries() const { return TxeEntries{e_id.as<const uint64_t>(), e_genome.as<const uint32_t>(), e_mates.as<const uint32_t>(), n_entries}; }
  unsigned long long* counts_p() const { return counts.as<unsigned long long>(); }
};

namespace {

int check_text(simmr_taxeval* h, const uint8_t* text, uint64_t n_bytes, const char* who) {
  simmr_engine* e = h->e;
  if (!h->reset_once) return eng_fail(e, SIMMR_ESTATE, "%s called before simmr_taxeval_reset", who);
  if (!text && n_bytes > 0) return eng_fail(e, SIMMR_EINVAL, "%s: NULL text", who);
  if (n_bytes > SIMMR_FIT_SAM_MAX_BYTES)
    return eng_fail(e, SIMMR_ENOTSUP, "%s: %llu bytes in one add (at most %llu: cut the text at a line's end)", who, (unsigned long long)n_bytes,
                    (unsigned long long)SIMMR_FIT_SAM_MAX_BYTES);
  return SIMMR_OK;
}

// the span `which` runs from here, unless it is the adds' and open already
int begin_span(simmr_taxeval* h, int which, hipStream_t st) {
  if (which == SPAN_ADDS && h->open) return SIMMR_OK;
  HIP_TRY(h->e, h->sp.begin(which, st));
  return SIMMR_OK;
}

// the spans that count into the sum, and closed.  Synchronises.
int fold_spans(simmr_taxeval* h) {
  float now = 0.f;
  if (int rc = h->sp.total_ms(h->e, "taxeval", &now)) return rc;
  h->done_ms += now;
  h->sp.invalidate_from(0);
  h->open = false;
  return SIMMR_OK;
}

// ... and ends behind what was enqueued; a launch that failed leaves the span as it was
int end_span(simmr_taxeval* h, int which, hipStream_t st, const char* what) {
  simmr_engine* e = h->e;
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "%s launch failed: %s", what, hipGetErrorString(rc));
  HIP_TRY(e, h->sp.end(which, st));
  if (which == SPAN_ADDS) h->open = true;
  h->sp.mark(which);
  return SIMMR_OK;
}

// the line index of text[0, n_bytes) into the object's buffers (n_bytes > 0)
int enqueue_index(simmr_taxeval* h, const uint8_t* text, uint64_t n_bytes, hipStream_t st, MevText* W, uint32_t* rec_grid) {
  simmr_engine* e = h->e;
  const uint64_t n_tiles = (n_bytes + FSAM_TILE - 1) / FSAM_TILE, start_cap = n_bytes / 2 + 1;
  if (!h->tile_sum.ensure(n_tiles * 8) || !h->tile_prefix.ensure((n_tiles + 1) * 8) || !h->starts.ensure(start_cap * 4))
    return eng_fail(e, SIMMR_ENOMEM, "taxeval line index: allocation failed for %llu bytes of text", (unsigned long long)n_bytes);
  const uint32_t cus = (uint32_t)std::max(eng_cu_count(e), 1);
  const uint32_t tile_grid = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)cus * 16u);
  *rec_grid = (uint32_t)std::min<uint64_t>(n_bytes / (TXE_WG_RECS * TXE_MIN_LINE) + 1, (uint64_t)cus * 8u);
  hipLaunchKernelGGL(k_txe_index, dim3(tile_grid), dim3(FSAM_WG), 0, st, text, n_bytes, n_tiles, h->tile_sum.as<uint64_t>(), (const uint64_t*)nullptr,
                     (uint32_t*)nullptr, 0ull);
  hipLaunchKernelGGL(k_txe_scan, dim3(1), dim3(256), 0, st, h->tile_sum.as<const uint64_t>(), h->tile_prefix.as<uint64_t>(), n_tiles);
  hipLaunchKernelGGL(k_txe_index, dim3(tile_grid), dim3(FSAM_WG), 0, st, text, n_bytes, n_tiles, h->tile_sum.as<uint64_t>(),
                     h->tile_prefix.as<const uint64_t>(), h->starts.as<uint32_t>(), start_cap);
  *W = MevText{text, n_bytes, h->tile_prefix.as<const uint64_t>() + n_tiles, h->starts.as<const uint32_t>()};
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

int simmr_taxeval_create(simmr_engine* e, simmr_taxeval** out) {
  if (!e) return SIMMR_EINVAL;
  if (!out) return eng_fail(e, SIMMR_EINVAL, "simmr_taxeval_create: NULL out");
  *out = nullptr;
  simmr_taxeval* h = new (std::nothrow) simmr_taxeval();
  if (!h) return eng_fail(e, SIMMR_ENOMEM, "simmr_taxeval_create: out of memory");
  h->e = e;
  *out = h;
  return SIMMR_OK;
}

void simmr_taxeval_destroy(simmr_taxeval* h) {
  if (!h) return;
  if (hipSetDevice(eng_device(h->e)) == hipSuccess) (void)hipStreamSynchronize(eng_stream(h->e));
  delete h;  // (its buffers and events go with it)
  (void)hipGetLastError();
}

int simmr_taxeval_reset(simmr_taxeval* h, const simmr_taxeval_config* cfg) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (!cfg || (cfg->n_nodes > 0 && (!cfg->taxid || !cfg->parent || !cfg->rank)) || (cfg->n_genomes > 0 && (!cfg->genome_id || !cfg->genome_taxid)))
    return eng_fail(e, SIMMR_EINVAL, "simmr_taxeval_reset: NULL argument");
  if (cfg->n_nodes > MAX_NODES) return eng_fail(e, SIMMR_ERANGE, "simmr_taxeval_reset: %llu nodes (at most 2^26)", (unsigned long long)cfg->n_nodes);
  if (cfg->n_genomes > MAX_GENOMES) return eng_fail(e, SIMMR_ERANGE, "simmr_taxeval_reset: %llu genomes (at most 2^24)", (unsigned long long)cfg->n_genomes);
  const uint32_t n = (uint32_t)cfg->n_nodes, ng = (uint32_t)cfg->n_genomes;
  std::vector<std::string> ids;
  ids.reserve(ng);
  for (uint32_t i = 0; i < ng; i++) {
    const char* s = cfg->genome_id[i];
    const size_t len = s ? std::strlen(s) : 0;
    if (len == 0 || len > SAM_RNAME_MAX) return eng_fail(e, SIMMR_ENOTSUP, "genome id %u is empty or longer than %u bytes", i, SAM_RNAME_MAX);
    if (std::strchr(s, '\t') || std::strchr(s, '\n')) return eng_fail(e, SIMMR_ENOTSUP, "genome id %u holds a tab or a newline", i);
    ids.emplace_back(s, len);
  }
  std::vector<uint32_t> order(ng);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {  // (bytewise, a prefix first, as mev_compare orders them)
    return std::lexicographical_compare(ids[a].begin(), ids[a].end(), ids[b].begin(), ids[b].end(),
                                        [](char x, char y) { return (unsigned char)x < (unsigned char)y; });
  });
  for (uint32_t i = 1; i < ng; i++)
    if (ids[order[i]] == ids[order[i - 1]]) return eng_fail(e, SIMMR_EINVAL, "genome id '%s' is given twice", ids[order[i]].c_str());
  std::vector<uint8_t> blob;
  std::vector<uint32_t> off{0u}, gtax(std::max(ng, 1u), 0u);
  for (uint32_t i = 0; i < ng; i++) {
    const std::string& s = ids[order[i]];
    blob.insert(blob.end(), s.begin(), s.end());
    off.push_back((uint32_t)blob.size());
    gtax[i] = cfg->genome_taxid[order[i]];
  }
  blob.resize(blob.size() + 8, 0);
  uint32_t largest = 0;
  for (uint32_t i = 0; i < n; i++) largest = std::max(largest, cfg->taxid[i]);
  std::vector<uint64_t> keys(std::max(n, 1u), 0ull);
  for (uint32_t i = 0; i < n; i++) keys[i] = cfg->taxid[i];

  HIP_TRY(e, hipSetDevice(eng_device(e)));
  if (int rc = sync_check(e, "taxeval reset")) return rc;
  h->planned = false;
  h->reset_once = false;
  h->sp.invalidate_from(0);
  h->open = false;
  h->done_ms = 0.f;
  h->n_entries = 0;
  h->line_cap = 0;
  if (int rc = h->sp.create_missing(e)) return rc;
  const uint64_t n1 = std::max(n, 1u), g1 = std::max(ng, 1u), n_tiles = (n + SAMSORT_PAIRS_TILE - 1) / SAMSORT_PAIRS_TILE;
  bool room = h->blob.ensure(blob.size()) && h->name_off.ensure(off.size() * 4) && h->g_taxid.ensure(g1 * 4) && h->g_node.ensure(g1 * 4) &&
              h->cursor.ensure(16) && h->counts.ensure(COUNT_WORDS * 8) && h->word.ensure(16) && h->look.ensure(64) && h->in_parent.ensure(n1 * 4) &&
              h->in_rank.ensure(n1) && h->rank.ensure(n1) && h->anc.ensure(n1 * TXE_RANKS * 4) && h->direct.ensure(n1 * 24) && h->clade.ensure(n1 * 24) &&
              h->hist.ensure(std::max<uint64_t>(n_tiles, 1) * SAMSORT_PAIRS_DIGITS * 4) && h->digit_total.ensure(SAMSORT_PAIRS_DIGITS * 4);
  for (DevBuf* b : {&h->t_key[0], &h->t_key[1]}) room = room && b->ensure(n1 * 8);
  for (DevBuf* b : {&h->t_idx[0], &h->t_idx[1], &h->taxid, &h->prow, &h->depth}) room = room && b->ensure(n1 * 4);
  if (!room) return eng_fail(e, SIMMR_ENOMEM, "taxeval reset: allocation failed (%u nodes, %u genomes)", n, ng);
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, hipMemcpyAsync(h->blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(e, hipMemcpyAsync(h->name_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, st));
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
  if (int rc = check_text(h, text, n_bytes, "simmr_taxeval_truth_add")) return rc;
  h->planned = false;
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  const uint64_t cap = h->line_cap + n_bytes / TXE_MIN_LINE + 1, held = h->line_cap;
  if (!h->u_id.grow_keep(cap * 8, held * 8, st) || !h->u_genome.grow_keep(cap * 4, held * 4, st))
    return eng_fail(e, SIMMR_ENOMEM, "taxeval truth: allocation failed for %llu lines", (unsigned long long)cap);
  h->line_cap = cap;
  if (int rc = begin_span(h, SPAN_ADDS, st)) return rc;
  MevText W;
  uint32_t rec_grid = 1;
  if (int rc = enqueue_index(h, text, n_bytes, st, &W, &rec_grid)) return rc;
  hipLaunchKernelGGL(k_txe_truth, dim3(rec_grid), dim3(TXE_WG), 0, st, W, h->names(), h->u_id.as<uint64_t>(), h->u_genome.as<uint32_t>(), cap,
                     h->cursor.as<unsigned long long>(), h->counts_p(), h->word.as<uint32_t>());
  return end_span(h, SPAN_ADDS, st, "taxeval truth add");
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
  if (int rc = fold_spans(h)) return rc;
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
  if (int rc = begin_span(h, SPAN_PLAN, st)) return rc;
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
  if (int rc = end_span(h, SPAN_PLAN, st, "taxeval truth plan")) return rc;
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
  if (int rc = fold_spans(h)) return rc;
  if (n_entries) *n_entries = h->n_entries;
  return SIMMR_OK;
}

int simmr_taxeval_add(simmr_taxeval* h, const uint8_t* text, uint64_t n_bytes) {
  if (!h) return SIMMR_EINVAL;
  simmr_engine* e = h->e;
  if (int rc = check_text(h, text, n_bytes, "simmr_taxeval_add")) return rc;
  if (!h->planned) return eng_fail(e, SIMMR_ESTATE, "simmr_taxeval_add called without a simmr_taxeval_truth_plan in force");
  if (n_bytes == 0) return SIMMR_OK;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  if (int rc = begin_span(h, SPAN_ADDS, st)) return rc;
  MevText W;
  uint32_t rec_grid = 1;
  if (int rc = enqueue_index(h, text, n_bytes, st, &W, &rec_grid)) return rc;
  hipLaunchKernelGGL(k_txe_record, dim3(rec_grid), dim3(TXE_WG), 0, st, W, h->entries(), h->tree(), h->g_node.as<const uint32_t>(), h->counts_p(),
                     h->counts_p() + TC_COUNT, h->direct.as<unsigned long long>(), h->seen.as<uint32_t>(), h->hits.as<uint32_t>(), h->word.as<uint32_t>());
  return end_span(h, SPAN_ADDS, st, "taxeval add");
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
  if (int rc = fold_spans(h)) return rc;  // (the next add of either side begins a new span)
  *ms = h->done_ms;
  return SIMMR_OK;
}

}  // extern "C"
