// taxeval_kernels.hip — a read classifier's calls scored against each read's true genome (gfx950): a taxonomy, the truth TSV and
// the classifier's per-read text in HBM to integer tables (include/simmr_hip.h states every rule: the tree, the two records, what
// is malformed, the order of the steps, the class of a rank, the tables).  Included by taxeval.hip alone, a translation unit of
// its own.  The reader's routines are taken, not restated: the line index and the scans of fit_sam_kernels.hip / sam_kernels.hip,
// the name row and the 16-way group search of mapeval_kernels.hip, through MEV_ROUTINES_ONLY (which brings FSAM_ROUTINES_ONLY).
//
// Ten kernels; a work item of the text kernels, of k_txe_nodes and of k_txe_look is shared by TXE_LANES = 16 lanes (one DPP row).
//   k_txe_index    fsam_index_tiles: launched to count a tile's line starts and, after the scan, to write them.
//   k_txe_scan     ONE workgroup: sam_scan_chunks over tile counts — the line index's, and the head counts of k_txe_heads.
//   k_txe_nodes    behind the sort of the taxids: a node per group — its taxid, rank and the row of its parent (mev_lower_bound),
//                  the refusals of a node; then a genome per group — the row of its taxid.
//   k_txe_lineage  a node per thread: the walk to the root — the depth, and the row of the nearest ancestor-or-self at each rank.
//   k_txe_look     ONE group: the lineage of one taxid as taxids, for simmr_taxeval_lineage.
//   k_txe_truth    a truth line per group: read id, pair, the genome's name row; an entry (id, row) is appended through an atomic
//                  cursor — the order is arbitrary and nothing depends on it: equal ids must agree in all that is kept.
//   k_txe_heads    behind the sort of the ids: an id that differs from the one before it is a head.  Launched to count a tile's
//                  heads and, after the scan, to write the entry of every head (id, genome row, the lines behind it).
//   k_txe_record   a candidate line per group: the three fields, the id looked up in the entries and the taxid in the nodes by
//                  mev_lower_bound, the lowest common ancestor by a walk, the class of rank r in lane r - 1; the counts and by_rank
//                  privatised in LDS, seen by one atomicOr and hits by one atomicAdd, and the three per-node counts combined in
//                  an LDS table keyed by (count, row) that goes to HBM when the workgroup ends: a classifier calls few taxa and a
//                  run has few genomes, so nearly every increment would land on one of a handful of addresses.
//   k_txe_reduce   the per-entry counts (paired, missing, multiple) and reads_by_rank over seen[] / hits[] / mates[].
//   k_txe_rollup   a node per thread: its three direct counts added to every node on its path to the root (the clade sums).
// Convergence.  Everything a group decides is decided from values all its 16 lanes hold alike, so the lanes of a group take every
// branch and loop trip together: the ballots of mev_lower_bound and mev_name_row always see the whole group.
// Bounds.  Every load of text is below n_bytes and inside the line's fields: a field is [a, b) with line <= a <= b <= the line's
// end <= n_bytes.  A truth entry is stored below the capacity the adds' byte counts gave.  A node row is a search result below
// n_nodes whose key was compared, or a parent row, an ancestor row or a genome's row, which k_txe_nodes made the same way and
// the reset checked (a reset that finds a refusal leaves the object without a tree, and no other kernel runs).  An entry row is a
// search result below n_entries; a genome row is a name row below the names.  A walk ends at a root (a row that is its own parent)
// after at most TXE_MAX_DEPTH steps, as k_txe_lineage showed for every node.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#define MEV_ROUTINES_ONLY
#include "mapeval_kernels.hip"  // mev_name_row, mev_lower_bound, MevNames, MevText; through it the reader's routines and the scans

namespace simmr {

#define TXE_LANES 16u
#define TXE_WG 256u
#define TXE_WG_RECS 16u      /* lines (or nodes) per workgroup and batch */
#define TXE_MIN_LINE 5u      /* the shortest record of either side: 3 one-byte fields and 2 tabs */
#define TXE_HEAD_TILE 256u   /* sorted ids per workgroup and round of k_txe_heads: an id a thread */
#define TXE_BUILD_WG 256u    /* nodes per workgroup and grid trip of k_txe_lineage and k_txe_rollup */
#define TXE_BUILD_TRIP_WGS 2u /* ... and workgroups per CU of their grids */
#define TXE_RANKS 8u
#define TXE_CLASSES 5u
#define TXE_MAX_DEPTH 255u
#define TXE_NONE 0xffffffffu
#define TXE_ROW_BITS 26u     /* a node row is below 2^26 */
#define TXE_HOT_SLOTS 512u   /* the LDS table of k_txe_record: (count, row) + 1 and its sum */
#define TXE_HOT_PROBES 4u
#define TXE_ERR_TRUTH 1u     /* a malformed truth record */
#define TXE_ERR_CAND 2u      /* a malformed candidate record */
#define TXE_ERR_GENOMES 4u   /* one read id with two genomes */
#define TXE_ERR_MATES 8u     /* more than two lines with one read id */
#define TXE_ERR_TAXID0 16u   /* the refusals of the tree */
#define TXE_ERR_TWICE 32u
#define TXE_ERR_PARENT 64u
#define TXE_ERR_DEPTH 128u
#define TXE_ERR_RANK 256u
#define TXE_ERR_GENOME_TAXID 512u
#define TXE_ERR_RANK_TWICE 1024u
#define TXE_ERR_PLAN (TXE_ERR_GENOMES | TXE_ERR_MATES)
#define TXE_ERR_TREE (TXE_ERR_TAXID0 | TXE_ERR_TWICE | TXE_ERR_PARENT | TXE_ERR_DEPTH | TXE_ERR_RANK | TXE_ERR_GENOME_TAXID | TXE_ERR_RANK_TWICE)
static_assert(TXE_LANES == MEV_LANES && TXE_LANES == FSAM_LANES, "the group of the search and of the ballot is the reader's");
static_assert(TXE_RANKS == SIMMR_TAXEVAL_RANKS && TXE_MAX_DEPTH == SIMMR_TAXEVAL_MAX_DEPTH, "the header's ranks and depth");
static_assert(TXE_RANKS <= TXE_LANES && 4u * TXE_RANKS == 32u, "a rank a lane, a nibble a rank");

enum { TC_T_LINES = 0, TC_T_HEADER, TC_T_ENTRIES, TC_T_PAIRED, TC_LINES, TC_HEADER, TC_RECORDS, TC_UNKNOWN_READ, TC_UNCLASSIFIED, TC_UNKNOWN_TAXON,
       TC_SCORED, TC_MISSING, TC_MULTIPLE, TC_COUNT };
static_assert(sizeof(simmr_taxeval_counts) == TC_COUNT * 8u, "the counts in the header's order");
#define TXE_REC_COUNTS ((uint32_t)(TC_MISSING - TC_LINES))  /* the counts k_txe_record makes */
#define TXE_RANK_WORDS (TXE_RANKS * TXE_CLASSES)

struct TxeTree {  // the nodes in taxid order
  const uint64_t* key;     // [n] the taxids
  const uint32_t* parent;  // [n] the parent's row; a root's is its own
  const uint32_t* depth;   // [n] steps to the root
  const uint32_t* anc;     // [n][8] the row of the nearest ancestor-or-self at rank r + 1, or TXE_NONE
  uint32_t n;
};

struct TxeEntries {  // the truth reads in id order
  const uint64_t* id;
  const uint32_t* genome;  // the name row
  const uint32_t* mates;   // the lines behind the entry: 1 or 2
  uint64_t n;
};

// The first three fields of the line at `line`: tb[j] is the place of tab j (FSAM_NONE: none), *end the line's end.
SIMMR_DEV uint32_t txe_fields(const uint8_t* __restrict__ t, uint32_t n, uint32_t line, uint32_t sub, uint32_t tb[3], uint32_t* end) {
#pragma unroll
  for (uint32_t j = 0; j < 3u; j++) tb[j] = FSAM_NONE;
  uint32_t n_tab = 0;
  *end = n;
  for (uint32_t p0 = line;; p0 += TXE_LANES) {  // (n is at most SIMMR_FIT_SAM_MAX_BYTES: p0 + 16 does not wrap)
    const uint32_t p = p0 + sub;
    const uint32_t c = p < n ? t[p] : '\n';
    uint32_t m_tab = fsam_ballot(c == '\t');
    const uint32_t m_nl = fsam_ballot(c == '\n');
    if (m_nl) {
      const uint32_t first = (uint32_t)__builtin_ctz(m_nl);
      m_tab &= (1u << first) - 1u;
      *end = p0 + first;
    }
    for (; m_tab; m_tab &= m_tab - 1u) {
      const uint32_t at = p0 + (uint32_t)__builtin_ctz(m_tab);
#pragma unroll
      for (uint32_t j = 0; j < 3u; j++)
        if (n_tab == j) tb[j] = at;
      n_tab++;
    }
    if (m_nl) break;
  }
  return n_tab;
}

// whether the line is a header line: its first byte is '#', or it starts with "read_id\t" (a lane a byte)
SIMMR_DEV bool txe_header(const uint8_t* __restrict__ t, uint32_t n, uint32_t line, uint32_t sub) {
  if (t[line] == '#') return true;
  const uint32_t want = (uint32_t)(0x0964695f64616572ull >> (8u * (sub & 7u))) & 0xffu;  // "read_id\t"
  const uint32_t p = line + sub;
  const uint32_t m = fsam_ballot(sub < 8u && p < n && t[p] == want);
  return m == 0xffu;
}

// the read id of the name text[a, b): 1 to 18 digits, then nothing, "/1" or "/2" (the name rule of simmr_ovleval_*; the mate is dropped)
SIMMR_DEV bool txe_read_id(const uint8_t* __restrict__ t, uint32_t a, uint32_t b, uint64_t* id) {
  if (b - a >= 3u && b >= a && t[b - 2u] == '/' && (t[b - 1u] == '1' || t[b - 1u] == '2')) b -= 2u;
  return fsam_field_number(t, a, b, false, id);
}

// the taxid of field 3 text[a, b): 1 to 10 digits below 2^32, or any text that ends in "(taxid <such digits>)"
SIMMR_DEV bool txe_taxon(const uint8_t* __restrict__ t, uint32_t a, uint32_t b, uint64_t* taxid) {
  if (b > a && t[b - 1u] == ')') {
    const uint32_t q = b - 1u;
    uint32_t p = q;
    while (p > a && q - p <= 10u && fsam_digit(t[p - 1u])) p--;
    if (p - a < 7u) return false;
    if (t[p - 7u] != '(' || t[p - 6u] != 't' || t[p - 5u] != 'a' || t[p - 4u] != 'x' || t[p - 3u] != 'i' || t[p - 2u] != 'd' || t[p - 1u] != ' ') return false;
    a = p;
    b = q;
  }
  return b - a <= 10u && fsam_field_number(t, a, b, false, taxid) && *taxid <= 0xffffffffull;
}

// the lowest common ancestor of the rows a and b (TXE_NONE: they stand under different roots): the depths made equal, then both
// walked up together
SIMMR_DEV uint32_t txe_lca(const TxeTree& T, uint32_t a, uint32_t b) {
  uint32_t da = T.depth[a], db = T.depth[b];
  for (; da > db; da--) a = T.parent[a];
  for (; db > da; db--) b = T.parent[b];
  for (; a != b && da > 0u; da--) {
    a = T.parent[a];
    b = T.parent[b];
  }
  return a == b ? a : TXE_NONE;
}

// ---- the line index and the scan ------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_txe_index(const uint8_t* __restrict__ text, uint64_t n_bytes, uint64_t n_tiles, uint64_t* __restrict__ tile_sum,
            const uint64_t* __restrict__ tile_prefix, uint32_t* __restrict__ starts, uint64_t start_capacity) {
  __shared__ uint32_t lds[FSAM_WG];
  fsam_index_tiles(text, n_bytes, n_tiles, tile_sum, tile_prefix, starts, start_capacity, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_txe_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

// ---- the tree -------------------------------------------------------------------------------------------------------------------
// Items [0, n): the node at place i of the sorted taxids (perm == nullptr: the order is the identity).  Items [n, n + n_genomes): a
// genome.  Every refusal goes to the error word; what is stored is a row below n whatever the input holds.
extern "C" __global__ void __launch_bounds__(TXE_WG)
k_txe_nodes(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ parent_in, const uint8_t* __restrict__ rank_in,
            uint32_t n, const uint32_t* __restrict__ g_taxid, uint32_t n_genomes, uint32_t* __restrict__ taxid, uint32_t* __restrict__ prow,
            uint8_t* __restrict__ rank, uint32_t* __restrict__ g_node, uint32_t* __restrict__ err) {
  const uint32_t tid = threadIdx.x, sub = tid & (TXE_LANES - 1u), row = tid / TXE_LANES;
  const uint64_t n_items = (uint64_t)n + n_genomes;
  for (uint64_t i = (uint64_t)blockIdx.x * TXE_WG_RECS + row; i < n_items; i += (uint64_t)gridDim.x * TXE_WG_RECS) {  // (uniform over the row)
    if (i < n) {
      const uint64_t from = perm ? perm[i] : i;
      if (from >= n) continue;  // (never: the sort writes a permutation)
      const uint32_t id = (uint32_t)skey[i], p = parent_in[from], r = rank_in[from];
      uint32_t bad = (id == 0u ? TXE_ERR_TAXID0 : 0u) | (i + 1u < n && skey[i + 1u] == skey[i] ? TXE_ERR_TWICE : 0u) | (r > TXE_RANKS ? TXE_ERR_RANK : 0u);
      uint32_t pr = (uint32_t)i;  // a root is its own parent
      if (p != 0u && p != id) {
        const uint64_t lb = mev_lower_bound(skey, n, p, sub);
        if (lb < n && skey[lb] == p) pr = (uint32_t)lb;
        else bad |= TXE_ERR_PARENT;
      }
      if (sub == 0u) {
        taxid[i] = id;
        prow[i] = pr;
        rank[i] = (uint8_t)(r > TXE_RANKS ? 0u : r);
        if (bad) atomicOr(err, bad);
      }
    } else {
      const uint64_t g = i - n;
      const uint32_t tx = g_taxid[g];
      const uint64_t lb = mev_lower_bound(skey, n, tx, sub);
      const bool found = tx != 0u && lb < n && skey[lb] == tx;
      if (sub == 0u) {
        g_node[g] = found ? (uint32_t)lb : 0u;  // (row 0 stands for a genome that is refused: nothing reads it)
        if (!found) atomicOr(err, TXE_ERR_GENOME_TAXID);
      }
    }
  }
}

// The walk of every node.  A lineage longer than TXE_MAX_DEPTH steps (a cycle is one) and a rank met twice are refusals.
extern "C" __global__ void __launch_bounds__(TXE_BUILD_WG)
k_txe_lineage(const uint32_t* __restrict__ prow, const uint8_t* __restrict__ rank, uint32_t n, uint32_t* __restrict__ depth, uint32_t* __restrict__ anc,
              uint32_t* __restrict__ err) {
  for (uint64_t i = (uint64_t)blockIdx.x * TXE_BUILD_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TXE_BUILD_WG) {
    uint32_t a[TXE_RANKS];
#pragma unroll
    for (uint32_t j = 0; j < TXE_RANKS; j++) a[j] = TXE_NONE;
    uint32_t cur = (uint32_t)i, d = 0u, bad = 0u;
    for (;;) {
      const uint32_t r = rank[cur];
#pragma unroll
      for (uint32_t j = 0; j < TXE_RANKS; j++)
        if (r == j + 1u) {
          if (a[j] == TXE_NONE) a[j] = cur;
          else bad |= TXE_ERR_RANK_TWICE;
        }
      const uint32_t p = prow[cur];
      if (p == cur || p >= n) break;  // (p >= n: never)
      if (d == TXE_MAX_DEPTH) { bad |= TXE_ERR_DEPTH; break; }
      cur = p;
      d++;
    }
    depth[i] = d;
#pragma unroll
    for (uint32_t j = 0; j < TXE_RANKS; j++) anc[i * TXE_RANKS + j] = a[j];
    if (bad) atomicOr(err, bad);
  }
}

// out[0 .. 8): the taxid of the ancestor-or-self at each rank (0: none), out[8] the depth, out[9] whether `taxid` is a node
extern "C" __global__ void __launch_bounds__(TXE_LANES)
k_txe_look(TxeTree T, const uint32_t* __restrict__ node_taxid, uint32_t taxid, uint32_t* __restrict__ out) {
  const uint32_t sub = threadIdx.x & (TXE_LANES - 1u);
  const uint64_t lb = mev_lower_bound(T.key, T.n, taxid, sub);
  const bool found = lb < T.n && T.key[lb] == taxid;
  uint32_t v = 0u;
  if (found && sub < TXE_RANKS) {
    const uint32_t at = T.anc[lb * TXE_RANKS + sub];
    v = at < T.n ? node_taxid[at] : 0u;
  }
  if (found && sub == TXE_RANKS) v = T.depth[lb];
  if (sub == TXE_RANKS + 1u) v = found ? 1u : 0u;
  if (sub < TXE_RANKS + 2u) out[sub] = v;
}

// ---- the truth ------------------------------------------------------------------------------------------------------------------
// cursor[0]: the lines appended so far (never reset between adds), cursor[1]: the largest id
extern "C" __global__ void __launch_bounds__(TXE_WG)
k_txe_truth(MevText W, MevNames N, uint64_t* __restrict__ u_id, uint32_t* __restrict__ u_genome, uint64_t capacity, unsigned long long* __restrict__ cursor,
            unsigned long long* __restrict__ counts, uint32_t* __restrict__ err) {
  __shared__ uint32_t l_cnt[2];  // lines, header lines
  const uint8_t* __restrict__ t = W.text;
  const uint32_t tid = threadIdx.x, sub = tid & (TXE_LANES - 1u), row = tid / TXE_LANES;
  if (tid < 2u) l_cnt[tid] = 0u;
  __syncthreads();
  const uint64_t n_lines = *W.n_lines;
  const uint32_t n = (uint32_t)W.n_bytes;  // (at most SIMMR_FIT_SAM_MAX_BYTES)
  const uint64_t n_batches = (n_lines + TXE_WG_RECS - 1u) / TXE_WG_RECS;
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t li = batch * TXE_WG_RECS + row;
    if (li >= n_lines) continue;  // (uniform over the row)
    const uint32_t line = W.starts[li];
    if (line >= n) continue;      // (never: the index holds places of the text)
    if (sub == 0u) atomicAdd(&l_cnt[0], 1u);
    if (txe_header(t, n, line, sub)) { if (sub == 0u) atomicAdd(&l_cnt[1], 1u); continue; }
    uint32_t tb[3], end;
    const uint32_t n_tab = txe_fields(t, n, line, sub, tb, &end);
    uint64_t id = 0;
    bool ok = n_tab >= 2u && fsam_field_number(t, line, tb[0], false, &id);
    ok = ok && tb[1] - tb[0] == 2u && (uint32_t)t[tb[0] + 1u] - '0' <= 2u;
    uint32_t name = MEV_NO_ROW;
    if (ok) {
      name = mev_name_row(N, t, tb[1] + 1u, n_tab > 2u ? tb[2] : end, sub);
      ok = name != MEV_NO_ROW;
    }
    if (!ok) { if (sub == 0u) atomicOr(err, TXE_ERR_TRUTH); continue; }
    if (sub == 0u) {
      const unsigned long long slot = atomicAdd(cursor, 1ull);
      atomicMax(cursor + 1, (unsigned long long)id);
      if (slot < capacity) {  // (always: an add's lines are fewer than its bytes / TXE_MIN_LINE + 1)
        u_id[slot] = id;
        u_genome[slot] = name;
      }
    }
  }
  __syncthreads();
  if (tid < 2u && l_cnt[tid]) atomicAdd(counts + TC_T_LINES + tid, (unsigned long long)l_cnt[tid]);
}

// The heads of the sorted ids sk[0, n).  e_id == nullptr: a tile's heads are counted into tile_sum.  Otherwise, behind the scan: the
// entry of every head — its id, its genome row and the lines behind it (perm == nullptr: the order is the identity).  Two lines of
// one id must name one genome; a third line is a refusal.
extern "C" __global__ void __launch_bounds__(256)
k_txe_heads(const uint64_t* __restrict__ sk, const uint32_t* __restrict__ perm, uint64_t n, uint64_t n_tiles, uint64_t* __restrict__ tile_sum,
            const uint64_t* __restrict__ tile_prefix, const uint32_t* __restrict__ u_genome, uint64_t* __restrict__ e_id, uint32_t* __restrict__ e_genome,
            uint32_t* __restrict__ e_mates, uint32_t* __restrict__ err) {
  __shared__ uint32_t lds[256];
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // (uniform over the workgroup)
    const uint64_t i = tile * TXE_HEAD_TILE + threadIdx.x;
    const uint32_t head = i < n && (i == 0u || sk[i] != sk[i - 1u]) ? 1u : 0u;
    uint32_t total;
    const uint32_t ex = sam_wg_scan<uint32_t>(head, lds, &total);
    if (!e_id) {
      if (threadIdx.x == 0) tile_sum[tile] = total;
      continue;
    }
    if (!head) continue;
    const uint64_t at = tile_prefix[tile] + ex;
    if (at >= n) continue;  // (never: the heads are at most the ids)
    const uint64_t from = perm ? perm[i] : i;
    const uint32_t g = from < n ? u_genome[from] : 0u;
    uint32_t m = 1u, bad = 0u;
    if (i + 1u < n && sk[i + 1u] == sk[i]) {
      m = 2u;
      const uint64_t from2 = perm ? perm[i + 1u] : i + 1u;
      if (from2 < n && u_genome[from2] != g) bad |= TXE_ERR_GENOMES;
      if (i + 2u < n && sk[i + 2u] == sk[i]) bad |= TXE_ERR_MATES;
    }
    e_id[at] = sk[i];
    e_genome[at] = g;
    e_mates[at] = m;
    if (bad) atomicOr(err, bad);
  }
}

// ---- the candidate records --------------------------------------------------------------------------------------------------------
// One more for the count `which` (0 true, 1 called, 2 both) of node `row`: into the workgroup's LDS table where its slot or one of
// the next few holds that (count, row) or is free, straight to HBM otherwise.
SIMMR_DEV void txe_bump(uint32_t* l_key, uint32_t* l_sum, uint32_t which, uint32_t row, unsigned long long* __restrict__ node_counts, uint32_t n_nodes) {
  const uint32_t tag = (which << TXE_ROW_BITS | row) + 1u;  // (0: a free slot)
  const uint32_t first = (tag * 2654435761u) >> 23;         // 9 bits
  for (uint32_t k = 0; k < TXE_HOT_PROBES; k++) {
    const uint32_t s = (first + k) & (TXE_HOT_SLOTS - 1u);
    const uint32_t old = atomicCAS(&l_key[s], 0u, tag);
    if (old == 0u || old == tag) { atomicAdd(&l_sum[s], 1u); return; }
  }
  atomicAdd(node_counts + (uint64_t)which * n_nodes + row, 1ull);
}

// node_counts: [3][n_nodes] — true, called, both
extern "C" __global__ void __launch_bounds__(TXE_WG)
k_txe_record(MevText W, TxeEntries E, TxeTree T, const uint32_t* __restrict__ g_node, unsigned long long* __restrict__ counts,
             unsigned long long* __restrict__ by_rank, unsigned long long* __restrict__ node_counts, uint32_t* __restrict__ seen, uint32_t* __restrict__ hits,
             uint32_t* __restrict__ err) {
  __shared__ uint32_t l_cnt[TXE_REC_COUNTS];
  __shared__ uint32_t l_rank[TXE_RANK_WORDS];
  __shared__ uint32_t l_key[TXE_HOT_SLOTS];
  __shared__ uint32_t l_sum[TXE_HOT_SLOTS];
  const uint8_t* __restrict__ t = W.text;
  const uint32_t tid = threadIdx.x, sub = tid & (TXE_LANES - 1u), row = tid / TXE_LANES;
  if (tid < TXE_REC_COUNTS) l_cnt[tid] = 0u;
  if (tid < TXE_RANK_WORDS) l_rank[tid] = 0u;
  for (uint32_t i = tid; i < TXE_HOT_SLOTS; i += TXE_WG) { l_key[i] = 0u; l_sum[i] = 0u; }
  __syncthreads();
#define TXE_COUNT(which) do { if (sub == 0u) atomicAdd(&l_cnt[(which) - TC_LINES], 1u); } while (0)
  const uint32_t n = (uint32_t)W.n_bytes;        // (at most SIMMR_FIT_SAM_MAX_BYTES)
  const uint32_t n_lines = (uint32_t)*W.n_lines;  // (a line start per two bytes at the most: below 2^31)
  const uint32_t n_batches = (n_lines + TXE_WG_RECS - 1u) / TXE_WG_RECS;
  for (uint32_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint32_t li = batch * TXE_WG_RECS + row;
    if (li >= n_lines) continue;  // (uniform over the row)
    const uint32_t line = W.starts[li];
    if (line >= n) continue;      // (never)
    TXE_COUNT(TC_LINES);
    if (txe_header(t, n, line, sub)) { TXE_COUNT(TC_HEADER); continue; }
    uint32_t tb[3], end;
    const uint32_t n_tab = txe_fields(t, n, line, sub, tb, &end);
    uint64_t taxid = 0;
    bool ok = n_tab >= 2u && tb[0] - line == 1u && (t[line] == 'C' || t[line] == 'U');
    ok = ok && txe_taxon(t, tb[1] + 1u, n_tab > 2u ? tb[2] : end, &taxid);
    if (!ok) { if (sub == 0u) atomicOr(err, TXE_ERR_CAND); continue; }
    TXE_COUNT(TC_RECORDS);
    // 1. the read
    uint64_t id = 0, entry = E.n;
    bool known = txe_read_id(t, tb[0] + 1u, tb[1], &id);
    if (known) {
      entry = mev_lower_bound(E.id, E.n, id, sub);
      known = entry < E.n && E.id[entry] == id;
    }
    if (!known) { TXE_COUNT(TC_UNKNOWN_READ); continue; }
    const uint32_t tn = g_node[E.genome[entry]];
    // 2. unclassified, 3. a taxid that is no node, 4. scored
    uint32_t kind = 1u, cn = 0u, lca = TXE_NONE;
    if (t[line] == 'C' && taxid != 0u) {
      const uint64_t lb = mev_lower_bound(T.key, T.n, taxid, sub);
      kind = lb < T.n && T.key[lb] == taxid ? 3u : 2u;
      if (kind == 3u) {
        cn = (uint32_t)lb;
        lca = txe_lca(T, tn, cn);
      }
    }
    TXE_COUNT(kind == 1u ? TC_UNCLASSIFIED : kind == 2u ? TC_UNKNOWN_TAXON : TC_SCORED);
    // the class of rank sub + 1
    uint32_t bit = 0u;
    if (sub < TXE_RANKS) {
      const uint32_t at = T.anc[(uint64_t)tn * TXE_RANKS + sub];
      uint32_t cls = 0u;
      if (at != TXE_NONE) {
        cls = kind;  // 1 unclassified, 2 wrong
        if (kind == 3u) {
          const uint32_t ac = T.anc[(uint64_t)cn * TXE_RANKS + sub];
          cls = ac != TXE_NONE ? (ac == at ? 4u : 2u) : (lca == cn ? 3u : 2u);
        }
      }
      atomicAdd(&l_rank[sub * TXE_CLASSES + cls], 1u);
      bit = cls ? 1u << (4u * sub + cls - 1u) : 0u;
    }
    bit = fsam_row_or(bit);
    if (sub == 0u) {
      atomicAdd(hits + entry, 1u);
      if (bit) atomicOr(seen + entry, bit);
      txe_bump(l_key, l_sum, 0u, tn, node_counts, T.n);
      if (kind == 3u) {
        txe_bump(l_key, l_sum, 1u, cn, node_counts, T.n);
        if (lca != TXE_NONE) txe_bump(l_key, l_sum, 2u, lca, node_counts, T.n);
      }
    }
  }
#undef TXE_COUNT
  __syncthreads();
  if (tid < TXE_REC_COUNTS && l_cnt[tid]) atomicAdd(counts + TC_LINES + tid, (unsigned long long)l_cnt[tid]);
  if (tid < TXE_RANK_WORDS && l_rank[tid]) atomicAdd(by_rank + tid, (unsigned long long)l_rank[tid]);
  for (uint32_t s = tid; s < TXE_HOT_SLOTS; s += TXE_WG) {
    const uint32_t k = l_key[s];
    if (k == 0u) continue;
    const uint32_t which = (k - 1u) >> TXE_ROW_BITS, at = (k - 1u) & ((1u << TXE_ROW_BITS) - 1u);
    if (which < 3u && at < T.n) atomicAdd(node_counts + (uint64_t)which * T.n + at, (unsigned long long)l_sum[s]);  // (always)
  }
}

// ---- the entries by the best class of their records -------------------------------------------------------------------------------
// l_sum: paired, missing, multiple, then reads_by_rank's 8 x 5 words (the entries are fewer than 2^31: no word overflows)
extern "C" __global__ void __launch_bounds__(256)
k_txe_reduce(TxeEntries E, const uint32_t* __restrict__ g_node, const uint32_t* __restrict__ anc, const uint32_t* __restrict__ seen,
             const uint32_t* __restrict__ hits, unsigned long long* __restrict__ counts, unsigned long long* __restrict__ reads_by_rank) {
  __shared__ uint32_t l_sum[3u + TXE_RANK_WORDS];
  for (uint32_t i = threadIdx.x; i < 3u + TXE_RANK_WORDS; i += 256u) l_sum[i] = 0u;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < E.n; i += (uint64_t)gridDim.x * 256u) {
    const uint32_t h = hits[i], s = seen[i], m = E.mates[i];
    const uint64_t tn = g_node[E.genome[i]];
    if (m == 2u) atomicAdd(&l_sum[0], 1u);
    if (h == 0u) atomicAdd(&l_sum[1], 1u);
    if (h > m) atomicAdd(&l_sum[2], 1u);
#pragma unroll
    for (uint32_t r = 0; r < TXE_RANKS; r++) {
      const uint32_t nib = (s >> (4u * r)) & 15u;
      const uint32_t cls = h == 0u ? (anc[tn * TXE_RANKS + r] != TXE_NONE ? 1u : 0u) : nib ? 32u - (uint32_t)__builtin_clz(nib) : 0u;
      atomicAdd(&l_sum[3u + r * TXE_CLASSES + cls], 1u);
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < 3u + TXE_RANK_WORDS; k += 256u) {
    const uint32_t v = l_sum[k];
    if (v) atomicAdd(k < 3u ? counts + (k == 0u ? TC_T_PAIRED : TC_MISSING + (k - 1u)) : reads_by_rank + (k - 3u), (unsigned long long)v);
  }
}

// ---- the clade sums ---------------------------------------------------------------------------------------------------------------
// clade[w][x] += direct[w][i] for every x on the path from node i to its root, i included.  direct[] is only read.
extern "C" __global__ void __launch_bounds__(TXE_BUILD_WG)
k_txe_rollup(const unsigned long long* __restrict__ direct, unsigned long long* __restrict__ clade, const uint32_t* __restrict__ prow, uint32_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * TXE_BUILD_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TXE_BUILD_WG) {
    const unsigned long long v0 = direct[i], v1 = direct[(uint64_t)n + i], v2 = direct[2ull * n + i];
    if ((v0 | v1 | v2) == 0ull) continue;
    uint32_t cur = (uint32_t)i;
    for (uint32_t d = 0; d <= TXE_MAX_DEPTH; d++) {
      if (v0) atomicAdd(clade + cur, v0);
      if (v1) atomicAdd(clade + (uint64_t)n + cur, v1);
      if (v2) atomicAdd(clade + 2ull * n + cur, v2);
      const uint32_t p = prow[cur];
      if (p == cur || p >= n) break;  // (p >= n: never)
      cur = p;
    }
  }
}

}  // namespace simmr
