// bineval_kernels.hip — a binner's contig bins scored against each contig's true genome (gfx950): two tab-separated texts in HBM to
// integer tables (include/simmr_hip.h states every rule: the texts, the names, what is malformed, the join, the assignment, the bin
// rows, the cells, the tables).  Included by bineval.hip alone, a translation unit of its own.  The reader's routines are taken, not
// restated: the line index and the scans of fit_sam_kernels.hip / sam_kernels.hip and the name row of mapeval_kernels.hip, through
// MEV_ROUTINES_ONLY (which brings FSAM_ROUTINES_ONLY with it).
//
// An add of either side is: index (count) -> scan -> index (write) -> lines -> chunks -> write.
//   k_bin_index        fsam_index_tiles: launched to count a tile's line starts and, after the scan, to write them.
//   k_bin_scan         ONE workgroup: sam_scan_chunks over the tile counts; the entry behind the last tile is the number of lines.
//   k_bin_lines        a line a thread, BIN_CHUNK lines a workgroup and trip (bin_parse: the fields, the numbers, the names'
//                      bytes): what it found goes to a 16-byte entry a line, and a chunk's sum (records << 32 | the bytes of the
//                      names the object keeps) to the scan.
//   k_bin_truth_write / k_bin_cand_write   behind k_bin_chunks, the same lines from their entries.  Truth: the contig's name into
//                      the object's pool, its offset, length, hash and bases, and where the genome field lies.  Candidate: THE
//                      LOOKUP (bin_find) of the contig's name, read from the caller's text, among the truth's; the record's
//                      contig; the contig's first record by a 32-bit atomicMin and its records by atomicAdd; the bin's name into
//                      the pool with its offset, length and hash.
//   k_bin_chunks       ONE workgroup: sam_scan_chunks over the chunk sums; the add's base (records, pool bytes) is the truth's
//                      device cursor, which it moves on, or what the host knows of the candidate side.
//   k_bin_genomes      truth only, a record per 16 lanes: the genome field among the sorted names (mev_name_row), or "." = none.
//   k_bin_keys         a sort's keys: the hashes cut to their low hash_bits bits (the sort works in whole 8-bit digits).
//   k_bin_iota         the identity order, where a sort over no bits launches nothing.
//   k_bin_truth_dups   behind samsort_sort_pairs over the low hash_bits bits: a name equal to an earlier one of its run.
//   k_bin_reps         behind the sort of the records by the bin name's hash: every known record searches the first place of its
//                      run of equal truncated hash and walks it forwards to the first known record whose bin name has its bytes
//                      (full hash, length, then bytes): the sort is stable, so that is the lowest ordinal, the representative.  A representative flags its own ordinal; the engine's scan of the flags ranks them.
//   k_bin_rows         a record's bin row = the flags in front of its representative; a representative writes first_record.
//   k_bin_assign       per truth contig: its bin row (that of its first record) and the cell key bin << 24 | genome; a contig
//                      without a record gets bin = n_bins, which sorts behind every cell.
//   k_bin_cell_heads   1 where a sorted cell key of a real bin differs from the one before it: the input of the engine's scan.
//   k_bin_cell_sum     the segmented sums over the sorted order: contigs and bases of every cell.
//   k_bin_truth_rows   per truth contig: the genome row's truth and the counts of the assignment.
//   k_bin_cell_tables  per cell, launched twice.  Phase 0: the bin's and the genome row's sums, the largest bases of a real genome
//                      in the bin and of a bin in the genome (64-bit atomicMax of the bases alone, so no width is given away to a
//                      row).  Phase 1: a cell that holds the largest bases names its row by a 32-bit atomicMin: ties go to the
//                      lowest row.
//   k_bin_finish       per bin and per genome row: the sums over them, the pair sums, the six classes, by_genome's last columns.
// Bounds.  Every load of text is below n_bytes: a line is [starts[li], its end) with the end at most the next line's start or
// n_bytes.  A truth row and its name are stored below capacities the host derived from the bytes of the truth adds (a record has
// 16 bytes or more, a name fewer bytes than its line); a candidate record and its bin name below capacities the host made after it
// had read the add's totals.  A lookup's result is an index of the sorted order, below the truth's contigs; rep, the bin rows and
// the cells are indexed by scan results below the totals the scans gave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#define MEV_ROUTINES_ONLY
#include "mapeval_kernels.hip"  // mev_name_row, MevNames, MevText; through it the line index, the scans and the ballots

namespace simmr {

#define BIN_WG 256u
#define BIN_CHUNK 256u        /* lines per workgroup and trip of the line kernels: a line a thread */
#define BIN_WG_RECS 16u       /* records per workgroup and batch of k_bin_genomes */
#define BIN_NAME_MAX 254u     /* longest contig or bin name */
#define BIN_GENOME_BITS 24u   /* a cell's key is bin << 24 | genome */
#define BIN_NONE 0xffffffffu
#define BIN_ERR_TRUTH 1u      /* a malformed truth text */
#define BIN_ERR_CAND 2u       /* a malformed candidate text */
#define BIN_ERR_DUP 4u        /* a contig name twice in the truth */
static_assert(BIN_CHUNK == BIN_WG && BIN_WG == 256u, "sam_wg_scan is over 256 threads");
static_assert(BIN_WG_RECS * MEV_LANES == BIN_WG, "a record per group of the name search");
static_assert(BIN_NAME_MAX == SAM_RNAME_MAX, "one name limit on both sides of the join");

enum { BC_T_RECORDS = 0, BC_T_BASES, BC_T_NONE, BC_RECORDS, BC_UNKNOWN, BC_REPEATED, BC_ASSIGNED, BC_ASSIGNED_BASES, BC_BINS, BC_CELLS,
       BC_SUM_TOP, BC_SUM_BEST, BC_PAIRS_CELLS, BC_PAIRS_BINS, BC_PAIRS_GENOMES, BC_C90_X5, BC_C70_X5, BC_C50_X5, BC_C90_X10, BC_C70_X10,
       BC_C50_X10, BC_COUNT };
static_assert(sizeof(simmr_bineval_counts) == BC_COUNT * 8u, "the counts in the header's order");
#define BIN_GENOME_COLS 7u    /* truth_contigs, truth_bases, assigned_contigs, assigned_bases, bins, best_bin, best_bases */
static_assert(SIMMR_BINEVAL_GENOME_COLS == BIN_GENOME_COLS, "the header's table");
static_assert(SIMMR_BINEVAL_FNV_OFFSET == 0xcbf29ce484222325ull && SIMMR_BINEVAL_FNV_PRIME == 0x100000001b3ull, "64-bit FNV-1a");

struct BinTot {  // what k_bin_chunks leaves of one add (64-bit words)
  uint64_t lines, bytes, records, base_records, base_bytes;
};

struct BinNames {  // names the object keeps: the truth's contigs, or the candidate records' bins
  uint8_t* pool;
  uint64_t* off;
  uint32_t* len;
  uint64_t* hash;
  uint64_t rows, bytes;  // the capacities
};

struct BinIndex {  // the truth's contigs in the order of the low bits of their hash
  const uint64_t* skey;  // the truncated hashes in that order
  const uint32_t* sidx;  // the contig at each place
  const uint8_t* pool;
  const uint64_t* off;
  const uint32_t* len;
  const uint64_t* hash;  // the full hashes, by contig
  uint32_t n;
  uint64_t mask;         // the low hash_bits bits
};

struct BinLine {  // a line as a thread reads it
  uint32_t kind;      // 0: no record, 1: a record, 2: malformed
  uint32_t a, a_len;  // the contig's name
  uint32_t b, b_len;  // truth: the genome field; candidate: the bin's name
  uint64_t length;    // truth: field 2
};

struct BinBins {  // the bin rows of a read
  uint32_t* contigs;
  uint32_t* real;       // the contigs of a real genome
  uint64_t* bases;
  uint64_t* none_bases;
  uint32_t* first_record;
  uint32_t* top_genome;
  unsigned long long* top_bases;
};

struct BinCells {  // the cells of a read in (bin, genome) order
  uint32_t* bin;
  uint32_t* genome;
  uint32_t* contigs;
  unsigned long long* bases;
};

SIMMR_DEV uint64_t bin_hash(const uint8_t* __restrict__ t, uint32_t a, uint32_t len) {
  uint64_t h = SIMMR_BINEVAL_FNV_OFFSET;
  for (uint32_t i = 0; i < len; i++) h = (h ^ t[a + i]) * SIMMR_BINEVAL_FNV_PRIME;
  return h;
}

// 1 to 254 bytes, none of them a tab, a blank or a control byte
SIMMR_DEV bool bin_name_ok(const uint8_t* __restrict__ t, uint32_t a, uint32_t len) {
  if (len == 0u || len > BIN_NAME_MAX) return false;
  for (uint32_t i = 0; i < len; i++) {
    const uint32_t c = t[a + i];
    if (c <= 0x20u || c == 0x7fu) return false;
  }
  return true;
}

// the first tab of [p, e), or e
SIMMR_DEV uint32_t bin_field_end(const uint8_t* __restrict__ t, uint32_t p, uint32_t e) {
  while (p < e && t[p] != '\t') p++;
  return p;
}

// The line [s, nxt) (byte s is no '\n'; nxt is the next line's start or the text's end).
SIMMR_DEV BinLine bin_parse(const uint8_t* __restrict__ t, uint32_t s, uint32_t nxt, bool truth) {
  BinLine L{};
  uint32_t e = nxt;
  while (e > s + 1u && t[e - 1u] == '\n') e--;
  if (e < nxt && e > s && t[e - 1u] == '\r') e--;
  if (e == s) return L;  // (a '\r' alone before its '\n')
  const uint32_t c0 = t[s];
  if (c0 == '#' || (!truth && c0 == '@')) return L;
  L.kind = 2u;
  uint32_t p = bin_field_end(t, s, e);
  L.a = s;
  L.a_len = p - s;
  if (p == e || !bin_name_ok(t, s, L.a_len)) return L;  // (no second field, or no name)
  if (truth) {
    for (uint32_t f = 2u; f <= 7u; f++) {
      const uint32_t q = p + 1u;
      p = bin_field_end(t, q, e);
      uint64_t v;
      if (p == e || !fsam_field_number(t, q, p, false, &v)) return L;  // (fewer than eight fields, or no number)
      if (f == 2u) L.length = v;
    }
  }
  L.b = p + 1u;
  L.b_len = bin_field_end(t, L.b, e) - L.b;
  if (truth ? L.b_len == 0u || L.b_len > BIN_NAME_MAX : !bin_name_ok(t, L.b, L.b_len)) return L;  // (both lengths fit the entry's bytes)
  L.kind = 1u;
  return L;
}

SIMMR_DEV bool bin_bytes_equal(const uint8_t* __restrict__ x, const uint8_t* __restrict__ y, uint32_t len) {
  for (uint32_t i = 0; i < len; i++)
    if (x[i] != y[i]) return false;
  return true;
}

// THE LOOKUP.  The truth contig whose name is name[0, len) with hash h (BIN_NONE: none).  A binary search for the first place of
// the run whose truncated hash is h's, then a walk of the run: the hash only narrows the search, byte equality decides the answer.
SIMMR_DEV uint32_t bin_find(const BinIndex& X, const uint8_t* __restrict__ name, uint32_t len, uint64_t h) {
  const uint64_t hm = h & X.mask;
  uint32_t lo = 0, hi = X.n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (X.skey[mid] < hm) lo = mid + 1u;
    else hi = mid;
  }
  for (uint32_t j = lo; j < X.n && X.skey[j] == hm; j++) {
    const uint32_t i = X.sidx[j];
    if (X.hash[i] == h && X.len[i] == len && bin_bytes_equal(X.pool + X.off[i], name, len)) return i;
  }
  return BIN_NONE;
}

SIMMR_DEV unsigned long long bin_wave_sum(unsigned long long v) {
  for (uint32_t d = 1; d < 64u; d <<= 1) v += __shfl_xor(v, (int)d, 64);
  return v;
}
// adds the wave's sum of v to *at (every lane of the wave calls it)
SIMMR_DEV void bin_wave_add(unsigned long long* at, unsigned long long v) {
  const unsigned long long s = bin_wave_sum(v);
  if ((threadIdx.x & 63u) == 0u && s) atomicAdd(at, s);
}

SIMMR_DEV unsigned long long bin_pairs(unsigned long long n) { return n * (n - (n ? 1ull : 0ull)) / 2ull; }

// ---- the line index -----------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_bin_index(const uint8_t* __restrict__ text, uint64_t n_bytes, uint64_t n_tiles, uint64_t* __restrict__ tile_sum,
            const uint64_t* __restrict__ tile_prefix, uint32_t* __restrict__ starts, uint64_t start_capacity) {
  __shared__ uint32_t lds[FSAM_WG];
  fsam_index_tiles(text, n_bytes, n_tiles, tile_sum, tile_prefix, starts, start_capacity, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_bin_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

// ---- the lines of either side ----------------------------------------------------------------------------------------------------
// info[li] = what bin_parse found (bin_info); chunk_sum[c] = records << 32 | the name bytes the object keeps of chunk c (truth: the
// contigs' names; candidate: the bins'); the error bit for a malformed line
extern "C" __global__ void __launch_bounds__(BIN_WG)
k_bin_lines(MevText W, uint64_t line_capacity, uint32_t truth, uint64_t* __restrict__ chunk_sum, uint4* __restrict__ info, uint32_t* __restrict__ err,
            uint32_t err_bit) {
  __shared__ uint64_t lds[BIN_WG];
  const uint8_t* __restrict__ t = W.text;
  const uint32_t n_lines = (uint32_t)(*W.n_lines < line_capacity ? *W.n_lines : line_capacity);  // (a line per two bytes: below 2^30)
  const uint32_t n_chunks = (n_lines + BIN_CHUNK - 1u) / BIN_CHUNK;
  for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // (uniform over the workgroup)
    const uint32_t li = chunk * BIN_CHUNK + threadIdx.x;
    BinLine L{};
    if (li < n_lines) {
      L = bin_parse(t, W.starts[li], li + 1u < n_lines ? W.starts[li + 1u] : (uint32_t)W.n_bytes, truth != 0u);
      info[li] = uint4{L.b, L.a_len | L.b_len << 8 | L.kind << 16, (uint32_t)L.length, (uint32_t)(L.length >> 32)};
      if (L.kind == 2u) atomicOr(err, err_bit);
    }
    uint64_t total;
    sam_wg_scan<uint64_t>(L.kind == 1u ? 1ull << 32 | (truth ? L.a_len : L.b_len) : 0ull, lds, &total);
    if (threadIdx.x == 0) chunk_sum[chunk] = total;
  }
}

// the line li as k_bin_lines left it (the contig's name begins the line)
SIMMR_DEV BinLine bin_info(const uint4* __restrict__ info, uint32_t li, uint32_t start) {
  const uint4 v = info[li];
  BinLine L{};
  L.kind = v.y >> 16;
  L.a = start;
  L.a_len = v.y & 0xffu;
  L.b = v.x;
  L.b_len = (v.y >> 8) & 0xffu;
  L.length = (uint64_t)v.w << 32 | v.z;
  return L;
}

// ---- the rows of the truth -------------------------------------------------------------------------------------------------------
// behind k_bin_chunks.  rec_field[2 r], rec_field[2 r + 1]: where the genome field of the add's record r begins and ends.
extern "C" __global__ void __launch_bounds__(BIN_WG)
k_bin_truth_write(MevText W, uint64_t line_capacity, const uint64_t* __restrict__ chunk_prefix, const uint4* __restrict__ info,
                  const BinTot* __restrict__ tot, BinNames T, uint64_t* __restrict__ t_length, uint32_t* __restrict__ rec_field) {
  __shared__ uint64_t lds[BIN_WG];
  const uint8_t* __restrict__ t = W.text;
  const uint32_t n_lines = (uint32_t)(*W.n_lines < line_capacity ? *W.n_lines : line_capacity);
  const uint32_t n_chunks = (n_lines + BIN_CHUNK - 1u) / BIN_CHUNK;
  for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // (uniform over the workgroup)
    const uint32_t li = chunk * BIN_CHUNK + threadIdx.x;
    BinLine L{};
    if (li < n_lines) L = bin_info(info, li, W.starts[li]);
    const bool rec = L.kind == 1u;
    uint64_t total;
    const uint64_t ex = sam_wg_scan<uint64_t>(rec ? 1ull << 32 | L.a_len : 0ull, lds, &total);
    if (!rec) continue;
    const uint64_t at = chunk_prefix[chunk] + ex;
    const uint64_t r_add = at >> 32, r = tot->base_records + r_add, off = tot->base_bytes + (uint32_t)at;
    if (r >= T.rows || off + L.a_len > T.bytes) continue;  // (never: the capacities come from the adds' bytes)
    T.off[r] = off;
    T.len[r] = L.a_len;
    T.hash[r] = bin_hash(t, L.a, L.a_len);
    t_length[r] = L.length;
    rec_field[2u * r_add] = L.b;
    rec_field[2u * r_add + 1u] = L.b + L.b_len;
    for (uint32_t i = 0; i < L.a_len; i++) T.pool[off + i] = t[L.a + i];
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_bin_chunks(const uint64_t* __restrict__ n_lines_p, uint64_t line_capacity, const uint64_t* __restrict__ chunk_sum, uint64_t* __restrict__ chunk_prefix,
             BinTot* __restrict__ tot, unsigned long long* __restrict__ cursor, unsigned long long base_records, unsigned long long base_bytes) {
  __shared__ uint64_t lds[256];
  const uint64_t n_lines = *n_lines_p < line_capacity ? *n_lines_p : line_capacity;
  const uint64_t n_chunks = (n_lines + BIN_CHUNK - 1u) / BIN_CHUNK;
  sam_scan_chunks(chunk_sum, chunk_prefix, n_chunks, lds);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t all = chunk_prefix[n_chunks];
    tot->lines = n_lines;
    tot->bytes = (uint32_t)all;
    tot->records = all >> 32;
    tot->base_records = cursor ? cursor[0] : base_records;
    tot->base_bytes = cursor ? cursor[1] : base_bytes;
    if (cursor) {
      cursor[0] += all >> 32;
      cursor[1] += (uint32_t)all;
    }
  }
}

// ---- the genome of every truth record -----------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(BIN_WG)
k_bin_genomes(MevText W, const BinTot* __restrict__ tot, const uint32_t* __restrict__ rec_field, MevNames N, uint32_t* __restrict__ t_genome,
              uint64_t row_capacity, uint32_t* __restrict__ err) {
  const uint8_t* __restrict__ t = W.text;
  const uint64_t n_rec = tot->records, base = tot->base_records;
  const uint32_t sub = threadIdx.x & (MEV_LANES - 1u), row = threadIdx.x / MEV_LANES;
  const uint64_t n_batches = (n_rec + BIN_WG_RECS - 1u) / BIN_WG_RECS;
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t r = batch * BIN_WG_RECS + row;
    if (r >= n_rec || base + r >= row_capacity) continue;  // (uniform over the row)
    const uint32_t a = rec_field[2u * r], b = rec_field[2u * r + 1u];
    uint32_t g = N.n;
    if (!(b - a == 1u && t[a] == '.')) {
      g = mev_name_row(N, t, a, b, sub);
      if (g == MEV_NO_ROW) {
        g = N.n;
        if (sub == 0u) atomicOr(err, BIN_ERR_TRUTH);
      }
    }
    if (sub == 0u) t_genome[base + r] = g;
  }
}

// ---- the records of the candidate ------------------------------------------------------------------------------------------------
// behind k_bin_chunks: the lookup and the record's columns
extern "C" __global__ void __launch_bounds__(BIN_WG)
k_bin_cand_write(MevText W, uint64_t line_capacity, const uint64_t* __restrict__ chunk_prefix, const uint4* __restrict__ info,
                 const BinTot* __restrict__ tot, BinIndex X, BinNames B, uint32_t* __restrict__ r_contig, uint32_t* __restrict__ t_first,
                 uint32_t* __restrict__ t_records, unsigned long long* __restrict__ unknown) {
  __shared__ uint64_t lds[BIN_WG];
  const uint8_t* __restrict__ t = W.text;
  const uint32_t n_lines = (uint32_t)(*W.n_lines < line_capacity ? *W.n_lines : line_capacity);
  const uint32_t n_chunks = (n_lines + BIN_CHUNK - 1u) / BIN_CHUNK;
  for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // (uniform over the workgroup)
    const uint32_t li = chunk * BIN_CHUNK + threadIdx.x;
    BinLine L{};
    if (li < n_lines) L = bin_info(info, li, W.starts[li]);
    const bool rec = L.kind == 1u;
    uint64_t total;
    const uint64_t ex = sam_wg_scan<uint64_t>(rec ? 1ull << 32 | L.b_len : 0ull, lds, &total);
    uint32_t miss = 0;
    if (rec) {
      const uint64_t at = chunk_prefix[chunk] + ex;
      const uint64_t o = tot->base_records + (at >> 32), off = tot->base_bytes + (uint32_t)at;
      if (o < B.rows && off + L.b_len <= B.bytes) {  // (always: the host made room after it had read the add's totals)
        const uint32_t c = bin_find(X, t + L.a, L.a_len, bin_hash(t, L.a, L.a_len));
        r_contig[o] = c;
        if (c != BIN_NONE) {
          atomicMin(t_first + c, (uint32_t)o);
          atomicAdd(t_records + c, 1u);
        } else {
          miss = 1u;
        }
        B.off[o] = off;
        B.len[o] = L.b_len;
        B.hash[o] = bin_hash(t, L.b, L.b_len);
        for (uint32_t i = 0; i < L.b_len; i++) B.pool[off + i] = t[L.b + i];
      }
    }
    bin_wave_add(unknown, miss);
  }
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
// the sort's keys: the low bits of the hashes, so that a sort in whole digits orders by these bits alone
extern "C" __global__ void __launch_bounds__(256)
k_bin_keys(const uint64_t* __restrict__ hash, uint64_t mask, uint64_t n, uint64_t* __restrict__ key) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u) key[j] = hash[j] & mask;
}

extern "C" __global__ void __launch_bounds__(256)
k_bin_iota(uint32_t* __restrict__ idx, uint64_t n) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u) idx[j] = (uint32_t)j;
}

extern "C" __global__ void __launch_bounds__(256)
k_bin_truth_dups(BinIndex X, uint32_t* __restrict__ err) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < X.n; j += (uint64_t)gridDim.x * 256u) {
    const uint64_t run = X.skey[j];
    const uint32_t me = X.sidx[j], len = X.len[me];
    const uint64_t h = X.hash[me];
    for (uint64_t i = j; i > 0u;) {
      i--;
      if (X.skey[i] != run) break;
      const uint32_t o = X.sidx[i];
      if (X.hash[o] == h && X.len[o] == len && bin_bytes_equal(X.pool + X.off[o], X.pool + X.off[me], len)) {
        atomicOr(err, BIN_ERR_DUP);
        break;
      }
    }
  }
}

// ---- the bin rows ------------------------------------------------------------------------------------------------------------------
// flag is zeroed before.  skey / sidx: the records in the order of the low bits of their bin name's hash (a stable sort: inside a
// run the ordinals ascend).
extern "C" __global__ void __launch_bounds__(256)
k_bin_reps(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ r_contig, BinNames B, uint64_t n,
           uint32_t* __restrict__ rep, uint32_t* __restrict__ flag) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u) {
    const uint32_t me = sidx[j];
    if (me >= n) continue;  // (never: the sort writes a permutation)
    if (r_contig[me] == BIN_NONE) { rep[me] = BIN_NONE; continue; }
    const uint64_t run = skey[j], h = B.hash[me];
    const uint32_t len = B.len[me];
    uint64_t lo = 0, hi = j;  // the run's first place: the keys ascend
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2u;
      if (skey[mid] < run) lo = mid + 1u;
      else hi = mid;
    }
    uint32_t best = me;
    for (uint64_t i = lo; i < j; i++) {  // the ordinals ascend inside the run: the first match is the lowest
      const uint32_t o = sidx[i];
      if (o < n && r_contig[o] != BIN_NONE && B.hash[o] == h && B.len[o] == len && bin_bytes_equal(B.pool + B.off[o], B.pool + B.off[me], len)) {
        best = o;
        break;
      }
    }
    rep[me] = best;
    if (best == me) flag[me] = 1u;
  }
}

// before[o] = the flags in front of ordinal o
extern "C" __global__ void __launch_bounds__(256)
k_bin_rows(const uint32_t* __restrict__ rep, const uint64_t* __restrict__ before, uint64_t n, uint64_t n_bins, uint32_t* __restrict__ rec_bin,
           uint32_t* __restrict__ first_record) {
  for (uint64_t o = (uint64_t)blockIdx.x * 256u + threadIdx.x; o < n; o += (uint64_t)gridDim.x * 256u) {
    const uint32_t r = rep[o];
    const uint64_t b = r < n ? before[r] : n_bins;
    rec_bin[o] = b < n_bins ? (uint32_t)b : BIN_NONE;
    if (r == o && b < n_bins) first_record[b] = (uint32_t)o;
  }
}

// ---- the cells ---------------------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
k_bin_assign(const uint32_t* __restrict__ t_first, const uint32_t* __restrict__ t_genome, const uint32_t* __restrict__ rec_bin, uint64_t n_truth,
             uint64_t n_records, uint32_t n_bins, uint64_t* __restrict__ key, uint32_t* __restrict__ t_bin) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_truth; i += (uint64_t)gridDim.x * 256u) {
    const uint32_t f = t_first[i];
    const uint32_t b = f < n_records ? rec_bin[f] : BIN_NONE;
    t_bin[i] = b;
    key[i] = (uint64_t)(b < n_bins ? b : n_bins) << BIN_GENOME_BITS | t_genome[i];
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_bin_cell_heads(const uint64_t* __restrict__ skey, uint64_t n, uint32_t n_bins, uint32_t* __restrict__ head) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u)
    head[j] = (skey[j] >> BIN_GENOME_BITS) < n_bins && (j == 0u || skey[j] != skey[j - 1u]) ? 1u : 0u;
}

// contigs and bases are zeroed before; before[j] = the heads in front of j
extern "C" __global__ void __launch_bounds__(256)
k_bin_cell_sum(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ sidx, const uint64_t* __restrict__ t_length, const uint64_t* __restrict__ before,
               uint64_t n, uint32_t n_bins, uint64_t n_cells, BinCells C) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u) {
    const uint64_t key = skey[j];
    if ((key >> BIN_GENOME_BITS) >= n_bins) continue;  // (a contig without a record)
    const bool head = j == 0u || key != skey[j - 1u];
    const uint64_t c = head ? before[j] : before[j] - 1u;
    const uint32_t i = sidx[j];
    if (c >= n_cells || i >= n) continue;  // (never)
    if (head) {
      C.bin[c] = (uint32_t)(key >> BIN_GENOME_BITS);
      C.genome[c] = (uint32_t)key & 0xffffffu;
    }
    atomicAdd(C.contigs + c, 1u);
    atomicAdd(C.bases + c, (unsigned long long)t_length[i]);
  }
}

// ---- the tables --------------------------------------------------------------------------------------------------------------------
// table[row][BIN_GENOME_COLS] and the counts of the assignment are zeroed before
extern "C" __global__ void __launch_bounds__(256)
k_bin_truth_rows(const uint32_t* __restrict__ t_genome, const uint64_t* __restrict__ t_length, const uint32_t* __restrict__ t_first,
                 const uint32_t* __restrict__ t_records, uint64_t n_truth, uint32_t n_genomes, unsigned long long* __restrict__ table,
                 unsigned long long* __restrict__ counts) {
  for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n_truth; i0 += (uint64_t)gridDim.x * 256u) {  // (uniform over the workgroup)
    const uint64_t i = i0 + threadIdx.x;
    unsigned long long len = 0, none = 0, assigned = 0, assigned_bases = 0, repeated = 0;
    if (i < n_truth) {
      const uint32_t g = t_genome[i], recs = t_records[i];
      len = t_length[i];
      if (g <= n_genomes) {
        atomicAdd(table + (uint64_t)g * BIN_GENOME_COLS, 1ull);
        atomicAdd(table + (uint64_t)g * BIN_GENOME_COLS + 1u, len);
      }
      none = g == n_genomes ? 1ull : 0ull;
      if (t_first[i] != BIN_NONE) {
        assigned = 1ull;
        assigned_bases = len;
        repeated = recs - 1u;
      }
    }
    bin_wave_add(counts + BC_T_BASES, len);
    bin_wave_add(counts + BC_T_NONE, none);
    bin_wave_add(counts + BC_ASSIGNED, assigned);
    bin_wave_add(counts + BC_ASSIGNED_BASES, assigned_bases);
    bin_wave_add(counts + BC_REPEATED, repeated);
  }
}

// phase 0: the sums and the largest bases (top_bases and best_bases are zeroed before); phase 1: the lowest row that holds them
// (top_genome and best_bin are 0xffffffff before)
extern "C" __global__ void __launch_bounds__(256)
k_bin_cell_tables(BinCells C, uint64_t n_cells, uint32_t n_bins, uint32_t n_genomes, uint32_t phase, BinBins Q, unsigned long long* __restrict__ table,
                  uint32_t* __restrict__ best_bin, unsigned long long* __restrict__ counts) {
  for (uint64_t c0 = (uint64_t)blockIdx.x * 256u; c0 < n_cells; c0 += (uint64_t)gridDim.x * 256u) {  // (uniform over the workgroup)
    const uint64_t c = c0 + threadIdx.x;
    unsigned long long pairs = 0;
    if (c < n_cells) {
      const uint32_t b = C.bin[c], g = C.genome[c], k = C.contigs[c];
      const unsigned long long bases = C.bases[c];
      if (b < n_bins && g <= n_genomes) {
        unsigned long long* row = table + (uint64_t)g * BIN_GENOME_COLS;
        if (phase == 0u) {
          atomicAdd(Q.contigs + b, k);
          atomicAdd((unsigned long long*)Q.bases + b, bases);
          atomicAdd(row + 2u, (unsigned long long)k);
          atomicAdd(row + 3u, bases);
          if (g == n_genomes) {
            atomicAdd((unsigned long long*)Q.none_bases + b, bases);
          } else {
            atomicAdd(Q.real + b, k);
            atomicMax(Q.top_bases + b, bases);
            atomicAdd(row + 4u, 1ull);
            atomicMax(row + 6u, bases);
            pairs = bin_pairs(k);
          }
        } else if (g < n_genomes) {
          if (bases == Q.top_bases[b]) atomicMin(Q.top_genome + b, g);
          if (bases == row[6]) atomicMin(best_bin + g, b);
        }
      }
    }
    if (phase == 0u) bin_wave_add(counts + BC_PAIRS_CELLS, pairs);
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_bin_finish(BinBins Q, uint32_t n_bins, uint32_t n_genomes, const uint32_t* __restrict__ best_bin, unsigned long long* __restrict__ table,
             unsigned long long* __restrict__ counts) {
  const uint64_t n = n_bins > n_genomes ? n_bins : n_genomes;
  for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += (uint64_t)gridDim.x * 256u) {  // (uniform over the workgroup)
    const uint64_t i = i0 + threadIdx.x;
    unsigned long long top = 0, best = 0, pairs_b = 0, pairs_g = 0;
    uint32_t cls = 0;  // bit j: the bin is in class j (the header's order)
    if (i < n_bins) {
      const uint32_t t = Q.top_genome[i];
      pairs_b = bin_pairs(Q.real[i]);
      if (t < n_genomes) {
        top = Q.top_bases[i];
        const unsigned long long bases = Q.bases[i], truth = table[(uint64_t)t * BIN_GENOME_COLS + 1u], rest = bases - top;
        const uint32_t x5 = 100ull * rest <= 5ull * bases ? 1u : 0u, x10 = 100ull * rest <= 10ull * bases ? 1u : 0u;
        const uint32_t c = (100ull * top >= 90ull * truth ? 1u : 0u) | (100ull * top >= 70ull * truth ? 2u : 0u) | (100ull * top >= 50ull * truth ? 4u : 0u);
        cls = (x5 ? c : 0u) | (x10 ? c << 3 : 0u);
      }
    }
    if (i < n_genomes) {
      unsigned long long* row = table + i * BIN_GENOME_COLS;
      row[5] = best_bin[i];
      best = row[6];
      pairs_g = bin_pairs(row[2]);
    }
    bin_wave_add(counts + BC_SUM_TOP, top);
    bin_wave_add(counts + BC_SUM_BEST, best);
    bin_wave_add(counts + BC_PAIRS_BINS, pairs_b);
    bin_wave_add(counts + BC_PAIRS_GENOMES, pairs_g);
#pragma unroll
    for (uint32_t j = 0; j < 6u; j++) bin_wave_add(counts + BC_C90_X5 + j, (cls >> j) & 1u);
  }
}

}  // namespace simmr
