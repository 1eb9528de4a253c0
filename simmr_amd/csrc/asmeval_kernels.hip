// asmeval_kernels.hip — an assembler's contigs scored against the gold-standard assembly by canonical k-mers (gfx950): two FASTA
// texts in HBM to integer tables (include/simmr_hip.h states every rule: the text, the bases, the k-mer and its key, the entry, the
// contig's columns, the tables).  Included by asmeval.hip alone, a translation unit of its own.  The reader's routines are taken,
// not restated: the line index and the scans of fit_sam_kernels.hip / sam_kernels.hip and the name row of mapeval_kernels.hip,
// through MEV_ROUTINES_ONLY (which brings FSAM_ROUTINES_ONLY with it).  mev_lower_bound is NOT used: it searches one key with the
// 16 lanes of a group, and here every lane holds k-mers of its own, so the lookup is a lane's search of its bucket (asm_find).
//
// An add of either side is: index (count) -> scan -> index (write) -> lines (count) -> chunks -> lines (write) -> pack -> roll.
//   k_asm_index      fsam_index_tiles: launched to count a tile's line starts and, after the scan, to write them.
//   k_asm_scan       ONE workgroup: sam_scan_chunks over the tile counts; the entry behind the last tile is the number of lines.
//   k_asm_lines      a line a thread, ASM_CHUNK lines a workgroup and trip: the line's class (header: its first byte is '>') and
//                    its bases (its bytes without the line end and without a '\r' directly before the '\n').  Launched to sum a
//                    chunk (headers << 32 | bases) and, after k_asm_chunks, to write per line the add's bases before it
//                    (line_base) and per header the record's first base (rec_start) and the header's byte (rec_hdr).
//   k_asm_chunks     ONE workgroup: sam_scan_chunks over the chunk sums; writes the add's totals (lines, bases, records), the
//                    entries behind the last line and the last record, and adds records and bases to the side's counts.
//   k_asm_pack       text to planes, 32 bases a thread: the line of the thread's first base by a search in line_base, then the
//                    bytes of that line and the next ones.  A 2-bit plane (base b: bits 2 (b % 16) of 32-bit word b / 16; a
//                    thread writes two words as one 64-bit store) and a validity plane (a bit a base, 32-bit words).
//   k_asm_genomes    truth only, a record per 16 lanes: the header's text between '>' and its first '|' among the sorted names.
//   k_asm_roll_truth / k_asm_roll_cand   THE ROLL (asm_roll): a lane takes the 32 k-mer ends of one validity word.  It starts
//                    k - 1 bases earlier, holds the 64 bases around in two 64-bit registers that it shifts down two bits a base,
//                    rolls the forward value up and the reverse complement's down, counts the valid bases since the last invalid
//                    one or record start, and has a k-mer wherever that count reaches k.  One 64-bit path for every k.
//                    Truth: the lane counts its k-mers first (the same walk, keys unused), a wave scan and ONE atomic a wave
//                    give it its place among the occurrences, the second walk stores (key, genome row).
//                    Candidate: every key is looked up (asm_find); the lane sums kmers / found / shared per contig in registers
//                    and adds them to the contig's columns when the contig changes or the lane ends; consecutive votes for one
//                    genome are one (contig << 24 | genome, count) pair, appended through an atomic cursor.
//   k_asm_heads      1 where a sorted key differs from the one before it: the input of the engine's scan.
//   k_asm_entries    behind samsort_sort_pairs and the scan: the distinct entries (key, first occurrence, genome: the maximum
//                    of the head's row and, where two neighbours of a run differ, the row "shared").
//   k_asm_mult       mult = the distance of two first occurrences.
//   k_asm_table      THE PREFIX TABLE.  Rule: bits = min(24, bit length of the number of entries); table[b] = the first entry
//                    whose key >> (2k - bits) is not below b, for b = 0 .. 2^bits (a thread a bucket, a binary search each, so a
//                    bucket that holds every entry costs what an empty one costs).  A lookup then searches table[b] ..
//                    table[b + 1]: with as many buckets as entries that is about one entry, so a k-mer costs the table read
//                    and one or two key reads instead of a search over all entries.
//   k_asm_vote_sum / k_asm_vote_top   behind the sort of one add's pairs and the scan of their heads: the votes of every
//                    (contig, genome), then the contig's top by a 64-bit atomicMax of votes << 24 | (0xffffff - genome) (ties
//                    go to the lowest row) and the number of genomes it voted for.
//   k_asm_contig_len / k_asm_contig_cols   the length column of an add's records; top_genome and top_kmers from the packed top.
//   k_asm_reduce_entries / k_asm_reduce_contigs   simmr_asmeval_read: the per-genome table and the contig classes; the rows
//                    below ASM_LDS_ROWS are combined in LDS before they reach HBM, the others go to HBM directly.
// Bounds.  Every load of text is below n_bytes: a line is [starts[li], its end) with the end at most the next line's start or
// n_bytes, and pack reads byte starts[li] + off only where off is below the line's bases.  line_base has lines + 1 entries,
// rec_start records + 1, both sized on the host from n_bytes (a line per two bytes).  A plane word is written for every 32 bases
// begun and read for those only.  Occurrences and pairs are stored below a capacity the host derived from the bytes of the adds
// (a k-mer and a pair need a base each); columns of contigs below c0 + the add's records, for which the host made room after it
// had read the totals; entry columns below the number of entries the scan gave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#define MEV_ROUTINES_ONLY
#include "mapeval_kernels.hip"  // mev_name_row, MevNames, MevText; through it the line index, the scans and the ballots

namespace simmr {

#define ASM_WG 256u
#define ASM_CHUNK 256u        /* lines per workgroup and trip of k_asm_lines: a line a thread */
#define ASM_WORD 32u          /* bases per lane of pack and roll: one validity word, two words of the 2-bit plane */
#define ASM_WG_RECS 16u       /* records per workgroup and batch of k_asm_genomes */
#define ASM_LDS_ROWS 1024u    /* rows of the per-genome table that are combined in LDS */
#define ASM_GENOME_BITS 24u   /* a vote pair's key is contig << 24 | genome */
#define ASM_NONE 0xffffffffu
#define ASM_ERR_TRUTH 1u      /* a malformed truth text */
#define ASM_ERR_CAND 2u       /* a malformed candidate text */
static_assert(ASM_CHUNK == ASM_WG && ASM_WG == 256u, "sam_wg_scan is over 256 threads");
static_assert(ASM_WG_RECS * MEV_LANES == ASM_WG, "a record per group of the name search");

enum { AC_T_RECORDS = 0, AC_T_BASES, AC_T_INVALID, AC_T_KMERS, AC_T_DISTINCT, AC_T_SHARED_DISTINCT, AC_RECORDS, AC_BASES, AC_INVALID, AC_KMERS,
       AC_FOUND, AC_SHARED, AC_NOVEL, AC_SHORT, AC_C_NOVEL, AC_PURE, AC_MIXED, AC_SHARED_ONLY, AC_COUNT };
static_assert(sizeof(simmr_asmeval_counts) == AC_COUNT * 8u, "the counts in the header's order");
#define ASM_GENOME_COLS 5u    /* distinct, distinct_found, over, contigs, contig_bases */
static_assert(SIMMR_ASMEVAL_GENOME_COLS == ASM_GENOME_COLS, "the header's table");

struct AsmLines {  // the lines of one add and what the scan over them gives
  uint32_t* line_base;  // [lines + 1] the add's bases before the line
  uint32_t* rec_start;  // [records + 1] the record's first base
  uint32_t* rec_hdr;    // [records] the byte of the header's '>'
  uint32_t* tot;        // [0] lines, [1] bases, [2] records
};

struct AsmPlane {
  const uint64_t* code;       // [words] 32 bases each
  const uint32_t* valid;      // [words]
  const uint32_t* rec_start;  // [records + 1]
  const uint32_t* tot;
};

struct AsmEntries {  // the distinct k-mers of the truth in key order, and the prefix table over them
  const uint64_t* key;
  const uint32_t* genome;
  const uint32_t* table;  // [2^bits + 1]; not read where bits == 0
  uint32_t n, bits, shift;
};

struct AsmContigs {  // the contig columns since the plan
  uint64_t* length;
  uint32_t* kmers;
  uint32_t* found;
  uint32_t* shared;
  unsigned long long* top;  // votes << 24 | (0xffffff - genome); 0: no vote
  uint32_t* n_voted;        // the genomes the contig voted for
};

// A C G T in either case are 0 1 2 3; every other byte is 4
SIMMR_DEV uint32_t asm_class(uint32_t c) {
  const uint32_t f = c | 0x20u;
  return f == 'a' ? 0u : f == 'c' ? 1u : f == 'g' ? 2u : f == 't' ? 3u : 4u;
}

// the number of entries of v[0, n) that are not above x (v ascends)
SIMMR_DEV uint32_t asm_upper_bound(const uint32_t* __restrict__ v, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (v[mid] <= x) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

// the entry whose key is `key` (ASM_NONE: a miss): the bucket from the table where there is one, then a lane's binary search
SIMMR_DEV uint32_t asm_find(const AsmEntries& E, uint64_t key) {
  uint32_t lo = 0, hi = E.n;
  if (E.bits) {
    const uint32_t b = (uint32_t)(key >> E.shift);
    lo = E.table[b];
    hi = E.table[b + 1u];
  }
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    const uint64_t at = E.key[mid];
    if (at == key) return mid;
    if (at < key) lo = mid + 1u;
    else hi = mid;
  }
  return ASM_NONE;
}

// THE ROLL.  emit(rec, key) for every k-mer that ends on a base of word w, in position order; rec is the record's ordinal in
// the add.  n_bases > 32 w.  A base before the add's first record (a malformed text) has no k-mer.
// asm_roll_at is the walk itself and hands out two things more: the add's position of the k-mer's LAST base, and whether the key
// is the reverse complement's value (asmmap_kernels.hip places k-mers with them); asm_roll is the same walk without them.
template <class F>
SIMMR_DEV void asm_roll_at(const AsmPlane& P, uint32_t w, uint32_t n_bases, uint32_t n_rec, uint32_t k, F&& emit) {
  const uint32_t pos0 = w * ASM_WORD, end = pos0 + ASM_WORD < n_bases ? pos0 + ASM_WORD : n_bases;
  const uint32_t back = pos0 < k - 1u ? pos0 : k - 1u, ps = pos0 - back;
  uint64_t chi = P.code[w], clo = w ? P.code[w - 1u] : 0ull;
  uint64_t v = (uint64_t)P.valid[w] << 32 | (w ? P.valid[w - 1u] : 0u);
  const uint32_t sh = ASM_WORD - back;  // the bases of the lower register in front of ps: 2 .. 32
  if (sh == ASM_WORD) { clo = chi; chi = 0ull; }
  else { clo = (clo >> (2u * sh)) | (chi << (64u - 2u * sh)); chi >>= 2u * sh; }
  v >>= sh;
  uint32_t rec = asm_upper_bound(P.rec_start, n_rec, ps) - 1u;  // the last record that starts at or before ps; ASM_NONE: none
  uint32_t next = P.rec_start[rec + 1u];
  const uint64_t mask = (1ull << (2u * k)) - 1ull;
  const uint32_t top = 2u * (k - 1u);
  uint64_t fwd = 0, rc = 0;
  uint32_t run = 0;
  for (uint32_t p = ps; p < end; p++) {
    if (p == next) {  // a record starts here: the last of those that start here has the base
      rec++;
      while (rec + 1u < n_rec && P.rec_start[rec + 1u] <= p) rec++;
      next = P.rec_start[rec + 1u];
      run = 0;
    }
    const uint64_t c = clo & 3ull;
    const bool ok = (v & 1ull) != 0ull;
    clo = (clo >> 2) | (chi << 62);
    chi >>= 2;
    v >>= 1;
    fwd = ((fwd << 2) | c) & mask;
    rc = (rc >> 2) | ((3ull - c) << top);
    run = ok ? run + 1u : 0u;
    if (p >= pos0 && run >= k && rec != ASM_NONE) emit(rec, fwd < rc ? fwd : rc, p, fwd < rc ? 0u : 1u);
  }
}

template <class F>
SIMMR_DEV void asm_roll(const AsmPlane& P, uint32_t w, uint32_t n_bases, uint32_t n_rec, uint32_t k, F&& emit) {
  asm_roll_at(P, w, n_bases, n_rec, k, [&](uint32_t rec, uint64_t key, uint32_t, uint32_t) { emit(rec, key); });
}

// The kernels.  asmmap_kernels.hip (a translation unit of its own) includes this file with ASM_ROUTINES_ONLY defined and takes the
// routines and the structs above without them; the text-to-planes stage reaches it through asmeval_front.hpp.
#ifndef ASM_ROUTINES_ONLY
// ---- the line index -----------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_asm_index(const uint8_t* __restrict__ text, uint64_t n_bytes, uint64_t n_tiles, uint64_t* __restrict__ tile_sum,
            const uint64_t* __restrict__ tile_prefix, uint32_t* __restrict__ starts, uint64_t start_capacity) {
  __shared__ uint32_t lds[FSAM_WG];
  fsam_index_tiles(text, n_bytes, n_tiles, tile_sum, tile_prefix, starts, start_capacity, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_asm_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

// ---- the lines: class, bases, and the scan of both per record ---------------------------------------------------------------------
// chunk_prefix == nullptr: chunk_sum[c] = headers << 32 | bases of chunk c.  Else: the line and record entries, and the error
// bit `err_bit` where a sequence line with a base stands before the add's first header.
extern "C" __global__ void __launch_bounds__(ASM_WG)
k_asm_lines(MevText W, uint64_t line_capacity, uint64_t* __restrict__ chunk_sum, const uint64_t* __restrict__ chunk_prefix, AsmLines L,
            uint32_t* __restrict__ err, uint32_t err_bit) {
  __shared__ uint64_t lds[ASM_WG];
  const uint8_t* __restrict__ t = W.text;
  const uint64_t n_lines = *W.n_lines < line_capacity ? *W.n_lines : line_capacity;
  const uint64_t n_chunks = (n_lines + ASM_CHUNK - 1u) / ASM_CHUNK;
  for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // (uniform over the workgroup)
    const uint64_t li = chunk * ASM_CHUNK + threadIdx.x;
    uint64_t v = 0;
    uint32_t s = 0, bases = 0;
    bool hdr = false;
    if (li < n_lines) {
      s = W.starts[li];
      const uint32_t nxt = li + 1u < n_lines ? W.starts[li + 1u] : (uint32_t)W.n_bytes;
      uint32_t e = nxt;
      while (e > s + 1u && t[e - 1u] == '\n') e--;  // (byte s is no '\n')
      if (e < nxt && e > s && t[e - 1u] == '\r') e--;
      hdr = t[s] == '>';
      bases = hdr ? 0u : e - s;
      v = hdr ? 1ull << 32 : (uint64_t)bases;
    }
    uint64_t total;
    const uint64_t ex = sam_wg_scan<uint64_t>(v, lds, &total);
    if (!chunk_prefix) {
      if (threadIdx.x == 0) chunk_sum[chunk] = total;
      continue;
    }
    if (li >= n_lines) continue;
    const uint64_t at = chunk_prefix[chunk] + ex;
    const uint32_t before = (uint32_t)at, recs = (uint32_t)(at >> 32);
    L.line_base[li] = before;
    if (hdr) {
      L.rec_start[recs] = before;
      L.rec_hdr[recs] = s;
    } else if (bases > 0u && recs == 0u) {
      atomicOr(err, err_bit);
    }
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_asm_chunks(const uint64_t* __restrict__ n_lines_p, uint64_t line_capacity, const uint64_t* __restrict__ chunk_sum, uint64_t* __restrict__ chunk_prefix,
             AsmLines L, unsigned long long* __restrict__ counts, uint32_t records_at, uint32_t bases_at) {
  __shared__ uint64_t lds[256];
  const uint64_t n_lines = *n_lines_p < line_capacity ? *n_lines_p : line_capacity;
  const uint64_t n_chunks = (n_lines + ASM_CHUNK - 1u) / ASM_CHUNK;
  sam_scan_chunks(chunk_sum, chunk_prefix, n_chunks, lds);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t all = chunk_prefix[n_chunks];
    const uint32_t bases = (uint32_t)all, recs = (uint32_t)(all >> 32);
    L.tot[0] = (uint32_t)n_lines;
    L.tot[1] = bases;
    L.tot[2] = recs;
    L.line_base[n_lines] = bases;
    L.rec_start[recs] = bases;
    counts[records_at] += recs;
    counts[bases_at] += bases;
  }
}

// ---- text to planes ---------------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(ASM_WG)
k_asm_pack(MevText W, AsmLines L, uint64_t* __restrict__ code, uint32_t* __restrict__ valid, unsigned long long* __restrict__ counts, uint32_t invalid_at) {
  const uint8_t* __restrict__ t = W.text;
  const uint32_t n_lines = L.tot[0], n_bases = L.tot[1];
  const uint32_t n_words = n_bases / ASM_WORD + (n_bases % ASM_WORD ? 1u : 0u);
  for (uint64_t w = (uint64_t)blockIdx.x * ASM_WG + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * ASM_WG) {
    const uint32_t b0 = (uint32_t)w * ASM_WORD, nb = n_bases - b0 < ASM_WORD ? n_bases - b0 : ASM_WORD;
    uint32_t li = asm_upper_bound(L.line_base, n_lines, b0) - 1u;  // (line_base[0] = 0: there is one) the line that holds base b0
    uint32_t first = L.line_base[li], len = L.line_base[li + 1u] - first, off = b0 - first, p = W.starts[li] + off;
    uint64_t c2 = 0;
    uint32_t ok = 0;
    for (uint32_t i = 0; i < nb; i++) {
      while (off >= len) {  // (b0 + i < n_bases: a later line has the base)
        li++;
        first = L.line_base[li];
        len = L.line_base[li + 1u] - first;
        off = 0;
        p = W.starts[li];
      }
      const uint32_t cls = asm_class(t[p]);
      if (cls < 4u) {
        c2 |= (uint64_t)cls << (2u * i);
        ok |= 1u << i;
      }
      p++;
      off++;
    }
    code[w] = c2;
    valid[w] = ok;
    const uint32_t bad = nb - (uint32_t)__popc(ok);
    if (bad) atomicAdd(counts + invalid_at, (unsigned long long)bad);
  }
}

// ---- the genome of every truth record -----------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(ASM_WG)
k_asm_genomes(MevText W, AsmLines L, MevNames N, uint32_t* __restrict__ rec_row, uint32_t* __restrict__ err) {
  const uint8_t* __restrict__ t = W.text;
  const uint32_t n = (uint32_t)W.n_bytes, n_rec = L.tot[2];
  const uint32_t sub = threadIdx.x & (MEV_LANES - 1u), row = threadIdx.x / MEV_LANES;
  const uint32_t n_batches = n_rec / ASM_WG_RECS + (n_rec % ASM_WG_RECS ? 1u : 0u);
  for (uint32_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint32_t r = batch * ASM_WG_RECS + row;
    if (r >= n_rec) continue;  // (uniform over the row)
    const uint32_t a = L.rec_hdr[r] + 1u;
    uint32_t bar = ASM_NONE;
    for (uint32_t p0 = a; p0 - a <= SAM_RNAME_MAX; p0 += MEV_LANES) {  // (uniform over the row)
      const uint32_t p = p0 + sub;
      const uint32_t c = p < n ? t[p] : '\n';
      const uint32_t m_bar = fsam_ballot(c == '|'), m_end = fsam_ballot(c == '\n' || c == ' ' || c == '\t' || c == '\r');
      const uint32_t f_bar = m_bar ? (uint32_t)__builtin_ctz(m_bar) : 32u, f_end = m_end ? (uint32_t)__builtin_ctz(m_end) : 32u;
      if (f_bar < f_end) bar = p0 + f_bar;
      if (m_bar | m_end) break;
    }
    const uint32_t g = bar != ASM_NONE ? mev_name_row(N, t, a, bar, sub) : MEV_NO_ROW;
    if (sub == 0u) {
      rec_row[r] = g;
      if (g == MEV_NO_ROW) atomicOr(err, ASM_ERR_TRUTH);
    }
  }
}

// ---- the roll over the truth: every k-mer occurrence as (key, genome row) -------------------------------------------------------
extern "C" __global__ void __launch_bounds__(ASM_WG)
k_asm_roll_truth(AsmPlane P, uint32_t k, const uint32_t* __restrict__ rec_row, uint64_t* __restrict__ occ_key, uint32_t* __restrict__ occ_row,
                 uint64_t capacity, unsigned long long* __restrict__ cursor) {
  const uint32_t n_bases = P.tot[1], n_rec = P.tot[2];
  const uint32_t n_words = n_bases / ASM_WORD + (n_bases % ASM_WORD ? 1u : 0u);
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t w0 = (uint64_t)blockIdx.x * ASM_WG + (threadIdx.x & ~63u); w0 < n_words; w0 += (uint64_t)gridDim.x * ASM_WG) {  // (uniform over the wave)
    const uint64_t w = w0 + lane;
    uint32_t cnt = 0;
    if (w < n_words) asm_roll(P, (uint32_t)w, n_bases, n_rec, k, [&](uint32_t, uint64_t) { cnt++; });
    uint32_t inc = cnt;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
      if (lane >= d) inc += o;
    }
    const uint32_t total = (uint32_t)__shfl((int)inc, 63, 64);
    unsigned long long base = 0;
    if (lane == 0u && total) base = atomicAdd(cursor, (unsigned long long)total);
    base = __shfl(base, 0, 64);
    uint64_t at = base + inc - cnt;
    if (w < n_words && cnt)
      asm_roll(P, (uint32_t)w, n_bases, n_rec, k, [&](uint32_t rec, uint64_t key) {
        if (at < capacity) {
          occ_key[at] = key;
          occ_row[at] = rec_row[rec];
        }
        at++;
      });
  }
}

// ---- the roll over the candidates: lookups, the contig's sums, the vote pairs ----------------------------------------------------
struct AsmLaneSums {  // what a lane holds of the contig it is in
  uint32_t rec, kmers, found, shared, v_genome, v_count;
};

extern "C" __global__ void __launch_bounds__(ASM_WG)
k_asm_roll_cand(AsmPlane P, uint32_t k, AsmEntries E, uint32_t n_genomes, uint32_t* __restrict__ hits, uint64_t c0, AsmContigs C,
                uint64_t* __restrict__ pair_key, uint32_t* __restrict__ pair_count, uint64_t pair_capacity, unsigned long long* __restrict__ pair_cursor) {
  const uint32_t n_bases = P.tot[1], n_rec = P.tot[2];
  const uint32_t n_words = n_bases / ASM_WORD + (n_bases % ASM_WORD ? 1u : 0u);
  for (uint64_t w = (uint64_t)blockIdx.x * ASM_WG + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * ASM_WG) {
    AsmLaneSums S{ASM_NONE, 0u, 0u, 0u, ASM_NONE, 0u};
    auto flush_vote = [&]() {
      if (S.v_count) {
        const unsigned long long at = atomicAdd(pair_cursor, 1ull);
        if (at < pair_capacity) {
          pair_key[at] = (c0 + S.rec) << ASM_GENOME_BITS | S.v_genome;
          pair_count[at] = S.v_count;
        }
      }
      S.v_count = 0u;
      S.v_genome = ASM_NONE;
    };
    auto flush = [&]() {
      flush_vote();
      if (S.rec != ASM_NONE) {
        const uint64_t c = c0 + S.rec;
        if (S.kmers) atomicAdd(C.kmers + c, S.kmers);
        if (S.found) atomicAdd(C.found + c, S.found);
        if (S.shared) atomicAdd(C.shared + c, S.shared);
      }
      S.kmers = S.found = S.shared = 0u;
    };
    asm_roll(P, (uint32_t)w, n_bases, n_rec, k, [&](uint32_t rec, uint64_t key) {
      if (rec != S.rec) {
        flush();
        S.rec = rec;
      }
      S.kmers++;
      const uint32_t e = asm_find(E, key);
      if (e == ASM_NONE) return;
      S.found++;
      atomicAdd(hits + e, 1u);
      const uint32_t g = E.genome[e];
      if (g == n_genomes) { S.shared++; return; }
      if (g != S.v_genome) {
        flush_vote();
        S.v_genome = g;
      }
      S.v_count++;
    });
    flush();
  }
}

// ---- the plan: run heads, distinct entries, the table ------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
k_asm_heads(const uint64_t* __restrict__ skey, uint64_t n, uint32_t* __restrict__ head) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u)
    head[j] = j == 0u || skey[j] != skey[j - 1u] ? 1u : 0u;
}

// e_genome is zeroed before; before[j] = the heads in front of j; n_entries = before[n]
extern "C" __global__ void __launch_bounds__(256)
k_asm_entries(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ occ_row, const uint64_t* __restrict__ before,
              uint64_t n, uint64_t n_entries, uint32_t n_genomes, uint64_t* __restrict__ e_key, uint32_t* __restrict__ e_start, uint32_t* __restrict__ e_genome) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u) {
    const uint64_t key = skey[j];
    const uint32_t row = occ_row[idx[j]];
    const bool head = j == 0u || key != skey[j - 1u];
    const uint64_t e = head ? before[j] : before[j] - 1u;
    if (e >= n_entries) continue;
    if (head) {
      e_key[e] = key;
      e_start[e] = (uint32_t)j;
      atomicMax(e_genome + e, row);
    } else if (occ_row[idx[j - 1u]] != row) {
      atomicMax(e_genome + e, n_genomes);
    }
    if (j == 0u) e_start[n_entries] = (uint32_t)n;
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_asm_mult(const uint32_t* __restrict__ e_start, uint64_t n_entries, uint32_t* __restrict__ mult) {
  for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < n_entries; e += (uint64_t)gridDim.x * 256u) mult[e] = e_start[e + 1u] - e_start[e];
}

extern "C" __global__ void __launch_bounds__(256)
k_asm_table(const uint64_t* __restrict__ e_key, uint32_t n_entries, uint32_t bits, uint32_t shift, uint32_t* __restrict__ table) {
  const uint64_t n_buckets = (1ull << bits) + 1ull;
  for (uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x; b < n_buckets; b += (uint64_t)gridDim.x * 256u) {
    const uint64_t want = b << shift;
    uint32_t lo = 0, hi = n_entries;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if (e_key[mid] < want) lo = mid + 1u;
      else hi = mid;
    }
    table[b] = lo;
  }
}

// ---- the votes of one add ----------------------------------------------------------------------------------------------------------
// v_count is zeroed before
extern "C" __global__ void __launch_bounds__(256)
k_asm_vote_sum(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ pair_count, const uint64_t* __restrict__ before,
               uint64_t n, uint64_t n_votes, uint64_t* __restrict__ v_key, uint32_t* __restrict__ v_count) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u) {
    const uint64_t key = skey[j];
    const bool head = j == 0u || key != skey[j - 1u];
    const uint64_t v = head ? before[j] : before[j] - 1u;
    if (v >= n_votes) continue;
    if (head) v_key[v] = key;
    atomicAdd(v_count + v, pair_count[idx[j]]);
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_asm_vote_top(const uint64_t* __restrict__ v_key, const uint32_t* __restrict__ v_count, uint64_t n_votes, uint64_t n_contigs, AsmContigs C) {
  for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < n_votes; v += (uint64_t)gridDim.x * 256u) {
    const uint64_t c = v_key[v] >> ASM_GENOME_BITS, g = v_key[v] & 0xffffffull;
    if (c >= n_contigs) continue;
    atomicMax(C.top + c, (unsigned long long)v_count[v] << ASM_GENOME_BITS | (0xffffffull - g));
    atomicAdd(C.n_voted + c, 1u);
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_asm_contig_len(const uint32_t* __restrict__ rec_start, uint32_t n_rec, uint64_t c0, uint64_t* __restrict__ length) {
  for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < n_rec; r += gridDim.x * 256u) length[c0 + r] = rec_start[r + 1u] - rec_start[r];
}

extern "C" __global__ void __launch_bounds__(256)
k_asm_contig_cols(const unsigned long long* __restrict__ top, uint64_t n_contigs, uint32_t* __restrict__ top_genome, uint32_t* __restrict__ top_kmers) {
  for (uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x; c < n_contigs; c += (uint64_t)gridDim.x * 256u) {
    const unsigned long long t = top[c];
    if (top_genome) top_genome[c] = t ? 0xffffffu - (uint32_t)(t & 0xffffffull) : ASM_NONE;
    if (top_kmers) top_kmers[c] = (uint32_t)(t >> ASM_GENOME_BITS);
  }
}

// ---- simmr_asmeval_read ------------------------------------------------------------------------------------------------------------
// table[row][ASM_GENOME_COLS]; rows below ASM_LDS_ROWS through LDS
extern "C" __global__ void __launch_bounds__(256)
k_asm_reduce_entries(const uint32_t* __restrict__ e_genome, const uint32_t* __restrict__ mult, const uint32_t* __restrict__ hits, uint64_t n_entries,
                     uint32_t n_rows, unsigned long long* __restrict__ table) {
  __shared__ uint32_t l_t[ASM_LDS_ROWS * 3u];
  for (uint32_t i = threadIdx.x; i < ASM_LDS_ROWS * 3u; i += 256u) l_t[i] = 0u;
  __syncthreads();
  for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < n_entries; e += (uint64_t)gridDim.x * 256u) {
    const uint32_t g = e_genome[e], h = hits[e];
    if (g >= n_rows) continue;
    const bool found = h > 0u, over = h > mult[e];
    if (g < ASM_LDS_ROWS) {
      atomicAdd(&l_t[g * 3u], 1u);
      if (found) atomicAdd(&l_t[g * 3u + 1u], 1u);
      if (over) atomicAdd(&l_t[g * 3u + 2u], 1u);
    } else {
      atomicAdd(table + (uint64_t)g * ASM_GENOME_COLS, 1ull);
      if (found) atomicAdd(table + (uint64_t)g * ASM_GENOME_COLS + 1u, 1ull);
      if (over) atomicAdd(table + (uint64_t)g * ASM_GENOME_COLS + 2u, 1ull);
    }
  }
  __syncthreads();
  const uint32_t lds_rows = n_rows < ASM_LDS_ROWS ? n_rows : ASM_LDS_ROWS;
  for (uint32_t i = threadIdx.x; i < lds_rows * 3u; i += 256u)
    if (l_t[i]) atomicAdd(table + (uint64_t)(i / 3u) * ASM_GENOME_COLS + i % 3u, (unsigned long long)l_t[i]);
}

#define ASM_CONTIG_SUMS 10u  /* records, bases, kmers, found, shared, then the five classes */
extern "C" __global__ void __launch_bounds__(256)
k_asm_reduce_contigs(AsmContigs C, uint64_t n_contigs, uint32_t n_genomes, unsigned long long* __restrict__ table, unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long l_g[ASM_LDS_ROWS * 2u];
  __shared__ unsigned long long l_c[ASM_CONTIG_SUMS];
  for (uint32_t i = threadIdx.x; i < ASM_LDS_ROWS * 2u; i += 256u) l_g[i] = 0ull;
  if (threadIdx.x < ASM_CONTIG_SUMS) l_c[threadIdx.x] = 0ull;
  __syncthreads();
  for (uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x; c < n_contigs; c += (uint64_t)gridDim.x * 256u) {
    const uint64_t len = C.length[c];
    const uint32_t kmers = C.kmers[c], found = C.found[c], shared = C.shared[c], voted = C.n_voted[c];
    const unsigned long long t = C.top[c];
    const uint32_t cls = kmers == 0u ? 0u : found == 0u ? 1u : t == 0ull ? 4u : voted == 1u ? 2u : 3u;  // short, novel, pure, mixed, shared only
    atomicAdd(&l_c[0], 1ull);
    atomicAdd(&l_c[1], (unsigned long long)len);
    atomicAdd(&l_c[2], (unsigned long long)kmers);
    atomicAdd(&l_c[3], (unsigned long long)found);
    atomicAdd(&l_c[4], (unsigned long long)shared);
    atomicAdd(&l_c[5u + cls], 1ull);
    if (t) {
      const uint32_t g = 0xffffffu - (uint32_t)(t & 0xffffffull);
      if (g >= n_genomes) continue;
      if (g < ASM_LDS_ROWS) {
        atomicAdd(&l_g[g * 2u], 1ull);
        atomicAdd(&l_g[g * 2u + 1u], (unsigned long long)len);
      } else {
        atomicAdd(table + (uint64_t)g * ASM_GENOME_COLS + 3u, 1ull);
        atomicAdd(table + (uint64_t)g * ASM_GENOME_COLS + 4u, (unsigned long long)len);
      }
    }
  }
  __syncthreads();
  const uint32_t lds_rows = n_genomes < ASM_LDS_ROWS ? n_genomes : ASM_LDS_ROWS;
  for (uint32_t i = threadIdx.x; i < lds_rows * 2u; i += 256u)
    if (l_g[i]) atomicAdd(table + (uint64_t)(i / 2u) * ASM_GENOME_COLS + 3u + i % 2u, l_g[i]);
  if (threadIdx.x < ASM_CONTIG_SUMS && l_c[threadIdx.x]) {
    // records, bases, ., kmers, found, shared, ., then the classes: AC_INVALID and AC_NOVEL are not made here
    const uint32_t at = threadIdx.x < 2u ? AC_RECORDS + threadIdx.x : threadIdx.x < 5u ? AC_KMERS + (threadIdx.x - 2u) : AC_SHORT + (threadIdx.x - 5u);
    atomicAdd(counts + at, l_c[threadIdx.x]);
  }
}

#endif  // ASM_ROUTINES_ONLY

}  // namespace simmr
