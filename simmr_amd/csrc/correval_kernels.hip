// correval_kernels.hip — a read error corrector's output scored against the true reads (gfx950): a SAM text and a FASTQ text in HBM
// to integer tables (include/simmr_hip.h states every rule: the truth record's steps, the entry, the corrected record, the name and
// its key, the verdict, the tables).  Included by correval.hip alone, a translation unit of its own.  The readers' routines are
// taken, not restated: ove_name_key of ovleval_kernels.hip through OVE_ROUTINES_ONLY, which brings mev_read_line and mev_lower_bound
// of mapeval_kernels.hip (MEV_ROUTINES_ONLY) and the SAM reader's routines and scans of fit_sam_kernels.hip / sam_kernels.hip with it.
//
// Seven kernels; a work item past a line index is a LINE (truth) or a RECORD (corrected) shared by CEV_LANES = 16 lanes (one DPP row).
//   k_cev_index    fsam_index_tiles: the truth's line index (empty lines never enter it); launched to count and, after the scan, to write.
//   k_cev_lines    the corrected side's line index, which keeps empty lines: a byte starts a line when it stands first or behind a
//                  '\n', so a tile's count is the '\n' before its bytes.  16 bytes a thread; launched to count a 4096-byte tile's
//                  starts and, after the scan, to write them at their places.
//   k_cev_scan     ONE workgroup: sam_scan_chunks over the tile counts; the entry behind the last tile is the number of lines.
//   k_cev_truth    a truth line per group: mev_read_line, then the field scan out to QUAL and the MD tag, the checks, a first walk
//                  over MD with fsam_md_lane that sums and validates it, room for L bytes in the two planes and an entry slot from
//                  atomic cursors (the order is arbitrary and nothing depends on it), and a second walk that fills the planes.
//                  THE FILL HAS NO PATCH: an MD byte is a run (a number: so many matches; a letter: one mismatch), the round's runs
//                  are scanned across the row and every position of the round is dealt to a lane, which finds its run by a search
//                  in the lanes' inclusive sums (k_fsam_expand's dealing) and stores its two plane bytes once.  No byte is written
//                  twice, so no store waits for another.
//   k_cev_gather   behind samsort_sort_pairs: the entry columns into key order, and the neighbour check for equal keys.
//   k_cev_score    a corrected record per group: its lines' ends, the name, ove_name_key, the 16-way key search, then 16 corrected
//                  bytes and 16 bytes of either plane a round, the verdict per lane.  Accumulation: the sums of the record in
//                  group-uniform registers from ballots and popcounts (`kept` by base: the four cells of the cube that take nearly
//                  every base); the cube's other cells, by_qual's and by_pos's other columns by one LDS atomic per such base;
//                  by_qual's kept column by one LDS atomic per DISTINCT quality of a round's 16 lanes; by_pos's kept column not at
//                  all: a histogram of the compared lengths (one LDS atomic a record) and a column of the not-kept positions give
//                  it by subtraction on the host.  Every table is privatised in LDS and added to HBM when the workgroup ends.
//   k_cev_reduce   the per-entry counts (missing, multiple, the six classes by before and residual) over hits[] / residual[] / before[].
// Bounds.  Every load of text is below n_bytes and inside the record's lines (past the field scan: inside the line's fields); an
// entry is stored below the capacity the adds' byte counts gave; a plane byte is stored at a column below L inside the L bytes the
// cursor gave, which end below the planes' capacity; hits[] and residual[] are indexed by a search result below n_entries; a
// plane byte is loaded at a position below the entry's L, which the truth writer planned.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#define OVE_ROUTINES_ONLY
#include "ovleval_kernels.hip"  // ove_name_key; through it mev_read_line, mev_lower_bound, MevText, the reader's routines and the scans

namespace simmr {

#define CEV_LANES 16u
#define CEV_WG 256u
#define CEV_WG_RECS 16u      /* lines or records per workgroup and batch */
#define CEV_MIN_LINE MEV_MIN_LINE
#define CEV_TILE FSAM_TILE
#define CEV_POS SIMMR_CORREVAL_POS
#define CEV_QUALS SIMMR_CORREVAL_QUALS
#define CEV_ERR_TRUTH 1u     /* a malformed truth record */
#define CEV_ERR_READS 2u     /* a malformed corrected text */
#define CEV_ERR_DUP 4u       /* two truth entries with one key */
static_assert(CEV_LANES == MEV_LANES && CEV_LANES == FSAM_LANES, "the group of the search and of the ballot is the reader's");

enum { CC_T_LINES = 0, CC_T_HEADER, CC_T_RECORDS, CC_T_ENTRIES, CC_T_SKIPPED, CC_LINES, CC_RECORDS, CC_UNKNOWN_READ, CC_SCORED, CC_TRIMMED_RECORDS,
       CC_LONGER_RECORDS, CC_COMPARED, CC_KEPT, CC_DAMAGED, CC_FIXED, CC_LEFT, CC_MISCORRECTED, CC_AMBIGUOUS, CC_TRIMMED_ERROR, CC_TRIMMED_CLEAN,
       CC_EXTRA, CC_MISSING, CC_MULTIPLE, CC_CLEAN_KEPT, CC_CLEAN_DAMAGED, CC_FIXED_ALL, CC_IMPROVED, CC_UNCHANGED, CC_WORSE, CC_COUNT };
static_assert(sizeof(simmr_correval_counts) == CC_COUNT * 8u, "the counts in the header's order");

// The object's table of 64-bit words: the counts, the cube, by_qual, by_pos (column 0: the compared positions that are NOT kept,
// the ambiguous ones included), the histogram of the compared lengths min(m, CEV_POS), and the sum of max(m - (CEV_POS - 1), 0).
enum { CT_CUBE = CC_COUNT, CT_QUAL = CT_CUBE + 125, CT_POS = CT_QUAL + CEV_QUALS * 5, CT_LEN = CT_POS + CEV_POS * 5, CT_TAIL = CT_LEN + CEV_POS + 1,
       CT_WORDS = CT_TAIL + 1 };

struct CevEntries {  // the truth entries: appended in any order, or gathered into key order
  uint64_t* key;
  uint32_t* len;     // L
  uint64_t* off;     // the entry's first byte in either plane
  uint32_t* before;
};

struct CevPlanes {
  uint8_t* ot;       // o | t << 3, in the read's orientation
  uint8_t* q;        // 0 .. 94
  uint64_t cap;
};

// A C G T in either letter case: 0 .. 3; every other byte: 4
SIMMR_DEV uint32_t cev_class(uint32_t x) { return fit_class(x & 0xdfu, 4u, 4u); }

// ---- the line indexes and the scan ----------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_cev_index(const uint8_t* __restrict__ text, uint64_t n_bytes, uint64_t n_tiles, uint64_t* __restrict__ tile_sum,
            const uint64_t* __restrict__ tile_prefix, uint32_t* __restrict__ starts, uint64_t start_capacity) {
  __shared__ uint32_t lds[FSAM_WG];
  fsam_index_tiles(text, n_bytes, n_tiles, tile_sum, tile_prefix, starts, start_capacity, lds);
}

// every line, the empty ones too: byte p (below n_bytes) starts one when p == 0 or text[p - 1] == '\n'
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_cev_lines(const uint8_t* __restrict__ text, uint64_t n_bytes, uint64_t n_tiles, uint64_t* __restrict__ tile_sum,
            const uint64_t* __restrict__ tile_prefix, uint32_t* __restrict__ starts, uint64_t start_capacity) {
  __shared__ uint32_t lds[FSAM_WG];
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // (uniform over the workgroup)
    const uint64_t p0 = tile * CEV_TILE + 16u * threadIdx.x;
    uint32_t mask = 0;
    if (p0 < n_bytes) {
      uint32_t prev = p0 ? text[p0 - 1u] : '\n';
      for (uint32_t b = 0; b < 16u && p0 + b < n_bytes; b++) {
        if (prev == '\n') mask |= 1u << b;
        prev = text[p0 + b];
      }
    }
    uint32_t total;
    const uint32_t ex = sam_wg_scan<uint32_t>((uint32_t)__popc(mask), lds, &total);
    if (!starts) {
      if (threadIdx.x == 0) tile_sum[tile] = total;
      continue;
    }
    uint64_t at = tile_prefix[tile] + ex;
    for (; mask; mask &= mask - 1u, at++)
      if (at < start_capacity) starts[at] = (uint32_t)(p0 + (uint32_t)__builtin_ctz(mask));
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_cev_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

#define CEV_COUNT(which) do { if (sub == 0u) atomicAdd(counts + (which), 1ull); } while (0)
#define CEV_BAD(which) do { if (sub == 0u) atomicOr(err, (which)); } while (0)

// ---- the truth ------------------------------------------------------------------------------------------------------------------
// cursor[0]: the entries so far (never reset between adds), cursor[1]: the largest key, cursor[2]: the plane bytes so far
extern "C" __global__ void __launch_bounds__(CEV_WG)
k_cev_truth(MevText W, CevEntries E, uint64_t capacity, CevPlanes P, unsigned long long* __restrict__ cursor, unsigned long long* __restrict__ counts,
            uint32_t* __restrict__ err) {
  const uint8_t* __restrict__ t = W.text;
  const uint32_t sub = threadIdx.x & (CEV_LANES - 1u), row = threadIdx.x / CEV_LANES;
  const uint64_t n_lines = *W.n_lines, n = W.n_bytes;
  const uint64_t n_batches = (n_lines + CEV_WG_RECS - 1u) / CEV_WG_RECS;
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t li = batch * CEV_WG_RECS + row;
    if (li >= n_lines) continue;  // (uniform over the row)
    const uint32_t line = W.starts[li];
    if (line >= n) continue;      // (never: the index holds places of the text)
    CEV_COUNT(CC_T_LINES);
    if (t[line] == '@') { CEV_COUNT(CC_T_HEADER); continue; }
    CEV_COUNT(CC_T_RECORDS);
    const MevLine R = mev_read_line(t, n, line, sub);
    if (R.bad) { CEV_BAD(CEV_ERR_TRUTH); continue; }
    // ---- the fields out to QUAL and the MD tag: tab j ends field j; the line ends at its '\n' or at the text's end
    uint32_t tb[11];
#pragma unroll
    for (uint32_t j = 0; j < 11u; j++) tb[j] = FSAM_NONE;
    uint32_t n_tab = 0, md = FSAM_NONE, md_end = FSAM_NONE, end = (uint32_t)n;
    for (uint64_t p0 = line;; p0 += CEV_LANES) {
      const uint64_t p = p0 + sub;
      const uint32_t c = p < n ? t[p] : '\n';
      uint32_t m_tab = fsam_ballot(c == '\t');
      const uint32_t m_nl = fsam_ballot(c == '\n');
      if (m_nl) {
        const uint32_t first = (uint32_t)__builtin_ctz(m_nl);
        m_tab &= (1u << first) - 1u;
        end = (uint32_t)(p0 + first);
      }
      for (; m_tab; m_tab &= m_tab - 1u) {
        const uint32_t at = (uint32_t)p0 + (uint32_t)__builtin_ctz(m_tab);
#pragma unroll
        for (uint32_t j = 0; j < 11u; j++)
          if (n_tab == j) tb[j] = at;
        n_tab++;
        if (md != FSAM_NONE && md_end == FSAM_NONE) md_end = at;
        if (n_tab >= 11u && md == FSAM_NONE && (uint64_t)at + 6u <= n && t[at + 1u] == 'M' && t[at + 2u] == 'D' && t[at + 3u] == ':' &&
            t[at + 4u] == 'Z' && t[at + 5u] == ':')
          md = at + 6u;
      }
      if (m_nl) break;
    }
    if (md != FSAM_NONE && md_end == FSAM_NONE) md_end = end;
    if (md != FSAM_NONE && md > md_end) md = FSAM_NONE;  // (the tag's five bytes ran over the line's end)
    if (n_tab < 10u) { CEV_BAD(CEV_ERR_TRUTH); continue; }  // (never: mev_read_line has counted the same tabs)
    const uint32_t cigar = tb[4] + 1u, cigar_end = tb[5], seq = tb[8] + 1u, seq_end = tb[9];
    const uint32_t qual = tb[9] + 1u, qual_end = n_tab > 10u ? tb[10] : end;
    const uint32_t L = seq_end - seq;
    // ---- step 1
    const bool seq_star = L == 1u && t[seq] == '*';
    uint64_t run = 0;
    const bool one_run = cigar_end > cigar && t[cigar_end - 1u] == 'M' && fsam_field_number(t, cigar, cigar_end - 1u, false, &run) && run == L && L > 0u;
    if ((R.flag & 0x904u) || seq_star || !one_run) { CEV_COUNT(CC_T_SKIPPED); continue; }
    // ---- step 2
    uint32_t bad = (!R.id_ok || R.pos == 0u || md == FSAM_NONE) ? 1u : 0u;
    const bool has_qual = !(qual_end - qual == 1u && t[qual] == '*');  // (a single '*' is "no qualities", whatever L is)
    if (has_qual && qual_end - qual != L) bad = 1u;
    if (!bad && has_qual) {
      uint32_t bad_q = 0;
      for (uint32_t i0 = 0; i0 < L; i0 += CEV_LANES) {
        const uint32_t i = i0 + sub;
        if (i < L && (uint32_t)t[qual + i] - 33u > 93u) bad_q = 1u;
      }
      bad = fsam_row_or(bad_q);
    }
    if (!bad) {  // MD: its sum and its bytes
      uint64_t md_m = 0;
      uint32_t md_bad = 0, in_del = 0;
      for (uint64_t p0 = md; p0 < md_end; p0 += CEV_LANES) {
        uint32_t len, byte;
        const uint32_t kind = fsam_md_lane(t, md, md_end, p0 + sub, sub, &in_del, &len, &byte);
        md_m += kind == 1u ? len : kind == 2u ? 1u : 0u;
        md_bad |= (kind >= 3u || byte == '^') ? 1u : 0u;
      }
      bad = fsam_row_or(md_bad) | (fsam_row_sum64(md_m) != L ? 1u : 0u);
    }
    if (bad) { CEV_BAD(CEV_ERR_TRUTH); continue; }
    // ---- step 3: the entry's slot and its room in the planes
    CEV_COUNT(CC_T_ENTRIES);
    const uint64_t key = R.id << 1 | ((R.flag >> 7) & 1u);
    const uint32_t rev = (uint32_t)(R.flag >> 4) & 1u;
    unsigned long long slot = 0, at = 0;
    if (sub == 0u) {
      slot = atomicAdd(cursor, 1ull);
      at = atomicAdd(cursor + 2, (unsigned long long)L);
      atomicMax(cursor + 1, (unsigned long long)key);
    }
    slot = __shfl(slot, 0, (int)CEV_LANES);
    at = __shfl(at, 0, (int)CEV_LANES);
    if (slot >= capacity || at + L > P.cap) continue;  // (never: an add's entries and bases are fewer than its bytes give room for)
    uint8_t* const ot = P.ot + at;
    uint8_t* const pq = P.q + at;
    uint32_t col0 = 0, before = 0, in_del = 0;
    for (uint64_t p0 = md; p0 < md_end; p0 += CEV_LANES) {
      uint32_t len, byte;
      const uint32_t kind = fsam_md_lane(t, md, md_end, p0 + sub, sub, &in_del, &len, &byte);
      const uint32_t cm = kind == 1u ? len : kind == 2u ? 1u : 0u;
      const uint32_t ic = sam_row_scan(cm);
      const uint32_t total = sam_row_lane(ic, CEV_LANES - 1u);
      for (uint32_t c0 = 0; c0 < total; c0 += CEV_LANES) {  // (uniform over the row)
        const uint32_t c = c0 + sub;
        // the run that holds position c of the round: the first lane whose inclusive sum passes c
        uint32_t j = 0;
#pragma unroll
        for (uint32_t step = 8u; step > 0u; step >>= 1)
          if (sam_row_lane(ic, j + step - 1u) <= c) j += step;
        j = j < CEV_LANES ? j : CEV_LANES - 1u;
        const uint32_t jk = sam_row_lane(kind, j), jb = sam_row_lane(byte, j);
        const uint32_t col = col0 + c;
        if (c >= total || col >= L) continue;
        uint32_t oc = cev_class(t[seq + col]);
        uint32_t tc = jk == 2u ? cev_class(jb) : oc;
        const uint32_t qv = has_qual ? (uint32_t)t[qual + col] - 33u : 94u;
        if (rev) {
          oc = oc < 4u ? oc ^ 3u : oc;
          tc = tc < 4u ? tc ^ 3u : tc;
        }
        const uint32_t i = rev ? L - 1u - col : col;
        ot[i] = (uint8_t)(oc | tc << 3);
        pq[i] = (uint8_t)(qv < 94u ? qv : 94u);
        before += oc != tc && tc != 4u ? 1u : 0u;
      }
      col0 += total;
    }
    before = fsam_row_sum(before);
    if (sub == 0u) {
      E.key[slot] = key;
      E.len[slot] = L;
      E.off[slot] = at;
      E.before[slot] = before;
    }
  }
}

// the entry columns into key order (perm == nullptr: a key without bits, the order is the identity), and equal neighbours
extern "C" __global__ void __launch_bounds__(256)
k_cev_gather(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ perm, CevEntries U, CevEntries S, uint64_t n, uint32_t* __restrict__ err) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t from = perm ? perm[i] : i;
    if (from >= n) continue;  // (never: the sort writes a permutation)
    S.len[i] = U.len[from];
    S.off[i] = U.off[from];
    S.before[i] = U.before[from];
    if (i + 1u < n && skey[i] == skey[i + 1u]) atomicOr(err, CEV_ERR_DUP);
  }
}

// ---- the corrected records --------------------------------------------------------------------------------------------------------
// the end of line li (its '\n', or the text's end): a line ends where the next one starts, less the '\n' between them
SIMMR_DEV uint32_t cev_line_end(const MevText& W, uint64_t li, uint64_t n_lines, uint32_t start) {
  const uint64_t next = li + 1u < n_lines ? (uint64_t)W.starts[li + 1u] : W.n_bytes;
  uint32_t end = (uint32_t)(next < W.n_bytes ? next : W.n_bytes);
  if (end < start) return start;  // (never: the starts ascend)
  if (end > start && W.text[end - 1u] == '\n') end--;
  return end;
}

extern "C" __global__ void __launch_bounds__(CEV_WG)
k_cev_score(MevText W, uint32_t lpr, const uint64_t* __restrict__ skey, CevEntries S, uint64_t n_entries, CevPlanes P, unsigned long long* __restrict__ table,
            uint32_t* __restrict__ residual, uint32_t* __restrict__ hits, uint32_t* __restrict__ err) {
  __shared__ uint32_t l_tab[CT_TAIL];  // the table's words but the last, 32 bits each: an add's positions are fewer than 2^32
  const uint8_t* __restrict__ t = W.text;
  const uint32_t tid = threadIdx.x, sub = tid & (CEV_LANES - 1u), row = tid / CEV_LANES;
  for (uint32_t i = tid; i < CT_TAIL; i += CEV_WG) l_tab[i] = 0u;
  __syncthreads();
  const uint64_t n_lines = *W.n_lines, n = W.n_bytes;
  const uint64_t n_recs = n_lines / lpr;
  if (blockIdx.x == 0 && tid == 0) {
    atomicAdd(&l_tab[CC_LINES], (uint32_t)n_lines);
    if (n_lines % lpr) atomicOr(err, CEV_ERR_READS);
  }
  const uint64_t n_batches = (n_recs + CEV_WG_RECS - 1u) / CEV_WG_RECS;
#define CEV_LCOUNT(which, v) do { if (sub == 0u && (v)) atomicAdd(&l_tab[(which)], (uint32_t)(v)); } while (0)
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t ri = batch * CEV_WG_RECS + row;
    if (ri >= n_recs) continue;  // (uniform over the row)
    const uint64_t l0 = ri * lpr;
    const uint32_t s0 = W.starts[l0], s1 = W.starts[l0 + 1u];
    if (s0 >= n || s1 > n) continue;  // (never: the index holds places of the text; s1 == n never either, a line starts below n)
    CEV_LCOUNT(CC_RECORDS, 1u);
    const uint32_t e0 = cev_line_end(W, l0, n_lines, s0), e1 = cev_line_end(W, l0 + 1u, n_lines, s1);
    uint32_t bad = e0 > s0 && t[s0] == (lpr == 4u ? '@' : '>') ? 0u : 1u;
    if (lpr == 4u) {
      const uint32_t s2 = W.starts[l0 + 2u], s3 = W.starts[l0 + 3u];
      if (s2 >= n || s3 > n) continue;  // (never)
      const uint32_t e2 = cev_line_end(W, l0 + 2u, n_lines, s2), e3 = cev_line_end(W, l0 + 3u, n_lines, s3);
      if (!(e2 > s2 && t[s2] == '+') || e3 - s3 != e1 - s1) bad = 1u;
    }
    if (bad) { CEV_BAD(CEV_ERR_READS); continue; }
    // ---- the name: behind the first character, up to the first blank or the line's end
    uint32_t name_end = e0;
    for (uint32_t p0 = s0 + 1u; p0 < e0; p0 += CEV_LANES) {  // (uniform over the row)
      const uint32_t p = p0 + sub;
      const uint32_t c = p < e0 ? t[p] : 0u;
      const uint32_t m = fsam_ballot(c == ' ' || c == '\t');
      if (m) { name_end = p0 + (uint32_t)__builtin_ctz(m); break; }
    }
    uint64_t key = 0;
    if (!ove_name_key(t, s0 + 1u, name_end, &key)) { CEV_LCOUNT(CC_UNKNOWN_READ, 1u); continue; }
    const uint64_t at = mev_lower_bound(skey, n_entries, key, sub);
    if (at >= n_entries || skey[at] != key) { CEV_LCOUNT(CC_UNKNOWN_READ, 1u); continue; }
    const uint32_t L = S.len[at], Lc = e1 - s1, m_cmp = L < Lc ? L : Lc;
    const uint64_t off = S.off[at];
    if (off + L > P.cap) continue;  // (never: the truth writer planned the entry inside the planes)
    const uint8_t* const ot = P.ot + off;
    const uint8_t* const pq = P.q + off;
    // ---- the positions: verdict v = 0 kept, 1 damaged, 2 fixed, 3 left, 4 miscorrected, 5 ambiguous, 6 trimmed_error, 7 trimmed_clean
    uint32_t kept_b[4] = {0u, 0u, 0u, 0u}, sum[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t i0 = 0; i0 < L; i0 += CEV_LANES) {  // (uniform over the row)
      const uint32_t i = i0 + sub;
      uint32_t v = 8u, o = 0, tt = 0, c = 0, q = 0;
      if (i < L) {
        const uint32_t pv = ot[i];
        q = pq[i];
        q = q < CEV_QUALS ? q : CEV_QUALS - 1u;
        o = pv & 7u;
        tt = (pv >> 3) & 7u;
        o = o < 4u ? o : 4u;
        tt = tt < 4u ? tt : 4u;
        if (i < Lc) {
          c = cev_class(t[s1 + i]);
          v = tt == 4u ? 5u : o == tt ? (c == tt ? 0u : 1u) : (c == tt ? 2u : c == o ? 3u : 4u);
        } else {
          v = tt == 4u ? 5u : o != tt ? 6u : 7u;
        }
      }
      // kept: by base from four ballots, by quality one LDS atomic per distinct quality of the round
#pragma unroll
      for (uint32_t b = 0; b < 4u; b++) kept_b[b] += (uint32_t)__popc(fsam_ballot(v == 0u && tt == b));
      uint32_t m = fsam_ballot(v == 0u);
      while (m) {  // (uniform over the row)
        const uint32_t lead = (uint32_t)__builtin_ctz(m);
        const uint32_t ql = sam_row_lane(q, lead);
        const uint32_t same = fsam_ballot(v == 0u && q == ql);
        if (sub == lead) atomicAdd(&l_tab[CT_QUAL + ql * 5u], (uint32_t)__popc(same));
        m &= ~same;
      }
      // everything else is rare
      if (fsam_ballot(v != 0u && v != 8u)) {
#pragma unroll
        for (uint32_t k = 0; k < 7u; k++) sum[k] += (uint32_t)__popc(fsam_ballot(v == k + 1u));
        if (v >= 1u && v <= 5u) {
          const uint32_t pr = i < CEV_POS - 1u ? i : CEV_POS - 1u;
          atomicAdd(&l_tab[CT_CUBE + tt * 25u + o * 5u + c], 1u);
          atomicAdd(&l_tab[CT_POS + pr * 5u], 1u);
          if (v <= 4u) {
            atomicAdd(&l_tab[CT_POS + pr * 5u + v], 1u);
            atomicAdd(&l_tab[CT_QUAL + q * 5u + v], 1u);
          }
        }
      }
    }
    // ---- the record's sums
    const uint32_t kept = kept_b[0] + kept_b[1] + kept_b[2] + kept_b[3], extra = Lc > L ? Lc - L : 0u;
    if (sub < 4u) {
      const uint32_t mine = sub == 0u ? kept_b[0] : sub == 1u ? kept_b[1] : sub == 2u ? kept_b[2] : kept_b[3];
      if (mine) atomicAdd(&l_tab[CT_CUBE + sub * 31u], mine);  // cube[b][b][b]
    }
    CEV_LCOUNT(CC_SCORED, 1u);
    CEV_LCOUNT(CC_TRIMMED_RECORDS, Lc < L ? 1u : 0u);
    CEV_LCOUNT(CC_LONGER_RECORDS, Lc > L ? 1u : 0u);
    CEV_LCOUNT(CC_COMPARED, m_cmp);
    CEV_LCOUNT(CC_KEPT, kept);
#pragma unroll
    for (uint32_t k = 0; k < 7u; k++) CEV_LCOUNT(CC_DAMAGED + k, sum[k]);
    CEV_LCOUNT(CC_EXTRA, extra);
    if (sub == 0u) {
      atomicAdd(&l_tab[CT_LEN + (m_cmp < CEV_POS ? m_cmp : CEV_POS)], 1u);
      if (m_cmp > CEV_POS - 1u) atomicAdd(table + CT_TAIL, (unsigned long long)(m_cmp - (CEV_POS - 1u)));
      const uint64_t res = (uint64_t)sum[0] + sum[2] + sum[3] + sum[5] + sum[6] + extra;
      atomicMin(residual + at, res < 0xfffffffeull ? (uint32_t)res : 0xfffffffeu);
      atomicAdd(hits + at, 1u);
    }
  }
#undef CEV_LCOUNT
  __syncthreads();
  for (uint32_t i = tid; i < CT_TAIL; i += CEV_WG) {
    const uint32_t v = l_tab[i];
    if (v) atomicAdd(table + i, (unsigned long long)v);
  }
}

// ---- the entries by what became of them -----------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
k_cev_reduce(const uint32_t* __restrict__ hits, const uint32_t* __restrict__ residual, const uint32_t* __restrict__ before, uint64_t n,
             unsigned long long* __restrict__ counts) {
  __shared__ uint32_t l_sum[8];
  if (threadIdx.x < 8u) l_sum[threadIdx.x] = 0u;
  __syncthreads();
  for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += (uint64_t)gridDim.x * 256u) {  // (uniform over the workgroup)
    const uint64_t i = i0 + threadIdx.x;
    uint32_t cls = 8u, many = 0u;  // 0 missing, 2 clean_kept, 3 clean_damaged, 4 fixed_all, 5 improved, 6 unchanged, 7 worse; 1 multiple goes beside them
    if (i < n) {
      const uint32_t h = hits[i], r = residual[i], b = before[i];
      many = h > 1u ? 1u : 0u;
      if (h == 0u) cls = 0u;
      else if (b == 0u) cls = r == 0u ? 2u : 3u;
      else cls = r == 0u ? 4u : r < b ? 5u : r == b ? 6u : 7u;
    }
#pragma unroll
    for (uint32_t j = 0; j < 8u; j++) {
      const uint32_t m = (uint32_t)__popcll(__ballot(j == 1u ? many != 0u : cls == j));
      if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&l_sum[j], m);
    }
    __syncthreads();
    if (threadIdx.x < 8u && l_sum[threadIdx.x]) {
      atomicAdd(counts + CC_MISSING + threadIdx.x, (unsigned long long)l_sum[threadIdx.x]);
      l_sum[threadIdx.x] = 0u;
    }
    __syncthreads();
  }
}

#undef CEV_COUNT
#undef CEV_BAD

}  // namespace simmr
