// fit_sam_kernels.hip — the front of the model fit for a user's SAM file (gfx950): SAM text in HBM to the tables of
// fit_device.hpp (include/simmr_hip.h states every rule: the filters, the rows, the orientation, what is malformed).
// Included by fit_sam.hip, a translation unit of its own beside fit.hip, whose kernels and budgets stay what they were; and, with
// FSAM_ROUTINES_ONLY defined, by mapeval_kernels.hip, which takes the reader's routines without the six kernels.
//
// Six kernels; a work item past the line index is a LINE or a TAKEN record, shared by FSAM_LANES = 16 lanes (one DPP row).
//   k_fsam_index    the line index.  A tile is FSAM_TILE = 4096 bytes, 16 per thread.  A byte starts a line when it is not
//                   '\n' and stands first or behind a '\n' (empty lines never enter the index).  Launched twice: to count a
//                   tile's starts, and, after the chunked scan over the tile counts, to write them at their places.
//   k_fsam_scan     ONE workgroup: the chunked scan of sam_kernels.hip over the tile counts; the entry behind the last tile
//                   is the number of lines, which stays on the device (the add only enqueues).
//   k_fsam_record   a line per lane group.  The group reads the line 16 bytes a round and takes the tabs and the '\n' from a
//                   ballot; the 11 mandatory fields and MD:Z: are group-uniform positions.  FLAG, MAPQ and TLEN are parsed by
//                   every lane; CIGAR and MD are summed bytewise — the lane that holds an op (or the last digit of an MD number)
//                   reads its at most nine digits backwards — so a record with hundreds of runs costs rounds, not a lane's
//                   loop.  Whether an MD letter is a deleted base is the nearest non-letter before it, from the ballot and a
//                   carry.  Then the filters in the header's order, the length, insert and quality histograms (offsets below
//                   FIT_LDS_POS privatised in LDS, added to HBM when the workgroup ends) and the counts.  A taken alignment
//                   gets a descriptor and `columns` bytes of the row buffer, both from an atomic cursor: the order is arbitrary
//                   and nothing depends on it, every table being an integer sum.
//   k_fsam_md       a taken record per group: MD's mismatch and deleted letters as class codes + 1 into the record's share of
//                   the side buffer (zero: a match), at the index their prefix sums give.
//   k_fsam_expand   the two rows: per round of 16 CIGAR bytes the runs' column, query, match and deletion offsets by four
//                   row scans; the round's columns are then dealt to the 16 lanes, each finding its run by a search in the
//                   lanes' inclusive sums, so one long run and three hundred short ones balance alike.  A column is one byte,
//                   reference class | query class << 3, written in the read's orientation.
//   k_fsam_windows  k_fit_add's roll over the rows (a second copy: k_fit_add's registers stay its own), the dense table
//                   privatised in LDS for k <= FIT_LDS_K.
// Bounds.  Every load of text is below n_bytes and, past the field scan, inside the line's fields; every store of a record is
// below its planned columns (`cols`, `n_m`, `n_d` of its descriptor), whatever the text says on the second reading.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#include "fit_device.hpp"
#define SAM_ROUTINES_ONLY
#include "sam_kernels.hip"  // sam_wg_scan, sam_scan_chunks, sam_row_scan: the scans' bodies without the kernels

namespace simmr {

#define FSAM_LANES 16u
#define FSAM_WG 256u
#define FSAM_WG_RECS 16u       /* lines or records per workgroup and batch */
#define FSAM_TILE 4096u        /* bytes of a line-index tile */
#define FSAM_MIN_TAKEN 28u     /* the shortest line of a taken alignment: 11 one-byte fields, 10 tabs, "\tMD:Z:0" */
#define FSAM_NONE 0xffffffffu

enum { FC_LINES = 0, FC_HEADER, FC_RECORDS, FC_TAKEN_Q, FC_TAKEN_ALN, FC_NO_SEQ, FC_SECONDARY, FC_TOO_LONG, FC_UNMAPPED, FC_MAPQ0,
       FC_MATE_UNMAPPED, FC_NO_MD, FC_INSERT, FC_CIGAR_OP, FC_INCONSISTENT };
static_assert(FC_INCONSISTENT + 1 == FIT_SAM_COUNTS && sizeof(simmr_fit_sam_counts) == FIT_SAM_COUNTS * 8u, "the counts in the header's order");

struct FsamRec {  // a taken alignment (byte offsets into the text)
  uint32_t cigar, cigar_end, md, md_end, seq, L, rev, cols, n_m, n_d;
  uint64_t row;   // its first byte in the row buffer and in the side buffer
};

struct FsamWork {
  const uint8_t* text;
  uint64_t n_bytes;
  const uint64_t* n_lines;     // the scan's last entry
  const uint32_t* starts;      // [lines]
  FsamRec* recs;
  uint64_t rec_capacity;
  uint8_t* rows;               // [row_capacity + 16]
  uint8_t* side;               // [row_capacity], zeroed before every add
  uint64_t row_capacity;
  unsigned long long* cursor;  // [0] taken records, [1] row bytes; zeroed before every add
};

// the 16 bits of the lane's group in a ballot of the wave
SIMMR_DEV uint32_t fsam_ballot(bool p) {
  const uint64_t b = __ballot(p);
  return (uint32_t)(b >> (threadIdx.x & 48u)) & 0xffffu;
}
SIMMR_DEV uint32_t fsam_row_sum(uint32_t v) {
  for (uint32_t d = 1; d < FSAM_LANES; d <<= 1) v += (uint32_t)__shfl_xor((int)v, (int)d, (int)FSAM_LANES);
  return v;
}
SIMMR_DEV uint64_t fsam_row_sum64(uint64_t v) {
  for (uint32_t d = 1; d < FSAM_LANES; d <<= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, (int)d, (int)FSAM_LANES);
  return v;
}
SIMMR_DEV uint32_t fsam_row_or(uint32_t v) {
  for (uint32_t d = 1; d < FSAM_LANES; d <<= 1) v |= (uint32_t)__shfl_xor((int)v, (int)d, (int)FSAM_LANES);
  return v;
}
SIMMR_DEV bool fsam_digit(uint32_t c) { return c - '0' <= 9u; }

// the one to nine digits that end before byte p and start at or behind a; false: none, or more than nine
SIMMR_DEV bool fsam_number_before(const uint8_t* __restrict__ t, uint32_t a, uint32_t p, uint32_t* v) {
  uint32_t val = 0, mul = 1, n = 0;
  while (p > a) {
    const uint32_t d = (uint32_t)t[p - 1u] - '0';
    if (d > 9u) break;
    if (n == 9u) return false;
    val += d * mul;
    mul *= 10u;
    n++;
    p--;
  }
  *v = val;
  return n > 0u;
}

// a decimal field [a, b): an optional '-' where `sign`, then one to eighteen digits
SIMMR_DEV bool fsam_field_number(const uint8_t* __restrict__ t, uint32_t a, uint32_t b, bool sign, uint64_t* v) {
  if (sign && a < b && t[a] == '-') a++;
  if (a >= b || b - a > 18u) return false;
  uint64_t val = 0;
  for (uint32_t p = a; p < b; p++) {
    const uint32_t d = (uint32_t)t[p] - '0';
    if (d > 9u) return false;
    val = val * 10u + d;
  }
  *v = val;
  return true;
}

// ---- the byte a lane holds in a round over CIGAR or MD ----------------------------------------------------------------------
// CIGAR byte p of [a, b): kind 0 none (a digit, or outside), 1 M = X, 2 I, 3 D, 4 S, 5 H, 6 another op, 7 an op without its number
SIMMR_DEV uint32_t fsam_cigar_lane(const uint8_t* __restrict__ t, uint32_t a, uint32_t b, uint64_t p, uint32_t* n) {
  *n = 0;
  if (p >= b) return 0u;
  const uint32_t c = t[p];
  if (fsam_digit(c)) return 0u;
  if (!fsam_number_before(t, a, (uint32_t)p, n)) { *n = 0; return 7u; }
  switch (c) {
    case 'M': case '=': case 'X': return 1u;
    case 'I': return 2u;
    case 'D': return 3u;
    case 'S': return 4u;
    case 'H': return 5u;
    default: return 6u;
  }
}

// MD byte p of [a, b): kind 0 none, 1 the last digit of a number (*n its value), 2 a mismatch letter, 3 a deleted letter, 4 a byte
// MD does not have or a number of more than nine digits.  in_del: whether a letter at the round's first byte continues a '^' run
// (group-uniform, carried to the next round).
SIMMR_DEV uint32_t fsam_md_lane(const uint8_t* __restrict__ t, uint32_t a, uint32_t b, uint64_t p, uint32_t sub, uint32_t* in_del, uint32_t* n,
                                uint32_t* byte) {
  const bool in = p < b;
  const uint32_t c = in ? t[p] : 0u;
  const bool dig = in && fsam_digit(c), let = in && c - 'A' < 26u, car = in && c == '^';
  const uint32_t m_let = fsam_ballot(let), m_car = fsam_ballot(car), non = ~m_let & 0xffffu;
  const uint32_t below = non & ((1u << sub) - 1u);
  const uint32_t del = below ? (m_car >> (31u - (uint32_t)__clz((int)below))) & 1u : *in_del;
  *in_del = non ? (m_car >> (31u - (uint32_t)__clz((int)non))) & 1u : *in_del;
  *n = 0;
  *byte = c;
  if (!in) return 0u;
  if (let) return del ? 3u : 2u;
  if (car) return 0u;
  if (!dig) return 4u;
  if (p + 1u < b && fsam_digit(t[p + 1u])) return 0u;
  return fsam_number_before(t, a, (uint32_t)p + 1u, n) ? 1u : 4u;
}

// ---- the line index -----------------------------------------------------------------------------------------------------------
// The bodies of the index's two kernels as device routines: mapeval_kernels.hip (a translation unit of its own) includes this
// file with FSAM_ROUTINES_ONLY defined and wraps them in kernels of its own, as sam_sort_kernels.hip does with sam_kernels.hip.
SIMMR_DEV void fsam_index_tiles(const uint8_t* __restrict__ text, uint64_t n_bytes, uint64_t n_tiles, uint64_t* __restrict__ tile_sum,
                                const uint64_t* __restrict__ tile_prefix, uint32_t* __restrict__ starts, uint64_t start_capacity, uint32_t* lds) {
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // (uniform over the workgroup)
    const uint64_t p0 = tile * FSAM_TILE + 16u * threadIdx.x;
    uint32_t mask = 0;
    if (p0 < n_bytes) {
      uint32_t prev = p0 ? text[p0 - 1u] : '\n';
      for (uint32_t b = 0; b < 16u && p0 + b < n_bytes; b++) {
        const uint32_t c = text[p0 + b];
        if (prev == '\n' && c != '\n') mask |= 1u << b;
        prev = c;
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

#ifndef FSAM_ROUTINES_ONLY
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_fsam_index(const uint8_t* __restrict__ text, uint64_t n_bytes, uint64_t n_tiles, uint64_t* __restrict__ tile_sum,
             const uint64_t* __restrict__ tile_prefix, uint32_t* __restrict__ starts, uint64_t start_capacity) {
  __shared__ uint32_t lds[FSAM_WG];
  fsam_index_tiles(text, n_bytes, n_tiles, tile_sum, tile_prefix, starts, start_capacity, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_fsam_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

// ---- the records --------------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_fsam_record(FsamWork W, uint32_t n_sets, FitTables T, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t l_q[FIT_LDS_POS * FIT_Q_STRIDE];
  const uint8_t* __restrict__ t = W.text;
  const uint32_t tid = threadIdx.x, sub = tid & (FSAM_LANES - 1u), row = tid / FSAM_LANES;
  for (uint32_t i = tid; i < FIT_LDS_POS * FIT_Q_STRIDE; i += FSAM_WG) l_q[i] = 0u;
  __syncthreads();
  const uint64_t n_lines = *W.n_lines, n = W.n_bytes;
  const uint64_t n_batches = (n_lines + FSAM_WG_RECS - 1u) / FSAM_WG_RECS;
#define FSAM_COUNT(which) do { if (sub == 0u) atomicAdd(counts + (which), 1ull); } while (0)
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t li = batch * FSAM_WG_RECS + row;
    if (li >= n_lines) continue;  // (uniform over the row)
    const uint32_t line = W.starts[li];
    if (line >= n) continue;      // (never: the index holds places of the text)
    FSAM_COUNT(FC_LINES);
    if (t[line] == '@') { FSAM_COUNT(FC_HEADER); continue; }
    FSAM_COUNT(FC_RECORDS);
    // ---- the fields: tab j ends field j; the line ends at its '\n' or at the text's end
    uint32_t tb[11];
#pragma unroll
    for (uint32_t j = 0; j < 11u; j++) tb[j] = FSAM_NONE;
    uint32_t n_tab = 0, md = FSAM_NONE, md_end = FSAM_NONE, end = (uint32_t)n;
    for (uint64_t p0 = line;; p0 += FSAM_LANES) {
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
    if (n_tab < 10u) { if (sub == 0u) atomicOr(T.err, FIT_ERR_SAM); continue; }
    const uint32_t qual = tb[9] + 1u, qual_end = n_tab > 10u ? tb[10] : end;
    const uint32_t seq = tb[8] + 1u, seq_end = tb[9], cigar = tb[4] + 1u, cigar_end = tb[5];
    uint64_t flag = 0, mapq = 0, tlen = 0;
    const bool numbers = fsam_field_number(t, tb[0] + 1u, tb[1], false, &flag) && fsam_field_number(t, tb[3] + 1u, tb[4], false, &mapq) &&
                         fsam_field_number(t, tb[7] + 1u, tb[8], true, &tlen);
    // ---- CIGAR: the sums by op class, and its syntax
    const bool cigar_star = cigar_end - cigar == 1u && t[cigar] == '*';
    uint32_t bad = numbers && cigar_end > cigar ? 0u : 1u;
    uint64_t s_m = 0, s_i = 0, s_d = 0, s_s = 0;
    uint32_t other = 0;
    if (!cigar_star && !bad) {
      if (fsam_digit(t[cigar_end - 1u])) bad = 1u;
      for (uint64_t p0 = cigar; p0 < cigar_end; p0 += FSAM_LANES) {
        uint32_t len;
        const uint32_t kind = fsam_cigar_lane(t, cigar, cigar_end, p0 + sub, &len);
        s_m += kind == 1u ? len : 0u;
        s_i += kind == 2u ? len : 0u;
        s_d += kind == 3u ? len : 0u;
        s_s += kind == 4u ? len : 0u;
        other |= kind == 6u ? 1u : 0u;
        bad |= kind == 7u ? 1u : 0u;
      }
      bad = fsam_row_or(bad);
      other = fsam_row_or(other);
    }
    // ---- SEQ, QUAL
    const bool seq_star = seq_end - seq == 1u && t[seq] == '*';
    const bool qual_star = qual_end - qual == 1u && t[qual] == '*';
    const uint32_t L = seq_star ? 0u : seq_end - seq;
    if (!qual_star && qual_end - qual != L) bad = 1u;
    if (seq_end == seq) bad = 1u;  // (an empty SEQ field: QUAL cannot be as long as nothing and be a field)
    const uint32_t rev = (uint32_t)(flag >> 4) & 1u;
    // filters 1 .. 3; step 4 runs with the QUAL check, which every record gets
    uint32_t stop = 0;
    if (!bad) {
      if (seq_star) { FSAM_COUNT(FC_NO_SEQ); stop = 1u; }
      else if (flag & 0x900u) { FSAM_COUNT(FC_SECONDARY); stop = 1u; }
      else if (L > SIMMR_FIT_MAX_L) { FSAM_COUNT(FC_TOO_LONG); stop = 1u; }
    }
    if (!bad && !qual_star) {
      uint32_t bad_q = 0;
      for (uint32_t i0 = 0; i0 < L; i0 += FSAM_LANES) {
        const uint32_t i = i0 + sub;
        if (i >= L) continue;
        const uint32_t q = (uint32_t)t[qual + (rev ? L - 1u - i : i)] - 33u;
        if (q > SIMMR_FIT_MAX_Q) { bad_q = 1u; continue; }
        if (stop) continue;
        if (i < FIT_LDS_POS) atomicAdd(&l_q[i * FIT_Q_STRIDE + q], 1u);
        else atomicAdd(T.qhist + (uint64_t)i * SIMMR_FIT_QUALS + q, 1ull);
      }
      bad = fsam_row_or(bad_q);
    }
    if (bad) { if (sub == 0u) atomicOr(T.err, FIT_ERR_SAM); continue; }
    if (stop) continue;
    FSAM_COUNT(FC_TAKEN_Q);
    if (sub == 0u) atomicAdd(T.lhist + L, 1ull);
    // ---- filters 5 .. 10
    const uint64_t ins = tlen;  // |TLEN|
    if (flag & 4u) { FSAM_COUNT(FC_UNMAPPED); continue; }
    if (mapq == 0u) { FSAM_COUNT(FC_MAPQ0); continue; }
    if (n_sets == 2u && tlen == 0u && (flag & 8u)) { FSAM_COUNT(FC_MATE_UNMAPPED); continue; }
    if (md == FSAM_NONE) { FSAM_COUNT(FC_NO_MD); continue; }
    if (n_sets == 2u && ins > SIMMR_FIT_MAX_INSERT) { FSAM_COUNT(FC_INSERT); continue; }
    if (n_sets == 2u && sub == 0u) atomicAdd(T.ihist + ins, 1ull);
    // ---- step 11: the alignment
    if (cigar_star || other) { FSAM_COUNT(FC_CIGAR_OP); continue; }
    uint64_t md_m = 0, md_d = 0;
    uint32_t md_bad = 0, in_del = 0;
    for (uint64_t p0 = md; p0 < md_end; p0 += FSAM_LANES) {
      uint32_t len, byte;
      const uint32_t kind = fsam_md_lane(t, md, md_end, p0 + sub, sub, &in_del, &len, &byte);
      md_m += kind == 1u ? len : kind == 2u ? 1u : 0u;
      md_d += kind == 3u ? 1u : 0u;
      md_bad |= kind == 4u ? 1u : 0u;
    }
    md_bad = fsam_row_or(md_bad);
    const uint64_t tot[6] = {fsam_row_sum64(s_m), fsam_row_sum64(s_i), fsam_row_sum64(s_d), fsam_row_sum64(s_s), fsam_row_sum64(md_m), fsam_row_sum64(md_d)};
    const uint64_t cols = tot[0] + tot[1] + tot[2];
    if (md_bad || tot[0] + tot[1] + tot[3] != L || tot[4] != tot[0] || tot[5] != tot[2] || cols > 0xffffffffull) {
      FSAM_COUNT(FC_INCONSISTENT);
      continue;
    }
    FSAM_COUNT(FC_TAKEN_ALN);
    if (sub == 0u) {
      const unsigned long long slot = atomicAdd(W.cursor, 1ull), at = atomicAdd(W.cursor + 1, (unsigned long long)cols);
      if (slot < W.rec_capacity && at + cols <= W.row_capacity)
        W.recs[slot] = FsamRec{cigar, cigar_end, md, md_end, seq, L, rev, (uint32_t)cols, (uint32_t)tot[0], (uint32_t)tot[2], at};
      else if (slot < W.rec_capacity)
        W.recs[slot] = FsamRec{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // (never: a line's columns are fewer than its bytes)
    }
  }
#undef FSAM_COUNT
  __syncthreads();
  for (uint32_t i = tid; i < FIT_LDS_POS * FIT_Q_STRIDE; i += FSAM_WG) {
    const uint32_t v = l_q[i];
    if (v) atomicAdd(T.qhist + (uint64_t)(i / FIT_Q_STRIDE) * SIMMR_FIT_QUALS + i % FIT_Q_STRIDE, (unsigned long long)v);
  }
}

// the taken records of this add (the cursor may have counted past the descriptors: never, see FSAM_MIN_TAKEN)
SIMMR_DEV uint64_t fsam_taken(const FsamWork& W) {
  const uint64_t n = W.cursor[0];
  return n < W.rec_capacity ? n : W.rec_capacity;
}

// ---- MD's letters -------------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_fsam_md(FsamWork W) {
  const uint8_t* __restrict__ t = W.text;
  const uint32_t sub = threadIdx.x & (FSAM_LANES - 1u), row = threadIdx.x / FSAM_LANES;
  const uint64_t n_recs = fsam_taken(W), n_batches = (n_recs + FSAM_WG_RECS - 1u) / FSAM_WG_RECS;
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t ri = batch * FSAM_WG_RECS + row;
    if (ri >= n_recs) continue;  // (uniform over the row)
    const FsamRec R = W.recs[ri];
    if (R.md_end > W.n_bytes || R.md > R.md_end) continue;
    uint8_t* const side = W.side + R.row;
    uint32_t m0 = 0, d0 = 0, in_del = 0;
    for (uint64_t p0 = R.md; p0 < R.md_end; p0 += FSAM_LANES) {
      uint32_t len, byte;
      const uint32_t kind = fsam_md_lane(t, R.md, R.md_end, p0 + sub, sub, &in_del, &len, &byte);
      const uint32_t cm = kind == 1u ? len : kind == 2u ? 1u : 0u, cd = kind == 3u ? 1u : 0u;
      const uint32_t im = sam_row_scan(cm), id = sam_row_scan(cd);
      const uint32_t code = fit_class(byte, 4u, 4u) + 1u;
      if (kind == 2u && m0 + (im - cm) < R.n_m) side[m0 + (im - cm)] = (uint8_t)code;
      if (kind == 3u && d0 + (id - cd) < R.n_d) side[(uint64_t)R.n_m + d0 + (id - cd)] = (uint8_t)code;
      m0 += sam_row_lane(im, FSAM_LANES - 1u);
      d0 += sam_row_lane(id, FSAM_LANES - 1u);
    }
  }
}

// ---- the rows -----------------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_fsam_expand(FsamWork W) {
  const uint8_t* __restrict__ t = W.text;
  const uint32_t sub = threadIdx.x & (FSAM_LANES - 1u), row = threadIdx.x / FSAM_LANES;
  const uint64_t n_recs = fsam_taken(W), n_batches = (n_recs + FSAM_WG_RECS - 1u) / FSAM_WG_RECS;
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t ri = batch * FSAM_WG_RECS + row;
    if (ri >= n_recs) continue;  // (uniform over the row)
    const FsamRec R = W.recs[ri];
    if (R.cigar_end > W.n_bytes || R.cigar > R.cigar_end || (uint64_t)R.seq + R.L > W.n_bytes) continue;
    const uint8_t* const side = W.side + R.row;
    uint8_t* const rows = W.rows + R.row;
    uint32_t col0 = 0, q0 = 0, m0 = 0, d0 = 0;
    for (uint64_t p0 = R.cigar; p0 < R.cigar_end; p0 += FSAM_LANES) {
      uint32_t len;
      const uint32_t kind = fsam_cigar_lane(t, R.cigar, R.cigar_end, p0 + sub, &len);
      const uint32_t cc = kind >= 1u && kind <= 3u ? len : 0u, cq = kind == 1u || kind == 2u || kind == 4u ? len : 0u;
      const uint32_t cm = kind == 1u ? len : 0u, cd = kind == 3u ? len : 0u;
      const uint32_t ic = sam_row_scan(cc), iq = sam_row_scan(cq), im = sam_row_scan(cm), id = sam_row_scan(cd);
      const uint32_t total = sam_row_lane(ic, FSAM_LANES - 1u);
      for (uint32_t c0 = 0; c0 < total; c0 += FSAM_LANES) {  // (uniform over the row)
        const uint32_t c = c0 + sub;
        // the run that holds column c of the round: the first lane whose inclusive sum passes c
        uint32_t j = 0;
#pragma unroll
        for (uint32_t step = 8u; step > 0u; step >>= 1)
          if (sam_row_lane(ic, j + step - 1u) <= c) j += step;
        j = j < FSAM_LANES ? j : FSAM_LANES - 1u;
        const uint32_t jk = sam_row_lane(kind, j), jlen = sam_row_lane(cc, j);
        const uint32_t jc = sam_row_lane(ic, j) - jlen, jq = sam_row_lane(iq - cq, j), jm = sam_row_lane(im - cm, j), jd = sam_row_lane(id - cd, j);
        if (c >= total) continue;
        const uint32_t r = c - jc, col = col0 + c;
        uint32_t refc = 4u, qc = 4u;
        if (jk == 1u || jk == 2u) {
          const uint32_t qi = q0 + jq + r;
          const uint32_t qb = qi < R.L ? t[R.seq + qi] : 'N';
          qc = fit_class(qb, 4u, 5u);
          if (jk == 1u) {
            const uint32_t mi = m0 + jm + r;
            const uint32_t mdv = mi < R.n_m ? side[mi] : 5u;
            refc = mdv ? mdv - 1u : fit_class(qb, 4u, 4u);
          }
        } else if (jk == 3u) {
          const uint32_t di = d0 + jd + r;
          const uint32_t mdv = di < R.n_d ? side[(uint64_t)R.n_m + di] : 5u;
          refc = mdv ? mdv - 1u : 4u;
        }
        if (col >= R.cols) continue;
        if (R.rev) {
          refc = refc < 4u ? refc ^ 3u : refc;
          qc = qc < 4u ? qc ^ 3u : qc;
        }
        rows[R.rev ? R.cols - 1u - col : col] = (uint8_t)(refc | qc << 3);
      }
      col0 += total;
      q0 += sam_row_lane(iq, FSAM_LANES - 1u);
      m0 += sam_row_lane(im, FSAM_LANES - 1u);
      d0 += sam_row_lane(id, FSAM_LANES - 1u);
    }
  }
}

// ---- the windows: k_fit_add's roll over two rows of class codes ----------------------------------------------------------------
// A 32-bit partial of the LDS dense table gains at most 2 per column: a workgroup adds it to HBM before the columns it has
// taken since could pass 2^31, and a batch that could pass it alone counts in HBM directly.
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_fsam_windows(FsamWork W, FitTables T) {
  __shared__ uint32_t l_dense[FIT_DENSE_LDS];
  __shared__ unsigned long long l_cols[2];
  const uint32_t tid = threadIdx.x, sub = tid & (FSAM_LANES - 1u), row = tid / FSAM_LANES;
  const uint32_t k = T.k, kmask = (1u << k) - 1u, top2 = 2u * (k - 1u), top3 = 3u * (k - 1u);
  const uint32_t n_dense_lds = k <= FIT_LDS_K ? 1u << (2u * k) : 0u;
  for (uint32_t i = tid; i < FIT_DENSE_LDS; i += FSAM_WG) l_dense[i] = 0u;
  if (tid == 0) l_cols[0] = l_cols[1] = 0ull;
  __syncthreads();
  const uint64_t n_recs = fsam_taken(W), n_batches = (n_recs + FSAM_WG_RECS - 1u) / FSAM_WG_RECS;
  uint64_t since_flush = 0;
  uint32_t turn = 0;
  for (uint64_t batch = blockIdx.x;; batch += gridDim.x, turn ^= 1u) {  // (uniform over the workgroup)
    const bool more = batch < n_batches;
    const uint64_t ri = batch * FSAM_WG_RECS + row;
    const bool mine_rec = more && ri < n_recs;
    FsamRec R{};
    if (mine_rec) R = W.recs[ri];
    if (mine_rec && R.row + R.cols > W.row_capacity) R.cols = 0u;  // (never)
    // the batch's columns: summed in the slot of this turn; the other slot, read a turn ago and added to a turn from now, is cleared
    if (mine_rec && sub == 0u) atomicAdd(&l_cols[turn], (unsigned long long)R.cols);
    __syncthreads();
    const uint64_t batch_cols = l_cols[turn];
    if (tid == 0) l_cols[turn ^ 1u] = 0ull;
    __syncthreads();
    const bool direct = batch_cols >= (1ull << 30);
    if (!more || (!direct && since_flush + batch_cols >= (1ull << 30))) {
      for (uint32_t i = tid; i < n_dense_lds; i += FSAM_WG) {
        const uint32_t v = l_dense[i];
        if (v) { atomicAdd(T.dense + i, (unsigned long long)v); l_dense[i] = 0u; }
      }
      __syncthreads();
      since_flush = 0;
      if (!more) break;
    }
    const bool dense_lds = n_dense_lds != 0u && !direct;
    if (dense_lds) since_flush += batch_cols;
    if (!mine_rec) continue;  // (uniform over the row)
    const uint8_t* const rows = W.rows + R.row;
    const uint32_t L = R.cols, n_groups = (L + 15u) >> 4;
    uint64_t carry_w = 0, carry_h = 0;  // lane 15's packs of the round before
    for (uint32_t g0 = 0; g0 < n_groups; g0 += FSAM_LANES) {  // (uniform over the row: every lane of it takes the shuffles)
      const uint32_t grp = g0 + sub;
      const bool mine = grp < n_groups;
      uint64_t pw = 0, ph = 0;  // the classes of columns 16 grp .. 16 grp + 15, three bits each
      if (mine) {
        const v4u32 v = *reinterpret_cast<const v4u32_unaligned*>(rows + 16u * (uint64_t)grp);  // (the buffer has 16 bytes of slack)
#pragma unroll
        for (uint32_t b = 0; b < 16u; b++) {
          const uint32_t x = FIT_BYTE(v, b);
          pw |= (uint64_t)(x & 7u) << (3u * b);
          ph |= (uint64_t)((x >> 3) & 7u) << (3u * b);
        }
      }
      uint64_t left_w = __shfl_up((unsigned long long)pw, 1u, (int)FSAM_LANES), left_h = __shfl_up((unsigned long long)ph, 1u, (int)FSAM_LANES);
      if (sub == 0u) { left_w = carry_w; left_h = carry_h; }
      carry_w = __shfl((unsigned long long)pw, (int)FSAM_LANES - 1, (int)FSAM_LANES);
      carry_h = __shfl((unsigned long long)ph, (int)FSAM_LANES - 1, (int)FSAM_LANES);
      if (!mine) continue;
      // roll: ref2 / ref3 / alt3 hold the last k columns, the masks one bit per column of them (all ones: not k columns yet)
      uint32_t ref2 = 0, ref3 = 0, alt3 = 0, ref_bad = kmask, alt_gap = 0, alt_bad = 0;
      const uint32_t e0 = grp * 16u, n_own = L - e0 < 16u ? L - e0 : 16u;
      for (uint32_t i = grp ? 17u - k : 16u; i < 16u + n_own; i++) {  // the k - 1 columns before the group, then its own
        const uint64_t sw = i < 16u ? left_w : pw, sh = i < 16u ? left_h : ph;
        const uint32_t at = 3u * (i & 15u), wc = (uint32_t)(sw >> at) & 7u, hc = (uint32_t)(sh >> at) & 7u;
        ref2 = (ref2 >> 2) | ((wc & 3u) << top2);
        ref3 = (ref3 >> 3) | (wc << top3);
        alt3 = (alt3 >> 3) | ((hc > 4u ? 4u : hc) << top3);
        ref_bad = ((ref_bad << 1) | (wc > 3u ? 1u : 0u)) & kmask;
        alt_gap = ((alt_gap << 1) | (hc == 4u ? 1u : 0u)) & kmask;
        alt_bad = ((alt_bad << 1) | (hc == 5u ? 1u : 0u)) & kmask;
        // the window that ends at column e = e0 + i - 16 starts at ndx = e + 1 - k; it counts when ndx + k < columns
        if (i < 16u || e0 + (i - 16u) + 1u >= L || ref_bad || alt_bad) continue;
        uint32_t alt = alt3;
        if (alt_gap) {  // N and '-' leave the query k-mer, N fills it up again; nothing left: no window
          uint32_t m = 0;
          alt = 0;
          for (uint32_t f = 0; f < k; f++) {
            const uint32_t c = (alt3 >> (3u * f)) & 7u;
            if (c < 4u) alt |= c << (3u * m++);
          }
          if (m == 0u) continue;
          for (; m < k; m++) alt |= 4u << (3u * m);
        }
        const uint32_t same = alt == ref3 ? 1u : 0u;
        if (dense_lds) atomicAdd(&l_dense[ref2], 1u + same);
        else atomicAdd(T.dense + ref2, (unsigned long long)(1u + same));
        if (!same) fit_pair_add(T, (uint64_t)ref3 << 32 | alt);
      }
    }
  }
}
#endif  // FSAM_ROUTINES_ONLY

}  // namespace simmr
