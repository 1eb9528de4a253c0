// vcfeval_kernels.hip — a variant caller's VCF scored against the strain's sites (gfx950): two VCF texts in HBM to integer tables
// (include/simmr_hip.h states every rule: the record, what is malformed, the key, the entry, the QUAL row, the called alleles, the
// calls of an allele, the verdict, the order of the steps).  Included by vcfeval.hip alone, a translation unit of its own.  The
// reader's routines are taken, not restated: the line index and the scans of fit_sam_kernels.hip / sam_kernels.hip, the name row
// and the 16-way group search of mapeval_kernels.hip, through MEV_ROUTINES_ONLY (which brings FSAM_ROUTINES_ONLY with it).
//
// Six kernels; a work item past the line index is a LINE shared by VCE_LANES = 16 lanes (one DPP row).
//   k_vce_index    fsam_index_tiles: launched to count a tile's line starts and, after the scan, to write them.
//   k_vce_scan     ONE workgroup: sam_scan_chunks over the tile counts; the entry behind the last tile is the number of lines.
//   k_vce_truth    a truth line per group: the fields from tab ballots, POS, the two bases, the name row, the AD= item of INFO
//                  found by a ballot over item starts; an entry (key, ref class << 2 | alt class, ad_alt) is appended through an
//                  atomic cursor — the order is arbitrary and nothing depends on it, the sort that follows being over unique
//                  keys.  The largest key goes to a word by atomicMax: the sort's width.
//   k_vce_gather   behind samsort_sort_pairs: the entry columns into key order, and the neighbour check for equal keys.
//   k_vce_record   a candidate line per group: the same fields, the QUAL row from the digits, FILTER, the GT of the first sample,
//                  the ALT list; every called allele's calls, each looked up in the sorted keys by mev_lower_bound (a lane a
//                  pivot, a ballot a round); the verdict; the counts and by_qual privatised in LDS (one LDS atomic a group, added
//                  to HBM when the workgroup ends), best by atomicMax and hits by atomicAdd.
//   k_vce_reduce   the per-entry counts (found, wrong, missed, multiple) and by_ad over best[] / hits[] / ad[], privatised in LDS.
// Convergence.  Everything a group decides is decided from values all its 16 lanes hold alike (field places from ballots, bytes
// every lane reads at the same address), so the lanes of a group take every branch and loop trip together: the ballots of
// mev_lower_bound and mev_name_row and the row shuffles always see the whole group.  Groups of one wave may part; a ballot is
// read 16 bits at the group's place.
// Bounds.  Every load of text is below n_bytes and, past the field scan, inside the line's fields: a field is [a, b) with
// line <= a <= b <= the line's end <= n_bytes, and a byte at p is read only where a <= p < b (the AD= match asks p + 3 <= b
// first; REF byte j is read beside ALT byte j only where both fields have the length L > j).  An entry is stored below the capacity
// the adds' byte counts gave; best[] and hits[] are indexed by a search result below n_entries whose key was compared; by_qual is
// indexed by a row that is at most 255, by_ad by a bit length that is at most 32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#define MEV_ROUTINES_ONLY
#include "mapeval_kernels.hip"  // mev_name_row, mev_lower_bound, MevNames, MevText; through it the reader's routines and the scans

namespace simmr {

#define VCE_LANES 16u
#define VCE_WG 256u
#define VCE_WG_RECS 16u      /* lines per workgroup and batch */
#define VCE_MIN_LINE 15u     /* the shortest record: 8 one-byte fields and 7 tabs */
#define VCE_MAX_POS (1ull << 40)
#define VCE_POS_BITS 40u
#define VCE_MAX_MNP 64u      /* the longest allele whose bases are compared one by one */
#define VCE_QUAL_ROWS 256u
#define VCE_AD_ROWS 33u      /* by_ad: the bit length of ad_alt, 0 .. 32 */
#define VCE_ERR_TRUTH 1u     /* a malformed truth record */
#define VCE_ERR_CAND 2u      /* a malformed candidate record */
#define VCE_ERR_DUP 4u       /* two truth entries with one key */
static_assert(VCE_LANES == MEV_LANES && VCE_LANES == FSAM_LANES, "the group of the search and of the ballot is the reader's");

enum { VC_T_LINES = 0, VC_T_HEADER, VC_T_ENTRIES, VC_LINES, VC_HEADER, VC_RECORDS, VC_FILTERED, VC_QUAL_MISSING, VC_REF_CALL, VC_SYMBOLIC, VC_INDEL,
       VC_LONG_ALLELE, VC_REF_CALL_ALLELE, VC_CALLS, VC_UNKNOWN_CONTIG, VC_NO_SITE, VC_REF_MISMATCH, VC_WRONG_ALLELE, VC_CORRECT, VC_WRONG,
       VC_SITES_FOUND, VC_SITES_WRONG, VC_SITES_MISSED, VC_SITES_MULTIPLE, VC_COUNT };
static_assert(sizeof(simmr_vcfeval_counts) == VC_COUNT * 8u, "the counts in the header's order");
static_assert(SIMMR_VCFEVAL_AD_ROWS == VCE_AD_ROWS, "by_ad's rows");
#define VCE_REC_COUNTS ((uint32_t)(VC_SITES_FOUND - VC_LINES))  /* the counts k_vce_record makes */

struct VceEntries {  // the truth entries: appended in any order, or gathered into key order
  uint64_t* key;
  uint32_t* alleles;  // ref class << 2 | alt class
  uint32_t* ad;       // ad_alt
};

struct VceLine {  // what both sides read of a record (group-uniform); a field is text[a, a_end)
  uint64_t pos;   // POS as written (1-based)
  uint32_t chrom_end, ref, ref_end, alt, alt_end, qual, qual_end, filt, filt_end, info, info_end;
  uint32_t fmt, fmt_end, smp, smp_end;  // FSAM_NONE: the record has no such column
  uint32_t bad;
};

// A byte folded for the comparisons: (c - 'A') with the case bit cleared, so A C G N T (either case) are 0 2 6 13 19 and no other
// byte is below 32 with one of those values.  (Bytes are compared as small differences from 'A': the constants stay inline.)
SIMMR_DEV uint32_t vce_fold(uint32_t c) { return (c - 'A') & ~0x20u; }
SIMMR_DEV bool vce_base5(uint32_t c) {  // ACGTNacgtn
  const uint32_t f = vce_fold(c);
  return f < 32u && ((0x82045u >> f) & 1u) != 0u;
}
// the class of a folded byte: A C G T are 0 1 2 3, every other byte 4
SIMMR_DEV uint32_t vce_class(uint32_t f) { return f == 0u ? 0u : f == 2u ? 1u : f == 6u ? 2u : f == 19u ? 3u : 4u; }

// The fields of the line at `line`.  bad: fewer than 8 fields; a POS that is no number of 1 to 18 digits, is 0 or above 2^40; an
// empty REF or one with a byte outside ACGTNacgtn; an empty ALT.  (QUAL's syntax is vce_qual_row's.)
SIMMR_DEV VceLine vce_read_line(const uint8_t* __restrict__ t, uint32_t n, uint32_t line, uint32_t sub) {
  VceLine L{};
  uint32_t tb[10];
#pragma unroll
  for (uint32_t j = 0; j < 10u; j++) tb[j] = FSAM_NONE;
  uint32_t n_tab = 0, end = n;
  for (uint32_t p0 = line;; p0 += VCE_LANES) {  // (n is at most SIMMR_FIT_SAM_MAX_BYTES: p0 + 16 does not wrap)
    const uint32_t p = p0 + sub;
    const uint32_t c = p < n ? t[p] : '\n';
    uint32_t m_tab = fsam_ballot(c == '\t');
    const uint32_t m_nl = fsam_ballot(c == '\n');
    if (m_nl) {
      const uint32_t first = (uint32_t)__builtin_ctz(m_nl);
      m_tab &= (1u << first) - 1u;
      end = p0 + first;
    }
    for (; m_tab; m_tab &= m_tab - 1u) {
      const uint32_t at = p0 + (uint32_t)__builtin_ctz(m_tab);
#pragma unroll
      for (uint32_t j = 0; j < 10u; j++)
        if (n_tab == j) tb[j] = at;
      n_tab++;
    }
    if (m_nl) break;
  }
  if (n_tab < 7u) { L.bad = 1u; return L; }
  L.chrom_end = tb[0];
  L.ref = tb[2] + 1u;   L.ref_end = tb[3];
  L.alt = tb[3] + 1u;   L.alt_end = tb[4];
  L.qual = tb[4] + 1u;  L.qual_end = tb[5];
  L.filt = tb[5] + 1u;  L.filt_end = tb[6];
  L.info = tb[6] + 1u;  L.info_end = n_tab > 7u ? tb[7] : end;
  L.fmt = n_tab > 7u ? tb[7] + 1u : FSAM_NONE;
  L.fmt_end = n_tab > 8u ? tb[8] : end;
  L.smp = n_tab > 8u ? tb[8] + 1u : FSAM_NONE;
  L.smp_end = n_tab > 9u ? tb[9] : end;
  bool ok = fsam_field_number(t, tb[0] + 1u, tb[1], false, &L.pos) && L.pos >= 1u && L.pos <= VCE_MAX_POS;
  ok = ok && L.ref_end > L.ref && L.alt_end > L.alt;
  uint32_t other = 0;
  if (ok)
    for (uint32_t p0 = L.ref; p0 < L.ref_end; p0 += VCE_LANES) {  // (uniform over the row)
      const uint32_t p = p0 + sub;
      if (p < L.ref_end && !vce_base5(t[p])) other = 1u;
    }
  other = fsam_row_or(other);
  L.bad = ok && !other ? 0u : 1u;
  return L;
}

// whether FILTER text[a, b) is "." or "PASS"
SIMMR_DEV bool vce_passes(const uint8_t* __restrict__ t, uint32_t a, uint32_t b) {
  if (b - a == 1u) return t[a] == '.';
  return b - a == 4u && t[a] - 'A' == 15u && t[a + 1u] - 'A' == 0u && t[a + 2u] - 'A' == 18u && t[a + 3u] - 'A' == 18u;  // PASS
}

// QUAL text[a, b): "." (row 0, *missing) or [0-9]+(\.[0-9]*)?([eE][+-]?[0-9]{1,3})? with at most 18 digits before the point;
// false: neither.  The row is min(255, floor(value)) from the digits alone: with ni digits before the point and the exponent e, the
// floor is the number the first ni + e digits spell (the digits before the point, then those behind it, then zeros; none: 0).
SIMMR_DEV bool vce_qual_row(const uint8_t* __restrict__ t, uint32_t a, uint32_t b, uint32_t* row, uint32_t* missing) {
  *row = 0u;
  *missing = 0u;
  if (b - a == 1u && t[a] == '.') { *missing = 1u; return true; }
  uint32_t p = a;
  while (p < b && fsam_digit(t[p])) p++;
  const uint32_t ni = p - a;
  if (ni == 0u || ni > 18u) return false;
  uint32_t f = p, nf = 0u;
  if (p < b && t[p] == '.') {
    f = ++p;
    while (p < b && fsam_digit(t[p])) p++;
    nf = p - f;
  }
  int32_t e = 0;
  if (p < b && vce_fold(t[p]) == 4u) {  // e or E
    p++;
    bool neg = false;
    if (p < b && (t[p] == '+' || t[p] == '-')) { neg = t[p] == '-'; p++; }
    const uint32_t e0 = p;
    int32_t ev = 0;
    while (p < b && p - e0 < 3u && fsam_digit(t[p])) { ev = ev * 10 + (int32_t)(t[p] - '0'); p++; }
    if (p == e0) return false;
    e = neg ? -ev : ev;
  }
  if (p != b) return false;
  const int32_t take = (int32_t)ni + e;  // at most 18 + 999
  uint32_t v = 0u;
  for (int32_t k = 0; k < take && v < 256u; k++) {  // (past 255 the row is 255 whatever follows)
    const uint32_t u = (uint32_t)k;
    if (u >= ni + nf && v == 0u) break;              // zeros behind a zero
    const uint32_t d = u < ni ? (uint32_t)t[a + u] - '0' : u - ni < nf ? (uint32_t)t[f + (u - ni)] - '0' : 0u;
    v = v * 10u + d;
  }
  *row = v < 255u ? v : 255u;
  return true;
}

// The GT text[g, g_end) of the first sample: numbers of 1 to 18 digits or ".", separated by '/' or '|'.  false: an item that is
// neither.  *largest: the largest number (0: none).
SIMMR_DEV bool vce_gt_largest(const uint8_t* __restrict__ t, uint32_t g, uint32_t g_end, uint64_t* largest) {
  uint64_t big = 0;
  for (uint32_t p = g;;) {
    uint32_t q = p;
    while (q < g_end && t[q] != '/' && t[q] - 'A' != 59u) q++;  // / or |
    if (!(q - p == 1u && t[p] == '.')) {
      uint64_t v;
      if (!fsam_field_number(t, p, q, false, &v)) return false;
      big = v > big ? v : big;
    }
    if (q >= g_end) break;
    p = q + 1u;
  }
  *largest = big;
  return true;
}
// whether the (checked) GT names the index k
SIMMR_DEV bool vce_gt_has(const uint8_t* __restrict__ t, uint32_t g, uint32_t g_end, uint64_t k) {
  for (uint32_t p = g;;) {
    uint32_t q = p;
    while (q < g_end && t[q] != '/' && t[q] - 'A' != 59u) q++;  // / or |
    uint64_t v;
    if (fsam_field_number(t, p, q, false, &v) && v == k) return true;
    if (q >= g_end) return false;
    p = q + 1u;
  }
}

// ---- the line index and the scan ------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_vce_index(const uint8_t* __restrict__ text, uint64_t n_bytes, uint64_t n_tiles, uint64_t* __restrict__ tile_sum,
            const uint64_t* __restrict__ tile_prefix, uint32_t* __restrict__ starts, uint64_t start_capacity) {
  __shared__ uint32_t lds[FSAM_WG];
  fsam_index_tiles(text, n_bytes, n_tiles, tile_sum, tile_prefix, starts, start_capacity, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_vce_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

// ---- the truth ------------------------------------------------------------------------------------------------------------------
// cursor[0]: the entries so far (never reset between adds), cursor[1]: the largest key
extern "C" __global__ void __launch_bounds__(VCE_WG)
k_vce_truth(MevText W, MevNames N, VceEntries E, uint64_t capacity, unsigned long long* __restrict__ cursor, unsigned long long* __restrict__ counts,
            uint32_t* __restrict__ err) {
  __shared__ uint32_t l_cnt[3];  // lines, header lines, entries
  const uint8_t* __restrict__ t = W.text;
  const uint32_t tid = threadIdx.x, sub = tid & (VCE_LANES - 1u), row = tid / VCE_LANES;
  if (tid < 3u) l_cnt[tid] = 0u;
  __syncthreads();
  const uint64_t n_lines = *W.n_lines;
  const uint32_t n = (uint32_t)W.n_bytes;  // (at most SIMMR_FIT_SAM_MAX_BYTES)
  const uint64_t n_batches = (n_lines + VCE_WG_RECS - 1u) / VCE_WG_RECS;
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t li = batch * VCE_WG_RECS + row;
    if (li >= n_lines) continue;  // (uniform over the row)
    const uint32_t line = W.starts[li];
    if (line >= n) continue;      // (never: the index holds places of the text)
    if (sub == 0u) atomicAdd(&l_cnt[0], 1u);
    if (t[line] == '#') { if (sub == 0u) atomicAdd(&l_cnt[1], 1u); continue; }
    const VceLine L = vce_read_line(t, n, line, sub);
    uint32_t row_q = 0u, missing = 0u;
    bool ok = !L.bad && vce_qual_row(t, L.qual, L.qual_end, &row_q, &missing);
    // one base each of ACGT, and two different ones
    uint32_t rc = 4u, ac = 4u;
    if (ok) {
      rc = L.ref_end - L.ref == 1u ? vce_class(vce_fold(t[L.ref])) : 4u;
      ac = L.alt_end - L.alt == 1u ? vce_class(vce_fold(t[L.alt])) : 4u;
      ok = rc < 4u && ac < 4u && rc != ac;
    }
    uint32_t name = MEV_NO_ROW;
    if (ok) {
      name = mev_name_row(N, t, line, L.chrom_end, sub);
      ok = name != MEV_NO_ROW;
    }
    // the first item of INFO that starts with "AD=": a lane a byte, the item starts from a ballot
    uint64_t ad = 0;
    if (ok) {
      uint32_t at = FSAM_NONE;
      for (uint32_t p0 = L.info; p0 < L.info_end && at == FSAM_NONE; p0 += VCE_LANES) {  // (uniform over the row)
        const uint32_t p = p0 + sub;
        const bool hit = p + 3u <= L.info_end && (p == L.info || t[p - 1u] == ';') && t[p] - 'A' == 0u && t[p + 1u] - 'A' == 3u && t[p + 2u] == '=';  // AD=
        const uint32_t m = fsam_ballot(hit);
        if (m) at = p0 + (uint32_t)__builtin_ctz(m) + 3u;
      }
      if (at != FSAM_NONE) {  // <1..10 digits>,<1..10 digits> and the item's end; the second below 2^32
        uint32_t comma = at, item_end;
        while (comma < L.info_end && t[comma] != ',' && t[comma] != ';') comma++;
        item_end = comma < L.info_end && t[comma] == ',' ? comma + 1u : comma;
        while (item_end < L.info_end && t[item_end] != ';') item_end++;
        uint64_t ad_ref;
        ok = comma < L.info_end && t[comma] == ',' && comma - at <= 10u && item_end - (comma + 1u) <= 10u &&
             fsam_field_number(t, at, comma, false, &ad_ref) && fsam_field_number(t, comma + 1u, item_end, false, &ad) && ad <= 0xffffffffull;
      }
    }
    if (!ok) { if (sub == 0u) atomicOr(err, VCE_ERR_TRUTH); continue; }
    if (sub == 0u) {
      atomicAdd(&l_cnt[2], 1u);
      const uint64_t key = (uint64_t)name << VCE_POS_BITS | (L.pos - 1u);
      const unsigned long long slot = atomicAdd(cursor, 1ull);
      atomicMax(cursor + 1, (unsigned long long)key);
      if (slot < capacity) {  // (always: an add's lines are fewer than its bytes / VCE_MIN_LINE + 1)
        E.key[slot] = key;
        E.alleles[slot] = rc << 2 | ac;
        E.ad[slot] = (uint32_t)ad;
      }
    }
  }
  __syncthreads();
  if (tid < 3u && l_cnt[tid]) atomicAdd(counts + VC_T_LINES + tid, (unsigned long long)l_cnt[tid]);
}

// the entry columns into key order (perm == nullptr: a key without bits, the order is the identity), and equal neighbours
extern "C" __global__ void __launch_bounds__(256)
k_vce_gather(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ perm, VceEntries U, VceEntries S, uint64_t n, uint32_t* __restrict__ err) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t from = perm ? perm[i] : i;
    if (from >= n) continue;  // (never: the sort writes a permutation)
    S.alleles[i] = U.alleles[from];
    S.ad[i] = U.ad[from];
    if (i + 1u < n && skey[i] == skey[i + 1u]) atomicOr(err, VCE_ERR_DUP);
  }
}

// ---- the candidate records --------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(VCE_WG)
k_vce_record(MevText W, MevNames N, const uint64_t* __restrict__ skey, const uint32_t* __restrict__ alleles, uint64_t n_entries, uint32_t use_filtered,
             unsigned long long* __restrict__ counts, uint32_t* __restrict__ best, uint32_t* __restrict__ hits, uint32_t* __restrict__ err) {
  __shared__ uint32_t l_cnt[VCE_REC_COUNTS];
  __shared__ uint32_t l_qual[2u * VCE_QUAL_ROWS];
  const uint8_t* __restrict__ t = W.text;
  const uint32_t tid = threadIdx.x, sub = tid & (VCE_LANES - 1u), row = tid / VCE_LANES;
  if (tid < VCE_REC_COUNTS) l_cnt[tid] = 0u;
  for (uint32_t i = tid; i < 2u * VCE_QUAL_ROWS; i += VCE_WG) l_qual[i] = 0u;
  __syncthreads();
#define VCE_COUNT(which) do { if (sub == 0u) atomicAdd(&l_cnt[(which) - VC_LINES], 1u); } while (0)
  const uint32_t n = (uint32_t)W.n_bytes;        // (at most SIMMR_FIT_SAM_MAX_BYTES)
  const uint32_t n_lines = (uint32_t)*W.n_lines;  // (a line start per two bytes at the most: below 2^31)
  const uint32_t n_batches = (n_lines + VCE_WG_RECS - 1u) / VCE_WG_RECS;
  for (uint32_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint32_t li = batch * VCE_WG_RECS + row;
    if (li >= n_lines) continue;  // (uniform over the row)
    const uint32_t line = W.starts[li];
    if (line >= n) continue;      // (never)
    VCE_COUNT(VC_LINES);
    if (t[line] == '#') { VCE_COUNT(VC_HEADER); continue; }
    const VceLine L = vce_read_line(t, n, line, sub);
    uint32_t qrow = 0u, missing = 0u;
    if (L.bad || !vce_qual_row(t, L.qual, L.qual_end, &qrow, &missing)) { if (sub == 0u) atomicOr(err, VCE_ERR_CAND); continue; }
    VCE_COUNT(VC_RECORDS);
    // 1. FILTER
    if (!use_filtered && !vce_passes(t, L.filt, L.filt_end)) { VCE_COUNT(VC_FILTERED); continue; }
    // 2. the QUAL row
    if (missing) VCE_COUNT(VC_QUAL_MISSING);
    // 3. the called alleles: those the GT of the first sample names, or all of them
    uint32_t commas = 0u;
    for (uint32_t p0 = L.alt; p0 < L.alt_end; p0 += VCE_LANES) {  // (uniform over the row)
      const uint32_t p = p0 + sub;
      commas += (uint32_t)__popc(fsam_ballot(p < L.alt_end && t[p] == ','));
    }
    const uint32_t n_alt = commas + 1u;
    const bool has_gt = L.smp != FSAM_NONE && L.fmt_end - L.fmt >= 2u && t[L.fmt] - 'A' == 6u && t[L.fmt + 1u] - 'A' == 19u &&  // GT
                        (L.fmt_end - L.fmt == 2u || t[L.fmt + 2u] == ':');
    uint32_t gt = 0u, gt_end = 0u;
    if (has_gt) {
      gt = L.smp;
      gt_end = gt;
      while (gt_end < L.smp_end && t[gt_end] != ':') gt_end++;
      uint64_t largest;
      if (!vce_gt_largest(t, gt, gt_end, &largest) || largest > n_alt) {  // (the read answers SIMMR_EINVAL: no count is seen)
        if (sub == 0u) atomicOr(err, VCE_ERR_CAND);
        continue;
      }
      if (largest == 0u) { VCE_COUNT(VC_REF_CALL); continue; }
    }
    const uint32_t name = mev_name_row(N, t, line, L.chrom_end, sub);
    const uint32_t ref_len = L.ref_end - L.ref;
    // 4. each called allele, in ALT order
    uint32_t a0 = L.alt;
    for (uint32_t k = 1u;; k++) {  // (uniform over the row)
      uint32_t a1 = a0, bracket = 0u, other = 0u;
      for (; a1 < L.alt_end && t[a1] != ','; a1++) {
        const uint32_t c = t[a1];
        bracket |= c - 'A' == 26u || c - 'A' == 28u ? 1u : 0u;  // [ or ]
        other |= vce_base5(c) ? 0u : 1u;
      }
      const uint32_t len = a1 - a0;
      // the allele's kind, without a branch: symbolic, indel, long, or a substitution of len bases
      const uint32_t first = t[a0 < L.alt_end ? a0 : L.alt];  // (an empty allele is an indel whatever this byte is)
      const uint32_t kind = (len == 1u && first == '*') || (len >= 1u && first == '<') || bracket ? VC_SYMBOLIC
                            : len != ref_len || other ? VC_INDEL : len > VCE_MAX_MNP ? VC_LONG_ALLELE : VC_CALLS;
      const bool called = !has_gt || vce_gt_has(t, gt, gt_end, k);
      if (called && kind != VC_CALLS) VCE_COUNT(kind);
      uint32_t differs = 0u;
      for (uint32_t j = 0u; called && kind == VC_CALLS && j < len; j++) {
        const uint32_t r = vce_fold(t[L.ref + j]), c = vce_fold(t[a0 + j]);  // (both of ACGTNacgtn here: equal iff the same letter)
        const uint32_t rc = vce_class(r), ac = vce_class(c);
        differs |= r != c ? 1u : 0u;
        if (r == c || rc > 3u || ac > 3u) continue;
        // 5. a call at POS + j.  The search runs over no key where there is nothing to find: an unknown CHROM, or a position
        // of 2^40 or more, where no entry lies (the key has 40 bits of position).
        const uint64_t pos = L.pos - 1u + j;
        const bool look = name != MEV_NO_ROW && pos < VCE_MAX_POS;
        const uint64_t key = (uint64_t)name << VCE_POS_BITS | pos;
        const uint64_t lb = mev_lower_bound(skey, look ? n_entries : 0ull, key, sub);
        const uint64_t at = lb < n_entries ? lb : 0ull;  // (skey[0] and alleles[0] exist even without entries)
        const bool found = look && lb < n_entries && skey[at] == key;
        const uint32_t al = alleles[at];
        const uint32_t which = name == MEV_NO_ROW ? VC_UNKNOWN_CONTIG : !found ? VC_NO_SITE : (al >> 2) != rc ? VC_REF_MISMATCH
                               : (al & 3u) != ac ? VC_WRONG_ALLELE : VC_CORRECT;
        if (sub == 0u) {
          atomicAdd(&l_cnt[VC_CALLS - VC_LINES], 1u);
          atomicAdd(&l_cnt[which - VC_LINES], 1u);
          if (which != VC_CORRECT) atomicAdd(&l_cnt[VC_WRONG - VC_LINES], 1u);
          atomicAdd(&l_qual[2u * qrow + (which == VC_CORRECT ? 0u : 1u)], 1u);
          if (found) {
            atomicMax(best + at, (which == VC_CORRECT ? 3u : 2u) << 8 | qrow);
            atomicAdd(hits + at, 1u);
          }
        }
      }
      if (called && kind == VC_CALLS && !differs) VCE_COUNT(VC_REF_CALL_ALLELE);
      if (a1 >= L.alt_end) break;
      a0 = a1 + 1u;
    }
  }
#undef VCE_COUNT
  __syncthreads();
  if (tid < VCE_REC_COUNTS && l_cnt[tid]) atomicAdd(counts + VC_LINES + tid, (unsigned long long)l_cnt[tid]);
  for (uint32_t i = tid; i < 2u * VCE_QUAL_ROWS; i += VCE_WG) {
    const uint32_t v = l_qual[i];
    if (v) atomicAdd(counts + VC_COUNT + i, (unsigned long long)v);  // by_qual stands behind the counts
  }
}

// ---- the entries by their best call -----------------------------------------------------------------------------------------------
// l_sum: found, wrong, missed, multiple, then by_ad's 33 x 2 words (the entries are fewer than 2^31: no word overflows)
extern "C" __global__ void __launch_bounds__(256)
k_vce_reduce(const uint32_t* __restrict__ best, const uint32_t* __restrict__ hits, const uint32_t* __restrict__ ad, uint64_t n,
             unsigned long long* __restrict__ counts, unsigned long long* __restrict__ by_ad) {
  __shared__ uint32_t l_sum[4u + 2u * VCE_AD_ROWS];
  for (uint32_t i = threadIdx.x; i < 4u + 2u * VCE_AD_ROWS; i += 256u) l_sum[i] = 0u;
  __syncthreads();
  for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += (uint64_t)gridDim.x * 256u) {  // (uniform over the workgroup)
    const uint64_t i = i0 + threadIdx.x;
    uint32_t c[4] = {0u, 0u, 0u, 0u};  // found, wrong, missed, multiple
    if (i < n) {
      const uint32_t h = hits[i], cls = best[i] >> 8;
      c[0] = cls == 3u ? 1u : 0u;
      c[1] = cls == 2u ? 1u : 0u;
      c[2] = h == 0u ? 1u : 0u;
      c[3] = h > 1u ? 1u : 0u;
      const uint32_t v = ad[i];
      const uint32_t bits = v ? 32u - (uint32_t)__builtin_clz(v) : 0u;  // at most 32: below VCE_AD_ROWS
      atomicAdd(&l_sum[4u + 2u * bits + (cls == 3u ? 0u : 1u)], 1u);
    }
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
      const uint32_t m = (uint32_t)__popcll(__ballot(c[j] != 0u));
      if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&l_sum[j], m);
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < 4u + 2u * VCE_AD_ROWS; k += 256u) {
    const uint32_t v = l_sum[k];
    if (v) atomicAdd(k < 4u ? counts + VC_SITES_FOUND + k : by_ad + (k - 4u), (unsigned long long)v);
  }
}

}  // namespace simmr
