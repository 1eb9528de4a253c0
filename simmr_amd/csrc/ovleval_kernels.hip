// ovleval_kernels.hip — an overlapper's PAF scored against the true overlaps (gfx950): two PAF texts in HBM to integer tables
// (include/simmr_hip.h states every rule: the record, the name and its key, the entry, the verdict, the order of the steps).
// Included by ovleval.hip alone, a translation unit of its own.  The reader's routines are taken, not restated: the line index
// and the scans of fit_sam_kernels.hip / sam_kernels.hip and the 16-way group search of mapeval_kernels.hip, through
// MEV_ROUTINES_ONLY (which brings FSAM_ROUTINES_ONLY with it).
//
// Eight kernels; a work item past the line index is a LINE shared by OVE_LANES = 16 lanes (one DPP row).
//   k_ove_index    fsam_index_tiles: launched to count a tile's line starts and, after the scan, to write them.
//   k_ove_scan     ONE workgroup: sam_scan_chunks over tile counts — the line index's, and the head counts of k_ove_heads.
//   k_ove_truth    a truth line per group: the twelve fields, the two names as keys; an entry (lo key, hi key, strand, the two
//                  intervals, ov) is appended through an atomic cursor — the order is arbitrary and nothing depends on it, the
//                  sort that follows being over unique keys.  The largest key goes to a word by atomicMax: the first sort's width.
//   k_ove_heads    behind the sort of the 2 n keys: a key that differs from the one before it is a head.  Launched to count a
//                  tile's heads and, after the scan, to write the distinct keys and every key's dense rank at the place it
//                  came from (the sort's permutation).
//   k_ove_keys     an entry's sort key, rank_lo << 31 | rank_hi, from the two ranks.
//   k_ove_gather   behind the second sort: the entry columns into key order, and the neighbour check for equal pairs.
//   k_ove_record   a candidate line per group: the same reading; its two keys looked up in the distinct keys and the pair in
//                  the entry keys by mev_lower_bound (a lane a pivot, a ballot a round); the verdict; the counts privatised
//                  in LDS (one LDS atomic a group, added to HBM when the workgroup ends), best by atomicMax, hits by atomicAdd.
//   k_ove_reduce   the per-entry counts (found, wrong, missed, multiple) and by_len over best[] / hits[] / ov[], privatised in LDS.
// Bounds.  Every load of text is below n_bytes and, past the field scan, inside the line's fields; an entry is stored below the
// capacity the adds' byte counts gave; a rank is below the number of heads, which is at most the 2 n keys the columns hold;
// best[] and hits[] are indexed by a search result below n_entries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#define MEV_ROUTINES_ONLY
#include "mapeval_kernels.hip"  // mev_lower_bound, MevText; through it the reader's routines of fit_sam_kernels.hip and the scans

namespace simmr {

#define OVE_LANES 16u
#define OVE_WG 256u
#define OVE_WG_RECS 16u      /* lines per workgroup and batch */
#define OVE_MIN_LINE 23u     /* the shortest record: 12 one-byte fields and 11 tabs */
#define OVE_HEAD_TILE 256u   /* sorted keys per workgroup and round of k_ove_heads: a key a thread */
#define OVE_MAX_LEN (1ull << 40)
#define OVE_RANK_BITS 31u
#define OVE_LEN_ROWS 41u     /* by_len: the bit length of ov, 0 .. 40 */
#define OVE_ERR_TRUTH 1u     /* a malformed truth record */
#define OVE_ERR_CAND 2u      /* a malformed candidate record */
#define OVE_ERR_DUP 4u       /* two truth entries with one pair */
#define OVE_STRAND (1ull << 63)
static_assert(OVE_LANES == MEV_LANES && OVE_LANES == FSAM_LANES, "the group of the search and of the ballot is the reader's");

enum { OC_T_LINES = 0, OC_T_ENTRIES, OC_T_READS, OC_LINES, OC_RECORDS, OC_UNKNOWN_READ, OC_SELF, OC_NO_PAIR, OC_WRONG_STRAND, OC_WRONG_INTERVAL,
       OC_CORRECT, OC_WRONG, OC_PAIRS_FOUND, OC_PAIRS_WRONG, OC_PAIRS_MISSED, OC_PAIRS_MULTIPLE, OC_COUNT };
static_assert(sizeof(simmr_ovleval_counts) == OC_COUNT * 8u, "the counts in the header's order");
static_assert(SIMMR_OVLEVAL_LEN_ROWS == OVE_LEN_ROWS, "by_len's rows");

struct OveEntries {  // the truth entries: appended in any order (keys: lo and hi interleaved), or gathered into pair order (ka, kb)
  uint64_t* keys;
  uint64_t* ka;
  uint64_t* kb;
  uint64_t* lo_s;    // the start of the lower-keyed read's interval | OVE_STRAND where the strands differ
  uint64_t* lo_e;
  uint64_t* hi_s;
  uint64_t* hi_e;
  uint64_t* ov;      // query end - query start
};

struct OveLine {  // what both sides read of a record (group-uniform)
  uint64_t ql, qs, qe, tl, ts, te;
  uint32_t qn_end, tn, tn_end;  // the query name is text[line, qn_end), the target name text[tn, tn_end)
  uint32_t minus, bad;
};

// The fields of the line at `line`.  bad: fewer than 12 fields; a field 2, 3, 4 or 7 .. 12 that is no number of 1 to 18 digits; a
// field 5 that is neither "+" nor "-"; a side without start <= end <= length < 2^40.
SIMMR_DEV OveLine ove_read_line(const uint8_t* __restrict__ t, uint64_t n, uint32_t line, uint32_t sub) {
  OveLine L{};
  uint32_t tb[12];
#pragma unroll
  for (uint32_t j = 0; j < 12u; j++) tb[j] = FSAM_NONE;
  uint32_t n_tab = 0, end = (uint32_t)n;
  for (uint64_t p0 = line;; p0 += OVE_LANES) {
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
      for (uint32_t j = 0; j < 12u; j++)
        if (n_tab == j) tb[j] = at;
      n_tab++;
    }
    if (m_nl) break;
  }
  if (n_tab < 11u) { L.bad = 1u; return L; }
  if (n_tab == 11u) tb[11] = end;  // (the twelfth field ends the line: no tags)
  uint64_t x;
  bool ok = fsam_field_number(t, tb[0] + 1u, tb[1], false, &L.ql) && fsam_field_number(t, tb[1] + 1u, tb[2], false, &L.qs) &&
            fsam_field_number(t, tb[2] + 1u, tb[3], false, &L.qe) && fsam_field_number(t, tb[5] + 1u, tb[6], false, &L.tl) &&
            fsam_field_number(t, tb[6] + 1u, tb[7], false, &L.ts) && fsam_field_number(t, tb[7] + 1u, tb[8], false, &L.te) &&
            fsam_field_number(t, tb[8] + 1u, tb[9], false, &x) && fsam_field_number(t, tb[9] + 1u, tb[10], false, &x) &&
            fsam_field_number(t, tb[10] + 1u, tb[11], false, &x);
  const uint32_t s = tb[4] - tb[3] == 2u ? (uint32_t)t[tb[3] + 1u] : 0u;
  ok = ok && (s == '+' || s == '-');
  ok = ok && L.qs <= L.qe && L.qe <= L.ql && L.ql < OVE_MAX_LEN && L.ts <= L.te && L.te <= L.tl && L.tl < OVE_MAX_LEN;
  L.minus = s == '-' ? 1u : 0u;
  L.qn_end = tb[0];
  L.tn = tb[4] + 1u;
  L.tn_end = tb[5];
  L.bad = ok ? 0u : 1u;
  return L;
}

// the key of the read name text[a, b): 1 to 18 digits, then nothing, "/1" or "/2"; false: not a read name
SIMMR_DEV bool ove_name_key(const uint8_t* __restrict__ t, uint32_t a, uint32_t b, uint64_t* key) {
  uint32_t mate = 0;
  if (b - a >= 3u && t[b - 2u] == '/' && (t[b - 1u] == '1' || t[b - 1u] == '2')) {
    mate = t[b - 1u] == '2' ? 1u : 0u;
    b -= 2u;
  }
  uint64_t id;
  if (!fsam_field_number(t, a, b, false, &id)) return false;
  *key = id << 1 | mate;
  return true;
}

// The kernels.  correval_kernels.hip (a translation unit of its own) includes this file with OVE_ROUTINES_ONLY defined and takes the
// routines above without them, as this file takes mapeval_kernels.hip's.
#ifndef OVE_ROUTINES_ONLY
// ---- the line index and the scan ------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_ove_index(const uint8_t* __restrict__ text, uint64_t n_bytes, uint64_t n_tiles, uint64_t* __restrict__ tile_sum,
            const uint64_t* __restrict__ tile_prefix, uint32_t* __restrict__ starts, uint64_t start_capacity) {
  __shared__ uint32_t lds[FSAM_WG];
  fsam_index_tiles(text, n_bytes, n_tiles, tile_sum, tile_prefix, starts, start_capacity, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_ove_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

// ---- the truth ------------------------------------------------------------------------------------------------------------------
// cursor[0]: the entries so far (never reset between adds), cursor[1]: the largest key
extern "C" __global__ void __launch_bounds__(OVE_WG)
k_ove_truth(MevText W, OveEntries E, uint64_t capacity, unsigned long long* __restrict__ cursor, unsigned long long* __restrict__ counts,
            uint32_t* __restrict__ err) {
  __shared__ uint32_t l_cnt[2];  // lines, entries
  const uint8_t* __restrict__ t = W.text;
  const uint32_t tid = threadIdx.x, sub = tid & (OVE_LANES - 1u), row = tid / OVE_LANES;
  if (tid < 2u) l_cnt[tid] = 0u;
  __syncthreads();
  const uint64_t n_lines = *W.n_lines, n = W.n_bytes;
  const uint64_t n_batches = (n_lines + OVE_WG_RECS - 1u) / OVE_WG_RECS;
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t li = batch * OVE_WG_RECS + row;
    if (li >= n_lines) continue;  // (uniform over the row)
    const uint32_t line = W.starts[li];
    if (line >= n) continue;      // (never: the index holds places of the text)
    if (sub == 0u) atomicAdd(&l_cnt[0], 1u);
    const OveLine L = ove_read_line(t, n, line, sub);
    uint64_t kq = 0, kt = 0;
    if (L.bad || !ove_name_key(t, line, L.qn_end, &kq) || !ove_name_key(t, L.tn, L.tn_end, &kt) || kq == kt) {
      if (sub == 0u) atomicOr(err, OVE_ERR_TRUTH);
      continue;
    }
    if (sub == 0u) {
      atomicAdd(&l_cnt[1], 1u);
      const bool q_lo = kq < kt;
      const unsigned long long slot = atomicAdd(cursor, 1ull);
      atomicMax(cursor + 1, (unsigned long long)(q_lo ? kt : kq));
      if (slot < capacity) {  // (always: an add's lines are fewer than its bytes / OVE_MIN_LINE + 1)
        E.keys[2u * slot] = q_lo ? kq : kt;
        E.keys[2u * slot + 1u] = q_lo ? kt : kq;
        E.lo_s[slot] = (q_lo ? L.qs : L.ts) | (L.minus ? OVE_STRAND : 0ull);
        E.lo_e[slot] = q_lo ? L.qe : L.te;
        E.hi_s[slot] = q_lo ? L.ts : L.qs;
        E.hi_e[slot] = q_lo ? L.te : L.qe;
        E.ov[slot] = L.qe - L.qs;
      }
    }
  }
  __syncthreads();
  if (tid < 2u && l_cnt[tid]) atomicAdd(counts + (tid ? OC_T_ENTRIES : OC_T_LINES), (unsigned long long)l_cnt[tid]);
}

// The heads of the sorted keys sk[0, n2).  uniq == nullptr: a tile's heads are counted into tile_sum.  Otherwise, behind the scan:
// the distinct keys into uniq[] and the rank of key i into rk[perm[i]] (perm == nullptr: the order is the identity).
extern "C" __global__ void __launch_bounds__(256)
k_ove_heads(const uint64_t* __restrict__ sk, const uint32_t* __restrict__ perm, uint64_t n2, uint64_t n_tiles, uint64_t* __restrict__ tile_sum,
            const uint64_t* __restrict__ tile_prefix, uint64_t* __restrict__ uniq, uint32_t* __restrict__ rk) {
  __shared__ uint32_t lds[256];
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // (uniform over the workgroup)
    const uint64_t i = tile * OVE_HEAD_TILE + threadIdx.x;
    const uint32_t head = i < n2 && (i == 0u || sk[i] != sk[i - 1u]) ? 1u : 0u;
    uint32_t total;
    const uint32_t ex = sam_wg_scan<uint32_t>(head, lds, &total);
    if (!uniq) {
      if (threadIdx.x == 0) tile_sum[tile] = total;
      continue;
    }
    if (i >= n2) continue;
    const uint64_t rank = tile_prefix[tile] + ex + head - 1u;  // (key 0 is a head: the sum is at least 1)
    if (rank >= n2) continue;                                  // (never: the heads are at most the keys)
    if (head) uniq[rank] = sk[i];
    const uint64_t from = perm ? perm[i] : i;
    if (from < n2) rk[from] = (uint32_t)rank;
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_ove_keys(const uint32_t* __restrict__ rk, uint64_t* __restrict__ ekey, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
    ekey[i] = (uint64_t)rk[2u * i] << OVE_RANK_BITS | rk[2u * i + 1u];
}

// the entry columns into pair order (perm == nullptr: the order is the identity), and equal neighbours
extern "C" __global__ void __launch_bounds__(256)
k_ove_gather(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ perm, OveEntries U, OveEntries S, uint64_t n, uint32_t* __restrict__ err) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t from = perm ? perm[i] : i;
    if (from >= n) continue;  // (never: the sort writes a permutation)
    S.ka[i] = U.keys[2u * from];
    S.kb[i] = U.keys[2u * from + 1u];
    S.lo_s[i] = U.lo_s[from];
    S.lo_e[i] = U.lo_e[from];
    S.hi_s[i] = U.hi_s[from];
    S.hi_e[i] = U.hi_e[from];
    S.ov[i] = U.ov[from];
    if (i + 1u < n && skey[i] == skey[i + 1u]) atomicOr(err, OVE_ERR_DUP);
  }
}

// ---- the candidate records --------------------------------------------------------------------------------------------------------
// whether [s, e) and the entry's [ts, te) share a base and at least min_pct percent of what they span together
SIMMR_DEV bool ove_interval_holds(uint64_t s, uint64_t e, uint64_t ts, uint64_t te, uint32_t min_pct) {
  const uint64_t a = s > ts ? s : ts, b = e < te ? e : te, ov = b > a ? b - a : 0u;
  const uint64_t un = (e > te ? e : te) - (s < ts ? s : ts);
  return ov >= 1u && 100u * ov >= (uint64_t)min_pct * un;
}

extern "C" __global__ void __launch_bounds__(OVE_WG)
k_ove_record(MevText W, const uint64_t* __restrict__ uniq, uint64_t n_reads, const uint64_t* __restrict__ skey, OveEntries S, uint64_t n_entries,
             uint32_t min_pct, unsigned long long* __restrict__ counts, uint32_t* __restrict__ best, uint32_t* __restrict__ hits,
             uint32_t* __restrict__ err) {
  __shared__ uint32_t l_cnt[OC_PAIRS_FOUND - OC_LINES];
  const uint8_t* __restrict__ t = W.text;
  const uint32_t tid = threadIdx.x, sub = tid & (OVE_LANES - 1u), row = tid / OVE_LANES;
  if (tid < (uint32_t)(OC_PAIRS_FOUND - OC_LINES)) l_cnt[tid] = 0u;
  __syncthreads();
#define OVE_COUNT(which) do { if (sub == 0u) atomicAdd(&l_cnt[(which) - OC_LINES], 1u); } while (0)
  const uint64_t n_lines = *W.n_lines, n = W.n_bytes;
  const uint64_t n_batches = (n_lines + OVE_WG_RECS - 1u) / OVE_WG_RECS;
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t li = batch * OVE_WG_RECS + row;
    if (li >= n_lines) continue;  // (uniform over the row)
    const uint32_t line = W.starts[li];
    if (line >= n) continue;      // (never)
    OVE_COUNT(OC_LINES);
    const OveLine L = ove_read_line(t, n, line, sub);
    if (L.bad) { if (sub == 0u) atomicOr(err, OVE_ERR_CAND); continue; }
    OVE_COUNT(OC_RECORDS);
    uint64_t kq = 0, kt = 0, rq = n_reads, rt = n_reads;
    bool known = ove_name_key(t, line, L.qn_end, &kq) && ove_name_key(t, L.tn, L.tn_end, &kt);
    if (known) {
      rq = mev_lower_bound(uniq, n_reads, kq, sub);
      known = rq < n_reads && uniq[rq] == kq;
    }
    if (known) {
      rt = mev_lower_bound(uniq, n_reads, kt, sub);
      known = rt < n_reads && uniq[rt] == kt;
    }
    if (!known) { OVE_COUNT(OC_UNKNOWN_READ); OVE_COUNT(OC_WRONG); continue; }
    if (kq == kt) { OVE_COUNT(OC_SELF); continue; }
    const bool q_lo = kq < kt;
    const uint64_t pair = (q_lo ? rq : rt) << OVE_RANK_BITS | (q_lo ? rt : rq);
    const uint64_t at = mev_lower_bound(skey, n_entries, pair, sub);
    if (at >= n_entries || skey[at] != pair) { OVE_COUNT(OC_NO_PAIR); OVE_COUNT(OC_WRONG); continue; }
    const uint64_t lo_s = S.lo_s[at];
    uint32_t cls = 2u;
    if ((lo_s >> 63) != L.minus) {
      OVE_COUNT(OC_WRONG_STRAND);
    } else if (!ove_interval_holds(q_lo ? L.qs : L.ts, q_lo ? L.qe : L.te, lo_s & ~OVE_STRAND, S.lo_e[at], min_pct) ||
               !ove_interval_holds(q_lo ? L.ts : L.qs, q_lo ? L.te : L.qe, S.hi_s[at], S.hi_e[at], min_pct)) {
      OVE_COUNT(OC_WRONG_INTERVAL);
    } else {
      cls = 3u;
    }
    OVE_COUNT(cls == 3u ? OC_CORRECT : OC_WRONG);
    if (sub == 0u) {
      atomicMax(best + at, cls);
      atomicAdd(hits + at, 1u);
    }
  }
#undef OVE_COUNT
  __syncthreads();
  if (tid < (uint32_t)(OC_PAIRS_FOUND - OC_LINES) && l_cnt[tid]) atomicAdd(counts + OC_LINES + tid, (unsigned long long)l_cnt[tid]);
}

// ---- the entries by their best record ---------------------------------------------------------------------------------------------
// l_sum: found, wrong, missed, multiple, then by_len's 41 x 2 words (the entries are fewer than 2^30: no word overflows)
extern "C" __global__ void __launch_bounds__(256)
k_ove_reduce(const uint32_t* __restrict__ best, const uint32_t* __restrict__ hits, const uint64_t* __restrict__ ov, uint64_t n,
             unsigned long long* __restrict__ counts, unsigned long long* __restrict__ by_len) {
  __shared__ uint32_t l_sum[4u + 2u * OVE_LEN_ROWS];
  for (uint32_t i = threadIdx.x; i < 4u + 2u * OVE_LEN_ROWS; i += 256u) l_sum[i] = 0u;
  __syncthreads();
  for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += (uint64_t)gridDim.x * 256u) {  // (uniform over the workgroup)
    const uint64_t i = i0 + threadIdx.x;
    uint32_t c[4] = {0u, 0u, 0u, 0u};  // found, wrong, missed, multiple
    if (i < n) {
      const uint32_t h = hits[i], cls = best[i];
      c[0] = cls == 3u ? 1u : 0u;
      c[1] = cls == 2u ? 1u : 0u;
      c[2] = h == 0u ? 1u : 0u;
      c[3] = h > 1u ? 1u : 0u;
      const uint64_t v = ov[i];
      const uint32_t bits = v ? 64u - (uint32_t)__builtin_clzll(v) : 0u;
      if (bits < OVE_LEN_ROWS) atomicAdd(&l_sum[4u + 2u * bits + (cls == 3u ? 0u : 1u)], 1u);  // (always: ov is below 2^40)
    }
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
      const uint32_t m = (uint32_t)__popcll(__ballot(c[j] != 0u));
      if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&l_sum[j], m);
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < 4u + 2u * OVE_LEN_ROWS; k += 256u) {
    const uint32_t v = l_sum[k];
    if (v) atomicAdd(k < 4u ? counts + OC_PAIRS_FOUND + k : by_len + (k - 4u), (unsigned long long)v);
  }
}
#endif  // OVE_ROUTINES_ONLY

}  // namespace simmr
