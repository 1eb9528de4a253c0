// mapeval_kernels.hip — an aligner's SAM scored against the true alignments (gfx950): two SAM texts in HBM to integer tables
// (include/simmr_hip.h states every rule: the key, the interval, the verdict, what is malformed, the order of the filters).
// Included by mapeval.hip, a translation unit of its own; and, with MEV_ROUTINES_ONLY defined, by ovleval_kernels.hip, which takes the
// group search and the text's structs without the six kernels.  The SAM reader is fit_sam_kernels.hip's, taken as routines
// (FSAM_ROUTINES_ONLY): the line index by tile counts and a chunked scan, a line per group of 16 lanes, the tabs from a ballot,
// the CIGAR summed bytewise with fsam_cigar_lane.
//
// Six kernels; a work item past the line index is a LINE shared by MEV_LANES = 16 lanes (one DPP row).
//   k_mev_index    fsam_index_tiles: launched to count a tile's line starts and, after the scan, to write them.
//   k_mev_scan     ONE workgroup: sam_scan_chunks over the tile counts; the entry behind the last tile is the number of lines.
//   k_mev_truth    a truth line per group: the fields, the numbers, the CIGAR sums, the name row; an entry (key, row | strand,
//                  interval) is appended through an atomic cursor — the order is arbitrary and nothing depends on it, the sort
//                  that follows being over unique keys.  The largest key goes to a word by atomicMax: the sort's width.
//   k_mev_gather   behind samsort_sort_pairs: the entry columns into key order, and the neighbour check for equal keys.
//   k_mev_record   an aligned line per group: the same reading, the filters in the header's order, the key looked up in the
//                  sorted keys by a 16-way search (a lane a pivot, a ballot a round: four bits a round), the verdict;
//                  by_mapq privatised in LDS (256 x 2 words, added to HBM when the workgroup ends), the counts one atomic per
//                  group, best by atomicMax and hits by atomicAdd.
//   k_mev_reduce   the per-entry counts (missing, multiple, the reads by their best class) over best[] / hits[].
// The name row of an RNAME: a binary search over the sorted names of the blob; a comparison reads 16 bytes of both names a round
// across the group and takes the first differing byte from a ballot.
// Bounds.  Every load of text is below n_bytes and, past the field scan, inside the line's fields; an entry is stored below the
// capacity the adds' byte counts gave; best[] and hits[] are indexed by a search result below n_entries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#define FSAM_ROUTINES_ONLY
#include "fit_sam_kernels.hip"  // the SAM reader's routines without its kernels (and, through it, the scans of sam_kernels.hip)

namespace simmr {

#define MEV_LANES 16u
#define MEV_WG 256u
#define MEV_WG_RECS 16u     /* lines per workgroup and batch */
#define MEV_MIN_LINE 21u    /* the shortest record: 11 one-byte fields and 10 tabs */
#define MEV_MAX_POS 0x7fffffffull
#define MEV_MAX_END (1ull << 40)
#define MEV_MAX_ID (1ull << 62)
#define MEV_ERR_TRUTH 1u    /* a malformed truth record */
#define MEV_ERR_ALIGNED 2u  /* a malformed aligned record */
#define MEV_ERR_DUP 4u      /* two truth entries with one key */
#define MEV_NO_ROW 0xffffffffu

enum { MC_T_LINES = 0, MC_T_HEADER, MC_T_ENTRIES, MC_T_SKIPPED, MC_LINES, MC_HEADER, MC_RECORDS, MC_SECONDARY, MC_CIGAR_OP, MC_UNKNOWN_READ,
       MC_UNKNOWN_REF, MC_UNMAPPED, MC_CORRECT, MC_WRONG, MC_MISSING, MC_MULTIPLE, MC_READS_CORRECT, MC_READS_WRONG, MC_READS_UNMAPPED, MC_COUNT };
static_assert(sizeof(simmr_mapeval_counts) == MC_COUNT * 8u, "the counts in the header's order");

struct MevNames {  // the reference names, sorted bytewise (a prefix before the longer name)
  const uint8_t* blob;
  const uint32_t* off;  // [n + 1]: name r is blob[off[r] .. off[r + 1])
  uint32_t n;
};

struct MevText {
  const uint8_t* text;
  uint64_t n_bytes;
  const uint64_t* n_lines;  // the scan's last entry
  const uint32_t* starts;   // [lines]
};

struct MevEntries {  // the truth entries: appended in any order, or gathered into key order
  uint64_t* key;
  uint32_t* meta;    // row | strand << 31
  uint64_t* lo;
  uint64_t* hi;
};

struct MevLine {  // what both sides read of a record (group-uniform)
  uint64_t flag, mapq, pos, id, span;  // span = M + D (M counts M, = and X)
  uint32_t rname, rname_end;
  uint32_t bad, other_op, id_ok, rname_star;
};

// name r of the table against text[a, b): < 0 the table's name is smaller, 0 equal, > 0 larger.  16 bytes of both a round.
SIMMR_DEV int mev_compare(const MevNames& N, uint32_t r, const uint8_t* __restrict__ t, uint32_t a, uint32_t b, uint32_t sub) {
  const uint32_t n0 = N.off[r], nl = N.off[r + 1u] - n0, rl = b - a, longer = nl > rl ? nl : rl;
  for (uint32_t i0 = 0; i0 < longer; i0 += MEV_LANES) {  // (uniform over the row)
    const uint32_t i = i0 + sub;
    const uint32_t cn = i < nl ? (uint32_t)N.blob[n0 + i] + 1u : 0u, ct = i < rl ? (uint32_t)t[a + i] + 1u : 0u;
    const uint32_t m = fsam_ballot(cn != ct);
    if (m) {
      const uint32_t first = (uint32_t)__builtin_ctz(m);
      return (int)sam_row_lane(cn, first) - (int)sam_row_lane(ct, first);
    }
  }
  return 0;
}

// the row of RNAME text[a, b) among the sorted names; MEV_NO_ROW: not one of them
SIMMR_DEV uint32_t mev_name_row(const MevNames& N, const uint8_t* __restrict__ t, uint32_t a, uint32_t b, uint32_t sub) {
  if (b - a > SAM_RNAME_MAX || b == a) return MEV_NO_ROW;
  uint32_t lo = 0, hi = N.n;
  while (lo < hi) {  // (uniform over the row)
    const uint32_t mid = lo + (hi - lo) / 2u;
    const int c = mev_compare(N, mid, t, a, b, sub);
    if (c == 0) return mid;
    if (c < 0) lo = mid + 1u;
    else hi = mid;
  }
  return MEV_NO_ROW;
}

// the first index of key[0, n) whose key is not below k (n: none).  A round puts 16 pivots, a lane each, across the open range and
// keeps the sixteenth the ballot names: 100 M keys take 7 rounds of one probe each.
SIMMR_DEV uint64_t mev_lower_bound(const uint64_t* __restrict__ key, uint64_t n, uint64_t k, uint32_t sub) {
  uint64_t a = 0, b = n;  // the answer is in [a, b]
  while (a < b) {         // (uniform over the row)
    const uint64_t step = (b - a + MEV_LANES - 1u) / MEV_LANES, at = a + (uint64_t)sub * step;
    const uint32_t below = (uint32_t)__popc(fsam_ballot(at < b && key[at] < k));  // the pivots ascend: the lanes below k are the first ones
    if (below == 0u) { b = a; break; }
    const uint64_t next = a + (uint64_t)below * step;
    a = a + (uint64_t)(below - 1u) * step + 1u;
    b = next < b ? next : b;
  }
  return a;
}

// The fields of the line at `line`, its numbers and its CIGAR sums.  bad: fewer than 11 fields, a FLAG / MAPQ / POS that is no
// number, a MAPQ above 255, a POS above 2^31 - 1, a CIGAR that is neither "*" nor (<1..9 digits><op>)+, an interval's end above 2^40.
SIMMR_DEV MevLine mev_read_line(const uint8_t* __restrict__ t, uint64_t n, uint32_t line, uint32_t sub) {
  MevLine L{};
  uint32_t tb[6];
#pragma unroll
  for (uint32_t j = 0; j < 6u; j++) tb[j] = FSAM_NONE;
  uint32_t n_tab = 0;
  for (uint64_t p0 = line;; p0 += MEV_LANES) {
    const uint64_t p = p0 + sub;
    const uint32_t c = p < n ? t[p] : '\n';
    uint32_t m_tab = fsam_ballot(c == '\t');
    const uint32_t m_nl = fsam_ballot(c == '\n');
    if (m_nl) m_tab &= (1u << (uint32_t)__builtin_ctz(m_nl)) - 1u;
    for (; m_tab; m_tab &= m_tab - 1u) {
      const uint32_t at = (uint32_t)p0 + (uint32_t)__builtin_ctz(m_tab);
#pragma unroll
      for (uint32_t j = 0; j < 6u; j++)
        if (n_tab == j) tb[j] = at;
      n_tab++;
    }
    if (m_nl) break;
  }
  if (n_tab < 10u) { L.bad = 1u; return L; }
  const uint32_t cigar = tb[4] + 1u, cigar_end = tb[5];
  L.rname = tb[1] + 1u;
  L.rname_end = tb[2];
  L.rname_star = L.rname_end - L.rname == 1u && t[L.rname] == '*' ? 1u : 0u;
  const bool numbers = fsam_field_number(t, tb[0] + 1u, tb[1], false, &L.flag) && fsam_field_number(t, tb[2] + 1u, tb[3], false, &L.pos) &&
                       fsam_field_number(t, tb[3] + 1u, tb[4], false, &L.mapq);
  L.id_ok = fsam_field_number(t, line, tb[0], false, &L.id) && L.id < MEV_MAX_ID ? 1u : 0u;
  const bool cigar_star = cigar_end - cigar == 1u && t[cigar] == '*';
  uint32_t bad = numbers && cigar_end > cigar && L.mapq <= 255u && L.pos <= MEV_MAX_POS ? 0u : 1u;
  uint64_t s = 0;
  uint32_t other = 0;
  if (!cigar_star && !bad) {
    if (fsam_digit(t[cigar_end - 1u])) bad = 1u;
    for (uint64_t p0 = cigar; p0 < cigar_end; p0 += MEV_LANES) {
      uint32_t len;
      const uint32_t kind = fsam_cigar_lane(t, cigar, cigar_end, p0 + sub, &len);
      s += kind == 1u || kind == 3u ? len : 0u;
      other |= kind == 6u ? 1u : 0u;
      bad |= kind == 7u ? 1u : 0u;
    }
    bad = fsam_row_or(bad);
    other = fsam_row_or(other);
    s = fsam_row_sum64(s);
  }
  L.span = s;
  if (!bad && (L.pos ? L.pos - 1u : 0u) + s > MEV_MAX_END) bad = 1u;
  L.bad = bad;
  L.other_op = other;
  return L;
}

// The kernels.  ovleval_kernels.hip (a translation unit of its own) includes this file with MEV_ROUTINES_ONLY defined and takes the
// routines above without them, as this file takes fit_sam_kernels.hip's.
#ifndef MEV_ROUTINES_ONLY
// ---- the line index -----------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(FSAM_WG)
k_mev_index(const uint8_t* __restrict__ text, uint64_t n_bytes, uint64_t n_tiles, uint64_t* __restrict__ tile_sum,
            const uint64_t* __restrict__ tile_prefix, uint32_t* __restrict__ starts, uint64_t start_capacity) {
  __shared__ uint32_t lds[FSAM_WG];
  fsam_index_tiles(text, n_bytes, n_tiles, tile_sum, tile_prefix, starts, start_capacity, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_mev_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

#define MEV_COUNT(which) do { if (sub == 0u) atomicAdd(counts + (which), 1ull); } while (0)

// ---- the truth ----------------------------------------------------------------------------------------------------------------
// cursor[0]: the entries so far (never reset between adds), cursor[1]: the largest key
extern "C" __global__ void __launch_bounds__(MEV_WG)
k_mev_truth(MevText W, MevNames N, MevEntries E, uint64_t capacity, unsigned long long* __restrict__ cursor,
            unsigned long long* __restrict__ counts, uint32_t* __restrict__ err) {
  const uint8_t* __restrict__ t = W.text;
  const uint32_t sub = threadIdx.x & (MEV_LANES - 1u), row = threadIdx.x / MEV_LANES;
  const uint64_t n_lines = *W.n_lines, n = W.n_bytes;
  const uint64_t n_batches = (n_lines + MEV_WG_RECS - 1u) / MEV_WG_RECS;
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t li = batch * MEV_WG_RECS + row;
    if (li >= n_lines) continue;  // (uniform over the row)
    const uint32_t line = W.starts[li];
    if (line >= n) continue;      // (never: the index holds places of the text)
    MEV_COUNT(MC_T_LINES);
    if (t[line] == '@') { MEV_COUNT(MC_T_HEADER); continue; }
    const MevLine L = mev_read_line(t, n, line, sub);
    if (L.bad) { if (sub == 0u) atomicOr(err, MEV_ERR_TRUTH); continue; }
    if ((L.flag & 0x904u) || L.other_op) { MEV_COUNT(MC_T_SKIPPED); continue; }
    const uint32_t name = mev_name_row(N, t, L.rname, L.rname_end, sub);
    if (!L.id_ok || name == MEV_NO_ROW || L.pos == 0u) { if (sub == 0u) atomicOr(err, MEV_ERR_TRUTH); continue; }
    MEV_COUNT(MC_T_ENTRIES);
    if (sub == 0u) {
      const uint64_t key = L.id << 1 | ((L.flag >> 7) & 1u);
      const unsigned long long slot = atomicAdd(cursor, 1ull);
      atomicMax(cursor + 1, (unsigned long long)key);
      if (slot < capacity) {  // (always: an add's lines are fewer than its bytes / MEV_MIN_LINE + 1)
        E.key[slot] = key;
        E.meta[slot] = name | (uint32_t)((L.flag >> 4) & 1u) << 31;
        E.lo[slot] = L.pos - 1u;
        E.hi[slot] = L.pos - 1u + L.span;
      }
    }
  }
}

// the entry columns into key order (perm == nullptr: a key without bits, the order is the identity), and equal neighbours
extern "C" __global__ void __launch_bounds__(256)
k_mev_gather(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ perm, MevEntries U, MevEntries S, uint64_t n, uint32_t* __restrict__ err) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t from = perm ? perm[i] : i;
    if (from >= n) continue;  // (never: the sort writes a permutation)
    S.meta[i] = U.meta[from];
    S.lo[i] = U.lo[from];
    S.hi[i] = U.hi[from];
    if (i + 1u < n && skey[i] == skey[i + 1u]) atomicOr(err, MEV_ERR_DUP);
  }
}

// ---- the aligned records ------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(MEV_WG)
k_mev_record(MevText W, MevNames N, const uint64_t* __restrict__ skey, MevEntries S, uint64_t n_entries, uint32_t min_pct,
             unsigned long long* __restrict__ counts, unsigned long long* __restrict__ by_mapq, uint32_t* __restrict__ best,
             uint32_t* __restrict__ hits, uint32_t* __restrict__ err) {
  __shared__ uint32_t l_mapq[512];
  const uint8_t* __restrict__ t = W.text;
  const uint32_t tid = threadIdx.x, sub = tid & (MEV_LANES - 1u), row = tid / MEV_LANES;
  for (uint32_t i = tid; i < 512u; i += MEV_WG) l_mapq[i] = 0u;
  __syncthreads();
  const uint64_t n_lines = *W.n_lines, n = W.n_bytes;
  const uint64_t n_batches = (n_lines + MEV_WG_RECS - 1u) / MEV_WG_RECS;
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t li = batch * MEV_WG_RECS + row;
    if (li >= n_lines) continue;  // (uniform over the row)
    const uint32_t line = W.starts[li];
    if (line >= n) continue;      // (never)
    MEV_COUNT(MC_LINES);
    if (t[line] == '@') { MEV_COUNT(MC_HEADER); continue; }
    MEV_COUNT(MC_RECORDS);
    const MevLine L = mev_read_line(t, n, line, sub);
    if (L.bad) { if (sub == 0u) atomicOr(err, MEV_ERR_ALIGNED); continue; }
    if (L.flag & 0x900u) { MEV_COUNT(MC_SECONDARY); continue; }
    if (L.other_op) { MEV_COUNT(MC_CIGAR_OP); continue; }
    if (!L.id_ok) { MEV_COUNT(MC_UNKNOWN_READ); continue; }
    const uint64_t key = L.id << 1 | ((L.flag >> 7) & 1u);
    const uint64_t at = mev_lower_bound(skey, n_entries, key, sub);
    if (at >= n_entries || skey[at] != key) { MEV_COUNT(MC_UNKNOWN_READ); continue; }
    uint32_t cls;
    if ((L.flag & 4u) || L.rname_star) {
      cls = 1u;
      MEV_COUNT(MC_UNMAPPED);
    } else {
      if (L.pos == 0u) { if (sub == 0u) atomicOr(err, MEV_ERR_ALIGNED); continue; }
      const uint32_t name = mev_name_row(N, t, L.rname, L.rname_end, sub);
      cls = 2u;
      if (name == MEV_NO_ROW) {
        MEV_COUNT(MC_UNKNOWN_REF);
      } else {
        const uint32_t meta = S.meta[at];
        const uint64_t lo = L.pos - 1u, hi = lo + L.span, tlo = S.lo[at], thi = S.hi[at];
        const uint64_t s = lo > tlo ? lo : tlo, e = hi < thi ? hi : thi, ov = e > s ? e - s : 0u;
        const uint64_t un = (hi > thi ? hi : thi) - (lo < tlo ? lo : tlo);
        if (meta == (name | (uint32_t)((L.flag >> 4) & 1u) << 31) && ov >= 1u && 100u * ov >= (uint64_t)min_pct * un) cls = 3u;
      }
      MEV_COUNT(cls == 3u ? MC_CORRECT : MC_WRONG);
      if (sub == 0u) atomicAdd(&l_mapq[2u * (uint32_t)L.mapq + (cls == 3u ? 0u : 1u)], 1u);
    }
    if (sub == 0u) {
      atomicMax(best + at, cls << 8 | (uint32_t)L.mapq);
      atomicAdd(hits + at, 1u);
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < 512u; i += MEV_WG) {
    const uint32_t v = l_mapq[i];
    if (v) atomicAdd(by_mapq + i, (unsigned long long)v);
  }
}

// ---- the entries by their best record -----------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
k_mev_reduce(const uint32_t* __restrict__ best, const uint32_t* __restrict__ hits, uint64_t n, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t l_sum[5];
  if (threadIdx.x < 5u) l_sum[threadIdx.x] = 0u;
  __syncthreads();
  for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += (uint64_t)gridDim.x * 256u) {  // (uniform over the workgroup)
    const uint64_t i = i0 + threadIdx.x;
    uint32_t c[5] = {0u, 0u, 0u, 0u, 0u};  // missing, multiple, correct, wrong, unmapped
    if (i < n) {
      const uint32_t h = hits[i], cls = best[i] >> 8;
      c[0] = h == 0u ? 1u : 0u;
      c[1] = h > 1u ? 1u : 0u;
      c[2] = cls == 3u ? 1u : 0u;
      c[3] = cls == 2u ? 1u : 0u;
      c[4] = cls == 1u ? 1u : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < 5u; j++) {
      const uint32_t m = (uint32_t)__popcll(__ballot(c[j] != 0u));
      if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&l_sum[j], m);
    }
    __syncthreads();
    if (threadIdx.x < 5u && l_sum[threadIdx.x]) {
      atomicAdd(counts + MC_MISSING + threadIdx.x, (unsigned long long)l_sum[threadIdx.x]);
      l_sum[threadIdx.x] = 0u;
    }
    __syncthreads();
  }
}

#undef MEV_COUNT
#endif  // MEV_ROUTINES_ONLY

}  // namespace simmr
