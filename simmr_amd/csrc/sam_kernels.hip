// sam_kernels.hip — the true alignments as SAM text on the device (gfx950): one alignment line per read, from the read
// columns and the truth pass's edit lists (include/simmr_hip.h states the record).  Included by sam.hip alone, the
// library's sixth translation unit: nothing here is seen by the other units, whose kernel budgets stay what they were, and
// nothing of kernels.hip is needed — the pass never touches the genome planes (MD and NM come from edit_pos / edit_ref).
//
// Four kernels.  No place comes from an atomic: sizes are counted, scanned, and the records written at their offsets, so
// launch geometry never changes a byte.
//   k_sam_size     every record's length (len[r], 32 bits) and the sum of every chunk of SAM_CHUNK reads;
//   k_sam_scan     ONE workgroup: exclusive scan of the chunk sums (64 bits), the total behind the last;
//   k_sam_offsets  a workgroup per chunk: off[r] = its chunk's prefix + the scan of the chunk's lengths;
//   k_sam_write    the records, at off[r].
// k_sam_size and k_sam_write are one routine, sam_record<WRITE>, so that a record's length and its bytes cannot disagree.
// The loops around it — over chunks for the sizes, over row batches for the writer — are rec_size_chunks and rec_write_places
// of record_stream.hpp, shared with the BAM writer and the sorted forms; SamRec below is what they know of a SAM record.
//
// Work item: a read.  SAM_LANES = 16 lanes (one DPP row) share it, as in the truth pass.  The record is five runs:
//   head   QNAME .. TLEN and their tabs (and "*\t*" for a read without bases): lane 0 of the row formats it into an LDS
//          slot with the decimal pieces of fastq_format.hpp, the row copies it out in 16-byte windows;
//   SEQ    the read's bases, 16 per lane and round: one unaligned 16-byte load, for a reverse read a byte reversal and the
//          complement, every byte outside ACGTN turned into N (word-parallel compares), one unaligned 16-byte store;
//   QUAL   the tab before it and the qualities, the same way (the tab is shifted into the first window);
//   tail   "\tNM:i:<n>\tMD:Z:" — lane 0, LDS, copied as dwords;
//   MD     token j of the n + 1 is the decimal gap before forward edit j and that edit's reference base, the last one the
//          gap behind the last edit and the '\n'.  Lane s of a round takes token 16 i + s; its place is the running cursor
//          + the row's exclusive prefix of token lengths (DPP row_shr, no LDS memory).  A token is at most six bytes and goes out
//          as a dword, a halfword and a byte at most.
// The windows of a run: window g starts at byte 16 g, except the last one, which ends AT the run's end (it overlaps its
// neighbour with identical bytes), so no load leaves the read in either layout — compact reads have no slack behind
// them, and the reverse mates of SIMMR_SLOT16 are right-aligned in their slots — and no store is partial.  Reads shorter
// than 16 bases are loaded and stored bytewise.
// Bounds.  sam_open checks a read before any address is formed from it (names, seq[], the edit columns); a refused read
// sets the error word and loads and stores nothing.  Every store of record r is bounded by off[r + 1] - off[r] (`room`),
// as k_truth<true> bounds its stores by `limit`: columns changed between the plan and the emit cannot carry a store out
// of the record.
// sam_sort_kernels.hip (the coordinate-sorted form, a unit of its own) includes this file with SAM_ROUTINES_ONLY defined: the
// constants, the record routine, its policy SamRec, the bodies of record_stream.hpp and the scans' bodies without the four
// kernels, which stay in sam.hip's budget alone.  For that form the place of a record is a parameter of sam_record (`at`: the
// entry of off[] the record starts at) beside the read it shows: here the two are the same number.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#include "device_types.hpp"

namespace simmr {

#define SAM_LANES 16u         /* lanes per read: one DPP row */
#define SAM_WG_READS 16u      /* reads per 256-thread workgroup and iteration */
#define SAM_WGS_PER_CU 8u     /* k_sam_write's grid is capped at this many workgroups per CU; beyond it workgroups loop */
#define SAM_CHUNK 1024u       /* reads per chunk of the size pass and of the scan */
#define SAM_MAX_L 65535u      /* longest read */
#define SAM_RNAME_MAX 254u    /* longest RNAME */
#define SAM_HEAD_PITCH 364u   /* LDS bytes of a head: 10 + 1 + 3 + 1 + 254 + 1 + 20 + 5 + 6 + 2 + 20 + 1 + 21 + 1 + 3 and the writer's slack */
#define SAM_TAIL_PITCH 36u    /* LDS bytes of a tail: 6 + 5 + 6 and the writer's slack */

#ifndef SIMMR_DEV
#define SIMMR_DEV __device__ __forceinline__
#endif
typedef uint64_t __attribute__((aligned(1))) u64_unaligned;
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
typedef uint16_t __attribute__((aligned(1))) u16_unaligned;
typedef uint32_t v4u32 __attribute__((ext_vector_type(4)));
typedef v4u32 __attribute__((aligned(1))) v4u32_unaligned;
typedef const __attribute__((address_space(1))) u64_unaligned* global_u64_unaligned_ptr;
typedef const __attribute__((address_space(1))) v4u32_unaligned* global_v4u32_unaligned_ptr;

#include "fastq_format.hpp"  // dec_digits, fq_eight_digits and the aligned LDS writer (plain device routines, no kernel)

struct SamReads {  // the columns simmr_*_emit filled (device pointers), every one of them
  const uint8_t* seq;
  const uint8_t* qual;
  const uint64_t* seq_off;
  const uint64_t* start;
  const uint64_t* end;
  const uint32_t* contig;
  const uint32_t* genome;
  const uint32_t* read_id;
  const uint8_t* flags;
  uint64_t seq_capacity;
  uint32_t slot16;
};
struct SamEdits {  // of simmr_truth_out
  const uint64_t* off;
  const uint32_t* pos;
  const uint8_t* ref;
  uint64_t capacity;
};
struct SamNames {
  const uint8_t* blob;        // the RNAMEs back to back; 8 bytes of padding
  const uint32_t* g_cbase;    // per engine genome slot: first row of its contigs in c_off / c_len
  const uint32_t* g_ncontig;  // 0 for a slot without names
  const uint32_t* c_off;
  const uint32_t* c_len;
  uint32_t n_slots;
};

// inclusive scan of one u32 over each row of 16 lanes (every lane of the row active): kernels.hip's ladder, restated
// because including that file would bring its kernels into this unit's budget
SIMMR_DEV uint32_t sam_row_scan(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);  // row_shr:8
  return v;
}
SIMMR_DEV uint32_t sam_row_lane(uint32_t v, uint32_t from) { return (uint32_t)__shfl((int)v, (int)from, (int)SAM_LANES); }

// up to eight characters as the bytes of a 64-bit word, first character lowest
template <unsigned N>
constexpr uint64_t sam_lit(const char (&s)[N]) {
  static_assert(N <= 9, "a literal piece is at most eight bytes");
  uint64_t v = 0;
  for (unsigned i = 0; i + 1 < N; i++) v |= (uint64_t)(uint8_t)s[i] << (8u * i);
  return v;
}

// ---- bytes ----------------------------------------------------------------------------------------------------------
// 0xff in every byte of x that equals the byte repeated in pat
SIMMR_DEV uint32_t sam_eq_bytes(uint32_t x, uint32_t pat) {
  const uint32_t t = x ^ pat;
  const uint32_t nz = (((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u;
  return ((nz ^ 0x80808080u) >> 7) * 0xffu;
}
// four bases as SAM shows them: A C G T N kept (forward) or complemented (reverse), every other byte N
SIMMR_DEV uint32_t sam_bases4(uint32_t x, uint32_t rev) {
  const uint32_t A = 0x41414141u, C = 0x43434343u, G = 0x47474747u, T = 0x54545454u, N = 0x4e4e4e4eu;
  return N ^ (sam_eq_bytes(x, A) & ((rev ? T : A) ^ N)) ^ (sam_eq_bytes(x, C) & ((rev ? G : C) ^ N)) ^
         (sam_eq_bytes(x, G) & ((rev ? C : G) ^ N)) ^ (sam_eq_bytes(x, T) & ((rev ? A : T) ^ N));
}
SIMMR_DEV uint32_t sam_base1(uint32_t b, uint32_t rev) { return sam_bases4(b, rev) & 0xffu; }
SIMMR_DEV v4u32 sam_reverse16(v4u32 v) {
  return v4u32{__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x)};
}
// the 16 bytes one place up, `c` in the first
SIMMR_DEV v4u32 sam_shift_in_front(v4u32 v, uint32_t c) {
  return v4u32{(v.x << 8) | c, __builtin_amdgcn_alignbyte(v.y, v.x, 3u), __builtin_amdgcn_alignbyte(v.z, v.y, 3u),
               __builtin_amdgcn_alignbyte(v.w, v.z, 3u)};
}

// ---- bounded stores: [at, at + n) of a record of `room` bytes, or nothing --------------------------------------------
SIMMR_DEV void sam_store16(uint8_t* rec, uint32_t at, uint32_t room, v4u32 v) {
  if (at <= room && room - at >= 16u) *reinterpret_cast<v4u32_unaligned*>(rec + at) = v;
}
SIMMR_DEV void sam_store4(uint8_t* rec, uint32_t at, uint32_t room, uint32_t v) {
  if (at <= room && room - at >= 4u) *reinterpret_cast<u32_unaligned*>(rec + at) = v;
}
SIMMR_DEV void sam_store1(uint8_t* rec, uint32_t at, uint32_t room, uint32_t v) {
  if (at < room) rec[at] = (uint8_t)v;
}
// the low n (<= 7) bytes of v: a dword, a halfword and a byte at most
SIMMR_DEV void sam_store_token(uint8_t* rec, uint32_t at, uint32_t room, uint64_t v, uint32_t n) {
  if (at > room || room - at < n) return;
  uint8_t* p = rec + at;
  if (n & 4u) { *reinterpret_cast<u32_unaligned*>(p) = (uint32_t)v; v >>= 32; p += 4; }
  if (n & 2u) { *reinterpret_cast<u16_unaligned*>(p) = (uint16_t)v; v >>= 16; p += 2; }
  if (n & 1u) *p = (uint8_t)v;
}

// n bytes of an LDS slot (4-byte aligned; its words are readable up to 20 bytes past n) to record bytes [at, at + n), by
// the row: 16-byte windows, the last one ending at the run's end; fewer than 16 bytes as dwords and then bytes
SIMMR_DEV void sam_copy_slot(const uint8_t* slot, uint32_t n, uint8_t* rec, uint32_t at, uint32_t room, uint32_t sub) {
  if (n >= 16u) {
    const uint32_t nw = (n + 15u) >> 4;
    for (uint32_t g = sub; g < nw; g += SAM_LANES) {
      const uint32_t k = 16u * g + 16u <= n ? 16u * g : n - 16u;
      sam_store16(rec, at + k, room, fq_read16(slot, k));
    }
  } else {
    const uint32_t nd = n >> 2;
    if (sub < nd) sam_store4(rec, at + 4u * sub, room, reinterpret_cast<const uint32_t*>(slot)[sub]);
    else if (sub - nd < (n & 3u)) sam_store1(rec, at + 4u * nd + (sub - nd), room, slot[4u * nd + (sub - nd)]);
  }
}

// ---- a read, opened -------------------------------------------------------------------------------------------------
// Every lane of a row reads the same columns (one address per row) and so takes the same branch: all-or-nothing per row,
// which keeps the DPP rows whole.  good == false: the row has no read, or the read was refused (the error word is set).
struct SamRead {
  uint64_t so, qb, e0, lo, pnext, span;
  uint32_t L, rev, n, flag, read_id, name_off, name_len, neg;
  bool good;
};
SIMMR_DEV SamRead sam_open(const SamReads& rd, const SamEdits& ed, const SamNames& nm, uint64_t r, uint64_t n_reads, uint32_t paired,
                           uint32_t* __restrict__ err, bool raise) {
  SamRead R{};
  if (r >= n_reads) return R;
  const uint64_t a = rd.start[r], b = rd.end[r];
  const uint64_t lo = a < b ? a : b, hi = a < b ? b : a, len = hi - lo;
  const uint32_t g = rd.genome[r], c = rd.contig[r];
  const uint64_t so = rd.seq_off[r], so1 = rd.seq_off[r + 1], e0 = ed.off[r], e1 = ed.off[r + 1];
  const uint32_t rev = rd.flags[r] & SIMMR_FLAG_REVCOMP;
  bool ok = len <= SAM_MAX_L && so <= so1 && so1 <= rd.seq_capacity && len <= so1 - so && e0 <= e1 && e1 <= ed.capacity &&
            e1 - e0 <= len && g < nm.n_slots;
  if (ok) ok = c < nm.g_ncontig[g];
  if (!ok) {
    if (raise) atomicOr(err, 1u);
    return R;
  }
  const uint32_t row = nm.g_cbase[g] + c;
  R.name_off = nm.c_off[row];
  R.name_len = nm.c_len[row];
  R.so = so;
  R.qb = rd.slot16 ? (so & ~15ull) : so;
  R.e0 = e0;
  R.n = (uint32_t)(e1 - e0);
  R.lo = lo;
  R.L = (uint32_t)len;
  R.rev = rev;
  R.read_id = rd.read_id[r];
  R.flag = rev ? 0x10u : 0u;
  if (paired) {
    const uint64_t ma = rd.start[r ^ 1ull], mb = rd.end[r ^ 1ull];  // (n_reads is even: the mate is a read of the call)
    const uint64_t mlo = ma < mb ? ma : mb, mhi = ma < mb ? mb : ma;
    const uint32_t mrev = rd.flags[r ^ 1ull] & SIMMR_FLAG_REVCOMP;
    R.flag |= 0x1u | 0x2u | (mrev ? 0x20u : 0u) | ((r & 1u) ? 0x80u : 0x40u);
    R.pnext = mlo + 1u;
    R.span = (hi > mhi ? hi : mhi) - (lo < mlo ? lo : mlo);
    const bool first = lo < mlo || (lo == mlo && !(r & 1u));  // the mate with the smaller lo is positive; on a tie mate 1
    R.neg = (!first && R.span != 0u) ? 1u : 0u;
  }
  R.good = true;
  return R;
}

// the head's bytes without writing it (what sam_format_head returns)
SIMMR_DEV uint32_t sam_head_len(const SamRead& R, uint32_t paired) {
  uint32_t n = dec_digits(R.read_id) + 1u + dec_digits(R.flag) + 1u + R.name_len + 1u + dec_digits(R.lo + 1u) + 5u;
  n += R.L ? dec_digits(R.L) + 2u : 2u + 3u;
  n += paired ? 2u + dec_digits(R.pnext) + 1u + R.neg + dec_digits(R.span) + 1u : 6u;
  return n;
}
// The head into an LDS slot.  Eight pieces — a literal of up to eight bytes, then a number or the name — in ONE loop, so
// that the decimal writer and the id copy exist once in the kernel, not once per field.
SIMMR_DEV uint32_t sam_format_head(uint8_t* slot, const SamRead& R, uint32_t paired, const uint8_t* __restrict__ blob) {
  FqW o = fq_begin(slot);
  const bool has = R.L != 0u;
#pragma clang loop unroll(disable)
  for (uint32_t i = 0; i < 8u; i++) {
    uint64_t lit = 0, v = 0;
    uint32_t ln = 0, dec = 0;
    if (i == 0u) { v = R.read_id; dec = 1; }
    else if (i == 1u) { lit = sam_lit("\t"); ln = 1; v = R.flag; dec = 1; }
    else if (i == 2u) { lit = sam_lit("\t"); ln = 1; }
    else if (i == 3u) { lit = sam_lit("\t"); ln = 1; v = R.lo + 1u; dec = 1; }
    else if (i == 4u) { lit = sam_lit("\t255\t*"); ln = has ? 5u : 6u; v = R.L; dec = has; }
    else if (i == 5u) {
      lit = paired ? sam_lit("M\t=\t") : sam_lit("M\t*\t0\t0\t");
      ln = paired ? 4u : 8u;
      if (!has) { lit >>= 8; ln--; }
      v = R.pnext; dec = paired;
    } else if (i == 6u) {
      if (paired) { lit = sam_lit("\t-"); ln = 1u + R.neg; v = R.span; dec = 1; }
    } else {
      lit = paired ? sam_lit("\t*\t*") : sam_lit("*\t*");
      ln = (paired ? 1u : 0u) + (has ? 0u : 3u);
    }
    if (ln) fq_put8(o, lit, ln);
    if (i == 2u) fq_put_global(o, blob + R.name_off, R.name_len);
    else if (dec) fq_put_dec(o, v);
  }
  return o.at;
}

// ---- a record: its length (WRITE == false) or its bytes (WRITE == true) ------------------------------------------------
// Called by all 16 lanes of a row for read r; returns the record's bytes (0 for a refused read) in every lane.  The record
// is bytes off[at] .. off[at + 1] of dst.
template <bool WRITE>
SIMMR_DEV uint32_t sam_record(const SamReads& rd, const SamEdits& ed, const SamNames& nm, uint64_t r, uint64_t at, uint64_t n_reads,
                              uint32_t paired, uint32_t sub, uint8_t* slot, const uint64_t* __restrict__ off, uint8_t* __restrict__ dst,
                              uint32_t* __restrict__ err) {
  const SamRead R = sam_open(rd, ed, nm, r, n_reads, paired, err, sub == 0u);
  if (!R.good) return 0u;
  const uint32_t L = R.L, rev = R.rev, n = R.n;
  uint32_t H, T, room = 0;
  uint8_t* rec = nullptr;
  if (WRITE) {
    const uint64_t o0 = off[at], o1 = off[at + 1];
    room = (o1 >= o0 && o1 - o0 <= 0xffffffffull) ? (uint32_t)(o1 - o0) : 0u;
    rec = dst + o0;
    uint32_t h = 0, t = 0;
    if (sub == 0u) {
      h = sam_format_head(slot, R, paired, nm.blob);
      FqW o = fq_begin(slot + SAM_HEAD_PITCH);
      fq_put8(o, sam_lit("\tNM:i:"), 6u);
      fq_put_dec(o, n);
      fq_put8(o, sam_lit("\tMD:Z:"), 6u);
      t = o.at;
    }
    H = sam_row_lane(h, 0u);
    T = sam_row_lane(t, 0u);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (LDS only: the row reads what its lane 0 wrote)
    __builtin_amdgcn_wave_barrier();
    sam_copy_slot(slot, H, rec, 0u, room, sub);
    // ---- SEQ and QUAL: window g of the bases, and window g of the tab and the qualities (L + 1 bytes)
    if (L >= 16u) {
      const uint8_t* seq = rd.seq + R.so;
      const uint8_t* qual = rd.qual + R.qb;
      const uint32_t nwq = (L + 1u + 15u) >> 4, nws = (L + 15u) >> 4;
      for (uint32_t g = sub; g < nwq; g += SAM_LANES) {
        const uint32_t kq = 16u * g + 16u <= L + 1u ? 16u * g : L + 1u - 16u;  // in the run "\t" + qualities
        const uint32_t kk = kq ? kq - 1u : 0u;                                  // the first quality of the window
        const uint32_t ks = 16u * g + 16u <= L ? 16u * g : L - 16u;
        const bool s_on = g < nws;
        v4u32 q = __builtin_nontemporal_load((global_v4u32_unaligned_ptr)(qual + (rev ? L - 16u - kk : kk)));
        v4u32 s = __builtin_nontemporal_load((global_v4u32_unaligned_ptr)(seq + (rev ? L - 16u - ks : ks)));  // (g == nws: window nws - 1 again, unused)
        if (rev) { q = sam_reverse16(q); s = sam_reverse16(s); }
        s = v4u32{sam_bases4(s.x, rev), sam_bases4(s.y, rev), sam_bases4(s.z, rev), sam_bases4(s.w, rev)};
        if (kq == 0u) q = sam_shift_in_front(q, '\t');
        if (s_on) sam_store16(rec, H + ks, room, s);
        sam_store16(rec, H + L + kq, room, q);
      }
    } else if (L > 0u) {
      if (sub < L) sam_store1(rec, H + (rev ? L - 1u - sub : sub), room, sam_base1(rd.seq[R.so + sub], rev));
      if (sub == 0u) sam_store1(rec, H + L, room, '\t');
      if (sub < L) sam_store1(rec, H + L + 1u + (rev ? L - 1u - sub : sub), room, rd.qual[R.qb + sub]);
    }
    sam_copy_slot(slot + SAM_HEAD_PITCH, T, rec, H + (L ? 2u * L + 1u : 0u), room, sub);
    __builtin_amdgcn_wave_barrier();  // the next read of the row overwrites the slot
  } else {
    H = sam_head_len(R, paired);
    T = 12u + dec_digits(n);
  }
  // ---- MD: tokens j = 0 .. n in forward-strand order; forward edit j is edit j of the read, or n - 1 - j of a reverse one
  const uint32_t md0 = H + (L ? 2u * L + 1u : 0u) + T;
  uint32_t cursor = 0;
  for (uint32_t j0 = 0; j0 <= n; j0 += SAM_LANES) {  // (uniform over the row)
    const uint32_t j = j0 + sub;
    uint32_t tl = 0;
    uint64_t tok = 0;
    if (j <= n) {
      // p: the forward offset of this token's edit (L behind the last), pp: that of the edit before it (-1 before the first)
      int32_t p = (int32_t)L, pp = -1;
      uint32_t c = '\n';
      bool ok = true;
      if (j < n) {
        const uint64_t at = R.e0 + (rev ? n - 1u - j : j);
        const uint32_t x = ed.pos[at];
        ok = x < L;
        p = (int32_t)(rev ? L - 1u - x : x);
        if (WRITE) c = sam_base1(ed.ref[at], rev);  // (a reference N, and every byte outside ACGT, is N in MD)
      }
      if (j > 0u) {
        const uint32_t x = ed.pos[R.e0 + (rev ? n - j : j - 1u)];
        ok = ok && x < L;
        pp = (int32_t)(rev ? L - 1u - x : x);
      }
      ok = ok && p > pp;
      if (ok) {
        const uint32_t gap = (uint32_t)(p - pp - 1), nd = dec_digits(gap);
        tl = nd + 1u;
        if (WRITE) tok = (fq_eight_digits(gap) >> (8u * (8u - nd))) | ((uint64_t)c << (8u * nd));
      } else {
        atomicOr(err, 1u);  // an edit_pos outside the read, or edits that do not ascend
      }
    }
    const uint32_t inc = sam_row_scan(tl);
    if (WRITE) sam_store_token(rec, md0 + cursor + (inc - tl), room, tok, tl);
    cursor += sam_row_lane(inc, SAM_LANES - 1u);
  }
  return md0 + cursor;
}

// exclusive scan of one value per thread over the 256-thread workgroup through LDS; *total = the sum
template <class T>
SIMMR_DEV T sam_wg_scan(T v, T* lds, T* total) {
  const uint32_t t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < 256u; d <<= 1) {
    const T o = t >= d ? lds[t - d] : (T)0;
    __syncthreads();
    lds[t] += o;
    __syncthreads();
  }
  const T inc = lds[t];
  *total = lds[255];
  __syncthreads();
  return inc - v;
}

// ONE workgroup: prefix[c] = the bytes before chunk c, prefix[n] = the total
SIMMR_DEV void sam_scan_chunks(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n, uint64_t* lds) {
  uint64_t carry = 0;
  for (uint64_t base = 0; base < n; base += 256u) {  // (uniform over the workgroup)
    const uint64_t i = base + threadIdx.x;
    uint64_t total;
    const uint64_t ex = sam_wg_scan<uint64_t>(i < n ? sum[i] : 0ull, lds, &total);
    if (i < n) prefix[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) prefix[n] = carry;
}

// a workgroup per chunk, four consecutive reads per thread: off[r] for r < n_reads, and off[n_reads] = the total
SIMMR_DEV void sam_chunk_offsets(const uint32_t* __restrict__ len, const uint64_t* __restrict__ prefix, uint64_t n_reads,
                                 uint64_t* __restrict__ off, uint32_t* lds) {
  const uint64_t n_chunks = (n_reads + SAM_CHUNK - 1u) / SAM_CHUNK;
  if (blockIdx.x == 0 && threadIdx.x == 0) off[n_reads] = prefix[n_chunks];
  for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // (uniform over the workgroup)
    const uint64_t r0 = chunk * SAM_CHUNK + 4u * threadIdx.x;
    uint32_t v[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) v[k] = r0 + k < n_reads ? len[r0 + k] : 0u;
    uint32_t total;
    uint32_t ex = sam_wg_scan<uint32_t>(v[0] + v[1] + v[2] + v[3], lds, &total);  // (a chunk is below 2^30 bytes)
    const uint64_t base = prefix[chunk];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
      if (r0 + k < n_reads) off[r0 + k] = base + ex;
      ex += v[k];
    }
  }
}

// ---- the record policy of record_stream.hpp: what a record is, for the bodies the writers share ---------------------------
// write: the record of read r at entry `at` of off[] (k_sam_write: at == r; the ordered writer of sam_sort_kernels.hip:
// r = perm[at]); slot: the row's SLOT_BYTES of LDS.
struct SamRec {
  static constexpr uint32_t SLOT_BYTES = SAM_HEAD_PITCH + SAM_TAIL_PITCH;
  SIMMR_DEV static uint32_t size(const SamReads& rd, const SamEdits& ed, const SamNames& nm, uint64_t r, uint64_t n_reads, uint32_t paired,
                                 uint32_t sub, uint32_t* __restrict__ err) {
    return sam_record<false>(rd, ed, nm, r, r, n_reads, paired, sub, nullptr, nullptr, nullptr, err);
  }
  SIMMR_DEV static void write(const SamReads& rd, const SamEdits& ed, const SamNames& nm, uint64_t r, uint64_t at, uint64_t n_reads,
                              uint32_t paired, uint32_t sub, uint8_t* slot, const uint64_t* __restrict__ off, uint8_t* __restrict__ dst,
                              uint32_t* __restrict__ err) {
    (void)sam_record<true>(rd, ed, nm, r, at, n_reads, paired, sub, slot, off, dst, err);
  }
};

}  // namespace simmr
#include "record_stream.hpp"  // rec_size_chunks, rec_size_keyed, rec_gather, rec_write_places
namespace simmr {

#ifndef SAM_ROUTINES_ONLY
// ---- sizes ----------------------------------------------------------------------------------------------------------
// A workgroup takes chunks of SAM_CHUNK consecutive reads, 16 at a time, and leaves every chunk's sum: the scan's first level.
extern "C" __global__ void __launch_bounds__(256)
k_sam_size(const SamReads rd, const SamEdits ed, const SamNames nm, uint64_t n_reads, uint32_t paired, uint32_t* __restrict__ len,
           uint64_t* __restrict__ chunk_sum, uint32_t* __restrict__ err) {
  __shared__ uint32_t part[SAM_WG_READS];
  rec_size_chunks<SamRec>(rd, ed, nm, n_reads, paired, len, chunk_sum, err, part);
}

extern "C" __global__ void __launch_bounds__(256)
k_sam_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_sam_offsets(const uint32_t* __restrict__ len, const uint64_t* __restrict__ prefix, uint64_t n_reads, uint64_t* __restrict__ off) {
  __shared__ uint32_t lds[256];
  sam_chunk_offsets(len, prefix, n_reads, off, lds);
}

// ---- the records ------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
k_sam_write(const SamReads rd, const SamEdits ed, const SamNames nm, uint64_t n_reads, uint32_t paired, const uint64_t* __restrict__ off,
            uint8_t* __restrict__ dst, uint32_t* __restrict__ err) {
  __shared__ __attribute__((aligned(16))) uint8_t slots[SAM_WG_READS][SamRec::SLOT_BYTES];
  rec_write_places<SamRec, false>(rd, ed, nm, n_reads, paired, nullptr, off, dst, err, &slots[0][0]);
}
#endif  // SAM_ROUTINES_ONLY

}  // namespace simmr
