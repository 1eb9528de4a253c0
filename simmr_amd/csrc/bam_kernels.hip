// bam_kernels.hip — the true alignments as BAM records, and BGZF framing of any device buffer (include/simmr_hip.h:
// simmr_bam_*, simmr_bgzf_*) on gfx950.  Included by bam.hip, a translation unit of libsimmr_hip.so of its own (and, without
// its kernels, by bam_index_kernels.hip: the same records in coordinate order).  What a
// read is, which reads are refused, the row scan, the bounded stores and the scans' bodies are those of sam_kernels.hip
// (included without its kernels): a BAM record shows the fields of the SAM line of the same read, as integers.
//
// Five kernels.  No place comes from an atomic: sizes are counted, scanned, and the records written at their offsets, so
// launch geometry never changes a byte.
//   k_bam_size     every record's length (len[r], 32 bits) and the sum of every chunk of SAM_CHUNK reads;
//   k_bam_scan     ONE workgroup: exclusive scan of the chunk sums (64 bits), the total behind the last;
//   k_bam_offsets  a workgroup per chunk: off[r] = its chunk's prefix + the scan of the chunk's lengths;
//   k_bam_write    the records, at off[r];
//   k_bgzf_frame   a workgroup per block of BGZF_BLOCK source bytes: header, stored deflate block, CRC-32, ISIZE.
// k_bam_size and k_bam_write are one routine, bam_record<WRITE>, so that a record's length and its bytes cannot disagree.
// The loops around it are rec_size_chunks and rec_write_places of record_stream.hpp, the SAM writer's; BamRec below is what they
// know of a BAM record.
//
// The record (SAM spec 4.2).  Work item: a read, shared by the SAM_LANES = 16 lanes of a DPP row.  No LDS: the few words that
// need formatting are made in registers by every lane of the row (the same instructions whether one lane or sixteen run them)
// and each lane stores the piece that is its own.
//   lanes 0..8   the nine words block_size .. tlen;
//   lanes 9..11  read_name: the digits above 10^8 (none, one or two), the up to eight digits below, and NUL with the CIGAR word;
//   lane 12      the tags' fixed bytes: NM, C or S, the count, MD, Z;
//   seq          16 bytes of packed bases per lane and round: two unaligned 16-byte loads (for a reverse read from the read's
//                other end, byte-reversed), the 4-bit codes by word-parallel compares (a reverse read's complemented), one
//                unaligned 16-byte store.  The windows are those of the SAM writer: window g starts at byte 16 g of the run,
//                except the last one, which ends AT the run's end, so no load leaves the read in either layout and no store
//                is partial.  The run is the L / 2 whole bytes; the half byte of an odd L, and a read of fewer than 32 bases,
//                are packed bytewise;
//   qual         max(byte, 33) - 33, 16 per lane and round, the same windows over L bytes; fewer than 16 bytewise;
//   MD           the tokens of the SAM writer, the last one ending in NUL.
// Every store of record r is bounded by off[r + 1] - off[r]; a refused read sets the error word and loads and stores nothing.
//
// The block (SAM spec 4.1).  Lane i of the 256 takes source bytes BGZF_SEG i .. BGZF_SEG (i + 1) - 1 of its block: 16-byte
// loads, the same 16 bytes stored to the payload (which starts at an odd offset: unaligned stores), and a CRC-32 over them
// by four tables (slicing by four; the tables are staged in LDS).  Lane 0's register starts at 0xffffffff, every other lane's
// at 0: the CRC register is linear in (start value, data), so the block's register is the XOR over the lanes of each lane's
// register shifted by the bytes behind its segment, and shifting by k zero bytes is a multiplication by x^(8k) mod P.  For a
// whole segment followed by whole segments the multiplier is one of BGZF_LANES - 1 constants (seg_mul[], from the host);
// behind them a short block has `rem` = n mod BGZF_SEG more bytes, by which the folded sum is shifted once (rem_mul[rem]) before
// the last lane's register joins it unshifted.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SAM_ROUTINES_ONLY
#include "sam_kernels.hip"

namespace simmr {

#define BAM_FIXED 36u        /* block_size and the 32 bytes of fixed fields */
#define BAM_MAX_POS 0x80000000ull /* pos and the end of the read are int32 */
#define BGZF_BLOCK 65280u    /* source bytes of a block (0xff00, htslib's figure) */
#define BGZF_SEG 256u        /* source bytes of a lane */
#define BGZF_LANES 256u
#define BGZF_HEAD 23u        /* gzip header with the BC field (18) and the stored block's header (5) */
#define BGZF_OVERHEAD 31u    /* BGZF_HEAD, CRC-32 and ISIZE */
#define BGZF_POLY 0xEDB88320u

static_assert(BGZF_BLOCK == (BGZF_LANES - 1u) * BGZF_SEG, "255 lanes take a whole block; the last one has none of it");
static_assert(BGZF_BLOCK + BGZF_OVERHEAD - 1u <= 0xffffu, "BSIZE is 16 bits");

// ---- BAM: bytes -----------------------------------------------------------------------------------------------------
// four bases as BAM's 4-bit codes, one per byte: A 1, C 2, G 4, T 8 (complemented for a reverse read), every other byte 15
SIMMR_DEV uint32_t bam_codes4(uint32_t x, uint32_t rev) {
  const uint32_t A = 0x41414141u, C = 0x43434343u, G = 0x47474747u, T = 0x54545454u, N = 0x0f0f0f0fu;
  const uint32_t c1 = 0x01010101u, c2 = 0x02020202u, c4 = 0x04040404u, c8 = 0x08080808u;
  return N ^ (sam_eq_bytes(x, A) & ((rev ? c8 : c1) ^ N)) ^ (sam_eq_bytes(x, C) & ((rev ? c4 : c2) ^ N)) ^
         (sam_eq_bytes(x, G) & ((rev ? c2 : c4) ^ N)) ^ (sam_eq_bytes(x, T) & ((rev ? c1 : c8) ^ N));
}
// the codes of eight bases (a first, its lowest byte first) as four bytes, the earlier base of a byte in the high nibble
SIMMR_DEV uint32_t bam_pack8(uint32_t a, uint32_t b) {
  const uint32_t pa = ((a << 4) | (a >> 8)) & 0x00ff00ffu, pb = ((b << 4) | (b >> 8)) & 0x00ff00ffu;
  return ((pa | (pa >> 8)) & 0xffffu) | ((pb | (pb >> 8)) << 16);
}
SIMMR_DEV uint32_t bam_pack16(v4u32 s, uint32_t half, uint32_t rev) {  // bytes 8 half .. 8 half + 7 of s
  return bam_pack8(bam_codes4(half ? s.z : s.x, rev), bam_codes4(half ? s.w : s.y, rev));
}
// four qualities: max(byte, 33) - 33 in every byte
SIMMR_DEV uint32_t bam_quals4(uint32_t x) {
  const uint32_t t = (x | 0x80808080u) - 0x21212121u;  // (no borrow between the bytes); bit 7: the low seven bits are >= 33
  const uint32_t m7 = t & 0x80808080u, hx = x & 0x80808080u;
  const uint32_t keep = ((m7 | hx) >> 7) * 0xffu;
  return ((t & 0x7f7f7f7fu) | (hx & m7)) & keep;
}
// the low n (<= 8) bytes of v at [at, at + n) of a record of `room` bytes, or nothing
SIMMR_DEV void bam_store_le(uint8_t* rec, uint32_t at, uint32_t room, uint64_t v, uint32_t n) {
  if (n == 0u || at > room || room - at < n) return;
  if (n & 8u) {
    *reinterpret_cast<u32_unaligned*>(rec + at) = (uint32_t)v;
    *reinterpret_cast<u32_unaligned*>(rec + at + 4u) = (uint32_t)(v >> 32);
    return;
  }
  sam_store_token(rec, at, room, v, n);
}
// SAM spec 5.3 for [beg, end), the 16 bits the field holds
SIMMR_DEV uint32_t bam_reg2bin(uint32_t beg, uint32_t end) {
  end--;
  uint32_t bin = 0u;
  if (beg >> 14 == end >> 14) bin = 4681u + (beg >> 14);
  else if (beg >> 17 == end >> 17) bin = 585u + (beg >> 17);
  else if (beg >> 20 == end >> 20) bin = 73u + (beg >> 20);
  else if (beg >> 23 == end >> 23) bin = 9u + (beg >> 23);
  else if (beg >> 26 == end >> 26) bin = 1u + (beg >> 26);
  return bin & 0xffffu;
}

// sam_open behind BAM's own refusal: a read that ends at 2^31 or beyond sets the error word and has nothing else loaded
SIMMR_DEV SamRead bam_open(const SamReads& rd, const SamEdits& ed, const SamNames& nm, uint64_t r, uint64_t n_reads, uint32_t paired,
                           uint32_t* __restrict__ err, bool raise) {
  if (r < n_reads) {
    const uint64_t a = rd.start[r], b = rd.end[r];
    if ((a > b ? a : b) >= BAM_MAX_POS) {
      if (raise) atomicOr(err, 1u);
      return SamRead{};
    }
  }
  return sam_open(rd, ed, nm, r, n_reads, paired, err, raise);
}

// ---- a record: its length (WRITE == false) or its bytes (WRITE == true) ------------------------------------------------
// Called by all 16 lanes of a row for read r; returns the record's bytes (0 for a refused read) in every lane.  The record is
// bytes off[place] .. off[place + 1] of dst: place == r in read order; the ordered writer of bam_index_kernels.hip gives the
// read's place in coordinate order.
template <bool WRITE>
SIMMR_DEV uint32_t bam_record(const SamReads& rd, const SamEdits& ed, const SamNames& nm, uint64_t r, uint64_t place, uint64_t n_reads,
                              uint32_t paired, uint32_t sub, const uint64_t* __restrict__ off, uint8_t* __restrict__ dst,
                              uint32_t* __restrict__ err) {
  const SamRead R = bam_open(rd, ed, nm, r, n_reads, paired, err, sub == 0u);
  if (!R.good) return 0u;
  const uint32_t L = R.L, rev = R.rev, n = R.n;
  const uint32_t nd = dec_digits(R.read_id);
  const uint32_t H = BAM_FIXED + nd + 1u + (L ? 4u : 0u);  // the fixed fields, read_name, cigar
  const uint32_t NB = (L + 1u) >> 1;                       // seq
  const uint32_t T = (n <= 255u ? 4u : 5u) + 3u;           // NM and its count, "MDZ"
  const uint32_t md0 = H + NB + L + T;
  uint32_t room = 0;
  uint8_t* rec = nullptr;
  if (WRITE) {
    const uint64_t o0 = off[place], o1 = off[place + 1];
    room = (o1 >= o0 && o1 - o0 <= 0xffffffffull) ? (uint32_t)(o1 - o0) : 0u;
    rec = dst + o0;
    // ---- the fixed fields, read_name, cigar and the tags' fixed bytes: a piece per lane
    {
      const uint32_t lo = (uint32_t)R.lo;
      const uint32_t row = nm.g_cbase[rd.genome[r]] + rd.contig[r];  // (sam_open has checked both)
      uint64_t v = 0;
      uint32_t at = 4u * sub, len = 4u;
      if (sub == 0u) v = room - 4u;
      else if (sub == 1u) v = row;
      else if (sub == 2u) v = lo;
      else if (sub == 3u) v = (nd + 1u) | (255u << 8) | (bam_reg2bin(lo, L ? lo + L : lo + 1u) << 16);
      else if (sub == 4u) v = (L ? 1u : 0u) | (R.flag << 16);
      else if (sub == 5u) v = L;
      else if (sub == 6u) v = paired ? row : 0xffffffffu;
      else if (sub == 7u) v = paired ? (uint32_t)(R.pnext - 1u) : 0xffffffffu;
      else if (sub == 8u) v = paired ? (R.neg ? 0u - (uint32_t)R.span : (uint32_t)R.span) : 0u;
      else {
        const uint32_t id = R.read_id, hi = id / 100000000u, low = id - hi * 100000000u;  // hi < 43
        const uint32_t nh = nd > 8u ? nd - 8u : 0u, nl = nd - nh;
        if (sub == 9u) {
          const uint32_t h1 = hi / 10u, h0 = hi - h1 * 10u;
          v = nh == 2u ? (uint64_t)(('0' + h1) | (('0' + h0) << 8)) : (uint64_t)('0' + h0);
          at = BAM_FIXED; len = nh;
        } else if (sub == 10u) {
          v = fq_eight_digits(low) >> (8u * (8u - nl));
          at = BAM_FIXED + nh; len = nl;
        } else if (sub == 11u) {
          v = (uint64_t)(L << 4) << 8;  // NUL, then L << 4 | 0: <L>M
          at = BAM_FIXED + nd; len = L ? 5u : 1u;
        } else if (sub == 12u) {
          const uint32_t wide = n > 255u ? 1u : 0u;
          const uint64_t nm_tag = sam_lit("NM") | ((uint64_t)(wide ? 'S' : 'C') << 16) | ((uint64_t)n << 24);
          v = nm_tag | (sam_lit("MDZ") << (wide ? 40u : 32u));
          at = H + NB + L; len = T;
        } else {
          len = 0u;
        }
      }
      bam_store_le(rec, at, room, v, len);
    }
    // ---- seq: the L / 2 whole bytes in windows of 16, the rest bytewise
    const uint32_t NBe = L >> 1;
    const uint8_t* seq = rd.seq + R.so;
    if (NBe >= 16u) {
      const uint32_t nw = (NBe + 15u) >> 4;
      for (uint32_t g = sub; g < nw; g += SAM_LANES) {
        const uint32_t k = 16u * g + 16u <= NBe ? 16u * g : NBe - 16u;  // output byte; forward bases 2 k .. 2 k + 31
        v4u32 s0 = __builtin_nontemporal_load((global_v4u32_unaligned_ptr)(seq + (rev ? L - 2u * k - 16u : 2u * k)));
        v4u32 s1 = __builtin_nontemporal_load((global_v4u32_unaligned_ptr)(seq + (rev ? L - 2u * k - 32u : 2u * k + 16u)));
        if (rev) { s0 = sam_reverse16(s0); s1 = sam_reverse16(s1); }
        sam_store16(rec, H + k, room, v4u32{bam_pack16(s0, 0u, rev), bam_pack16(s0, 1u, rev), bam_pack16(s1, 0u, rev), bam_pack16(s1, 1u, rev)});
      }
      if ((L & 1u) && sub == SAM_LANES - 1u)
        sam_store1(rec, H + NBe, room, (bam_codes4(seq[rev ? 0u : L - 1u], rev) & 0xfu) << 4);
    } else if (sub < NB) {  // fewer than 32 bases (33 with the half byte): a byte per lane
      const uint32_t i0 = 2u * sub, i1 = i0 + 1u;
      const uint32_t c0 = bam_codes4(seq[rev ? L - 1u - i0 : i0], rev) & 0xfu;
      const uint32_t c1 = i1 < L ? bam_codes4(seq[rev ? L - 1u - i1 : i1], rev) & 0xfu : 0u;
      sam_store1(rec, H + sub, room, (c0 << 4) | c1);
    }
    // ---- qual
    const uint8_t* qual = rd.qual + R.qb;
    if (L >= 16u) {
      const uint32_t nw = (L + 15u) >> 4;
      for (uint32_t g = sub; g < nw; g += SAM_LANES) {
        const uint32_t k = 16u * g + 16u <= L ? 16u * g : L - 16u;
        v4u32 q = __builtin_nontemporal_load((global_v4u32_unaligned_ptr)(qual + (rev ? L - 16u - k : k)));
        if (rev) q = sam_reverse16(q);
        sam_store16(rec, H + NB + k, room, v4u32{bam_quals4(q.x), bam_quals4(q.y), bam_quals4(q.z), bam_quals4(q.w)});
      }
    } else if (sub < L) {
      sam_store1(rec, H + NB + (rev ? L - 1u - sub : sub), room, bam_quals4(qual[sub]) & 0xffu);
    }
  }
  // ---- MD: tokens j = 0 .. n in forward-strand order (the SAM writer's), the last one ending in NUL
  uint32_t cursor = 0;
  for (uint32_t j0 = 0; j0 <= n; j0 += SAM_LANES) {  // (uniform over the row)
    const uint32_t j = j0 + sub;
    uint32_t tl = 0;
    uint64_t tok = 0;
    if (j <= n) {
      int32_t p = (int32_t)L, pp = -1;
      uint32_t c = 0u;
      bool ok = true;
      if (j < n) {
        const uint64_t at = R.e0 + (rev ? n - 1u - j : j);
        const uint32_t x = ed.pos[at];
        ok = x < L;
        p = (int32_t)(rev ? L - 1u - x : x);
        if (WRITE) c = sam_base1(ed.ref[at], rev);
      }
      if (j > 0u) {
        const uint32_t x = ed.pos[R.e0 + (rev ? n - j : j - 1u)];
        ok = ok && x < L;
        pp = (int32_t)(rev ? L - 1u - x : x);
      }
      ok = ok && p > pp;
      if (ok) {
        const uint32_t gap = (uint32_t)(p - pp - 1), ng = dec_digits(gap);
        tl = ng + 1u;
        if (WRITE) tok = (fq_eight_digits(gap) >> (8u * (8u - ng))) | ((uint64_t)c << (8u * ng));
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

// the record policy of record_stream.hpp; no LDS: a record's pieces are made in registers
struct BamRec {
  static constexpr uint32_t SLOT_BYTES = 0u;
  SIMMR_DEV static uint32_t size(const SamReads& rd, const SamEdits& ed, const SamNames& nm, uint64_t r, uint64_t n_reads, uint32_t paired,
                                 uint32_t sub, uint32_t* __restrict__ err) {
    return bam_record<false>(rd, ed, nm, r, r, n_reads, paired, sub, nullptr, nullptr, err);
  }
  SIMMR_DEV static void write(const SamReads& rd, const SamEdits& ed, const SamNames& nm, uint64_t r, uint64_t place, uint64_t n_reads,
                              uint32_t paired, uint32_t sub, uint8_t*, const uint64_t* __restrict__ off, uint8_t* __restrict__ dst,
                              uint32_t* __restrict__ err) {
    (void)bam_record<true>(rd, ed, nm, r, place, n_reads, paired, sub, off, dst, err);
  }
};

// BAM_ROUTINES_ONLY: the routines without the five kernels, for bam_index_kernels.hip (the sorted writer and the index)
#ifndef BAM_ROUTINES_ONLY
// ---- sizes ----------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
k_bam_size(const SamReads rd, const SamEdits ed, const SamNames nm, uint64_t n_reads, uint32_t paired, uint32_t* __restrict__ len,
           uint64_t* __restrict__ chunk_sum, uint32_t* __restrict__ err) {
  __shared__ uint32_t part[SAM_WG_READS];
  rec_size_chunks<BamRec>(rd, ed, nm, n_reads, paired, len, chunk_sum, err, part);
}

extern "C" __global__ void __launch_bounds__(256)
k_bam_scan(const uint64_t* __restrict__ sum, uint64_t* __restrict__ prefix, uint64_t n) {
  __shared__ uint64_t lds[256];
  sam_scan_chunks(sum, prefix, n, lds);
}

extern "C" __global__ void __launch_bounds__(256)
k_bam_offsets(const uint32_t* __restrict__ len, const uint64_t* __restrict__ prefix, uint64_t n_reads, uint64_t* __restrict__ off) {
  __shared__ uint32_t lds[256];
  sam_chunk_offsets(len, prefix, n_reads, off, lds);
}

// ---- the records ------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
k_bam_write(const SamReads rd, const SamEdits ed, const SamNames nm, uint64_t n_reads, uint32_t paired, const uint64_t* __restrict__ off,
            uint8_t* __restrict__ dst, uint32_t* __restrict__ err) {
  rec_write_places<BamRec, false>(rd, ed, nm, n_reads, paired, nullptr, off, dst, err, nullptr);
}
#endif  // BAM_ROUTINES_ONLY

// ---- BGZF -------------------------------------------------------------------------------------------------------------
struct BgzfTables {            // device memory, made on the host (bgzf_tables.hpp)
  const uint32_t* crc;         // [4][256]: crc[k][b] = the register after byte b and k zero bytes, from 0
  const uint32_t* seg_mul;     // [BGZF_LANES - 1]: seg_mul[j] = x^(8 BGZF_SEG j) mod P
  const uint32_t* rem_mul;     // [BGZF_SEG]: rem_mul[k] = x^(8 k) mod P
};

// a(x) b(x) mod P, bit-reflected: bit 31 is x^0 (zlib's multmodp, without its early exit)
SIMMR_DEV uint32_t bgzf_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 4
  for (uint32_t i = 0; i < 32u; i++) {
    p ^= (a & (0x80000000u >> i)) ? b : 0u;
    b = (b >> 1) ^ ((b & 1u) ? BGZF_POLY : 0u);
  }
  return p;
}
SIMMR_DEV uint32_t bgzf_crc_word(const uint32_t* t, uint32_t c, uint32_t w) {
  c ^= w;
  return t[768u + (c & 0xffu)] ^ t[512u + ((c >> 8) & 0xffu)] ^ t[256u + ((c >> 16) & 0xffu)] ^ t[c >> 24];
}

#ifndef BAM_ROUTINES_ONLY
extern "C" __global__ void __launch_bounds__(BGZF_LANES)
k_bgzf_frame(const uint8_t* __restrict__ src, uint64_t n_bytes, uint8_t* __restrict__ dst, const BgzfTables tb) {
  __shared__ uint32_t table[4u * 256u];
  __shared__ uint32_t fold[BGZF_LANES];
  __shared__ uint32_t last_crc;
  const uint32_t t = threadIdx.x;
  for (uint32_t i = t; i < 4u * 256u; i += BGZF_LANES) table[i] = tb.crc[i];
  __syncthreads();
  const uint64_t n_blocks = (n_bytes + BGZF_BLOCK - 1u) / BGZF_BLOCK;
  for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {  // (uniform over the workgroup)
    const uint64_t s0 = blk * BGZF_BLOCK;
    const uint32_t n = (uint32_t)(n_bytes - s0 < BGZF_BLOCK ? n_bytes - s0 : BGZF_BLOCK);  // 1 .. BGZF_BLOCK
    const uint32_t n_full = n / BGZF_SEG, rem = n % BGZF_SEG;                               // whole segments, and the bytes behind them
    uint8_t* out = dst + blk * (uint64_t)(BGZF_BLOCK + BGZF_OVERHEAD);
    // ---- the 23 bytes before the payload, a byte per lane
    if (t < BGZF_HEAD) {
      const uint32_t bsize = n + BGZF_OVERHEAD - 1u;
      uint32_t b = 0u;
      if (t == 0u) b = 0x1fu; else if (t == 1u) b = 0x8bu; else if (t == 2u) b = 8u; else if (t == 3u) b = 4u;
      else if (t == 9u) b = 0xffu; else if (t == 10u) b = 6u; else if (t == 12u) b = 'B'; else if (t == 13u) b = 'C'; else if (t == 14u) b = 2u;
      else if (t == 16u) b = bsize & 0xffu; else if (t == 17u) b = bsize >> 8;
      else if (t == 18u) b = 1u;  // BFINAL, BTYPE 00: stored
      else if (t == 19u) b = n & 0xffu; else if (t == 20u) b = n >> 8;
      else if (t == 21u) b = ~n & 0xffu; else if (t == 22u) b = (~n >> 8) & 0xffu;
      out[t] = (uint8_t)b;
    }
    // ---- this lane's segment: copy and CRC
    const uint32_t seg0 = t * BGZF_SEG;
    const uint32_t mine = seg0 >= n ? 0u : (n - seg0 < BGZF_SEG ? n - seg0 : BGZF_SEG);
    const uint8_t* sp = src + s0 + seg0;
    uint8_t* dp = out + BGZF_HEAD + seg0;
    uint32_t c = t == 0u ? 0xffffffffu : 0u;
    uint32_t i = 0;
    for (; i + 16u <= mine; i += 16u) {
      const v4u32 v = __builtin_nontemporal_load((global_v4u32_unaligned_ptr)(sp + i));
      *reinterpret_cast<v4u32_unaligned*>(dp + i) = v;
      c = bgzf_crc_word(table, c, v.x);
      c = bgzf_crc_word(table, c, v.y);
      c = bgzf_crc_word(table, c, v.z);
      c = bgzf_crc_word(table, c, v.w);
    }
    for (; i < mine; i++) {
      const uint32_t b = sp[i];
      dp[i] = (uint8_t)b;
      c = table[(c ^ b) & 0xffu] ^ (c >> 8);
    }
    // ---- fold: whole segment i has n_full - 1 - i whole segments behind it (and then rem bytes, applied to the sum)
    fold[t] = t < n_full ? bgzf_mulmod(tb.seg_mul[n_full - 1u - t], c) : 0u;
    if (t == n_full) last_crc = c;  // the lane of the rem bytes; with rem == 0 its register is untouched (0, or the start value of an empty lane 0: never, n >= 1)
    __syncthreads();
    for (uint32_t d = BGZF_LANES / 2u; d > 0u; d >>= 1) {
      if (t < d) fold[t] ^= fold[t + d];
      __syncthreads();
    }
    if (t == 0u) {
      uint32_t crc = fold[0];
      if (rem) crc = bgzf_mulmod(tb.rem_mul[rem], crc) ^ last_crc;
      crc = ~crc;
      u32_unaligned* foot = reinterpret_cast<u32_unaligned*>(out + BGZF_HEAD + n);
      foot[0] = crc;
      foot[1] = n;
    }
    __syncthreads();  // fold[] and last_crc are the next block's
  }
}
#endif  // BAM_ROUTINES_ONLY

}  // namespace simmr
