// truth_kernels.hip — ground truth per read (gfx950): which bases of an emitted read differ from the staged
// reference, as counts (nm) and as CSR edit lists.  Included by truth.hip; entry points simmr_truth_plan /
// simmr_truth_emit (include/simmr_hip.h states what an edit is).
//
// The pass is a DIFF of seq[] against the 2-bit planes, not a replay of the draws: it serves every profile, rng mode
// and layout, and bytes the caller changed after the emit.  One template, two instantiations:
//   k_truth<false>  counts the edits of every read (nm[r]); the engine's scan turns the counts into edit_off[];
//   k_truth<true>   finds the same edits again and writes them at edit_off[r] + their rank inside the read.
// No slot is handed out by an atomic: an edit's place is a function of the inputs alone.
//
// Work item: 16 bases.  TRUTH_LANES = 16 lanes (one DPP row) share a read; in round i lane s takes bases
// [16 (16 i + s), +16): a round covers 256 consecutive bases in lane order, so the rank of an edit is the round's
// running base + the row's exclusive prefix of popcounts (DPP row_shr, no LDS memory) + the bit's rank in its lane.  A long
// read (65 535 bases) is 256 rounds of its row, never one lane's loop over the whole read.
// The window of a lane is one unaligned 16-byte load of seq[] (nontemporal: every byte is read once per pass).  The last
// window of a read ends AT the read's end (it overlaps its neighbour; the overlapped bits are masked), so no load leaves
// the read in either layout — compact reads have no slack behind them, and the reverse mates of SIMMR_SLOT16 are
// right-aligned in their slots.  Reads shorter than 16 bases are loaded bytewise.
// The expected bytes come from gather_piece (the emit kernels' funnel-shift addressing and code-domain reverse
// complement) and expand4; the comparison is bytewise, so 'N' and '-' need no special case.
// The bounds check and the window loads are the read walker of read_walk.hpp (walk_open / walk_window), which k_read_stats
// (stats_kernels.hip, a unit of its own) and k_fit_add (fit_kernels.hip, a unit of its own) use too.
#pragma once

#include "read_walk.hpp"  // TruthReads and the read walker (walk_open / walk_window), shared with fit_kernels.hip

namespace simmr {

#define TRUTH_LANES 16u       /* lanes per read: one DPP row */
#define TRUTH_WG_READS 16u    /* reads per 256-thread workgroup and iteration */
#define TRUTH_WGS_PER_CU 64u  /* the grid is capped at this many workgroups per CU; beyond it workgroups loop */

struct TruthCols {
  uint32_t* pos;
  uint8_t* ref;
  uint8_t* alt;
  uint8_t* qual;
};

// byte b (0..15) of four words, without indexing registers by a lane value
SIMMR_DEV uint32_t truth_byte(const v4u32 v, uint32_t b) {
  const uint32_t lo = (b & 4u) ? v.y : v.x, hi = (b & 4u) ? v.w : v.z;
  return (((b & 8u) ? hi : lo) >> ((b & 3u) * 8u)) & 0xffu;
}

template <bool WRITE>
__global__ void __launch_bounds__(256)
k_truth(const GenomeDev* __restrict__ genomes, uint32_t n_genomes, TruthReads rd, uint64_t n_reads,
        uint32_t* __restrict__ nm, const uint64_t* __restrict__ edit_off, TruthCols out, uint32_t* __restrict__ err) {
  const uint32_t sub = threadIdx.x & (TRUTH_LANES - 1u), row = threadIdx.x / TRUTH_LANES;
  const uint64_t n_batches = (n_reads + TRUTH_WG_READS - 1u) / TRUTH_WG_READS;
  for (uint64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    const uint64_t r = batch * TRUTH_WG_READS + row;
    const ReadWalk w = walk_open<0xffffffffull>(genomes, n_genomes, rd, r, n_reads, err, SIMMR_ERRBIT_TRUTH, sub == 0);
    const uint32_t L = w.L;
    const uint64_t so = w.so;
    const uint8_t* seq = rd.seq + so;
    const uint32_t n_groups = (L + 15u) >> 4;
    uint64_t cursor = 0;  // WRITE: where the next edit of this round's first lane goes
    uint64_t qbase = 0, limit = 0;
    if (WRITE) {
      if (L) { cursor = edit_off[r]; limit = edit_off[r + 1]; }
      qbase = rd.slot16 ? (so & ~15ull) : so;
    }
    uint32_t count = 0;
    for (uint32_t g0 = 0; g0 < n_groups; g0 += TRUTH_LANES) {  // (uniform over the row)
      const uint32_t grp = g0 + sub;
      ReadWindow x{};
      if (grp < n_groups) x = walk_window<false>(w, grp, seq, nullptr);
      const uint32_t n = __builtin_popcount(x.diff);
      if (!WRITE) {
        count += n;
      } else {
        // inclusive scan over the row of 16 lanes (lanes without a group add 0)
        const uint32_t inc = row_inclusive_scan_u32(n);
        const uint32_t round_total = (uint32_t)__shfl((int)inc, (int)TRUTH_LANES - 1, (int)TRUTH_LANES);  // the row's last lane
        uint64_t o = cursor + (inc - n);
        // (o < limit: seq[] changed between the plan and this call must not carry a store past the read's own slots)
        for (uint32_t m = x.diff; m && o < limit; m &= m - 1u, o++) {
          const uint32_t bit = (uint32_t)__builtin_ctz(m);
          if (out.pos) out.pos[o] = x.k + bit;
          if (out.ref) out.ref[o] = (uint8_t)truth_byte(x.want, bit);
          if (out.alt) out.alt[o] = (uint8_t)truth_byte(x.have, bit);
          if (out.qual) out.qual[o] = rd.qual[qbase + x.k + bit];
        }
        cursor += round_total;
      }
    }
    if (!WRITE) {
      count = row_inclusive_scan_u32(count);  // the row's sum, kept by its last lane
      if (sub == TRUTH_LANES - 1u && r < n_reads) nm[r] = count;
    }
  }
}

}  // namespace simmr
