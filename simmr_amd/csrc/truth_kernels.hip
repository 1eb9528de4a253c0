// truth_kernels.hip — ground truth per read (gfx950): which bases of an emitted read differ from the staged
// reference, as counts (nm) and as CSR edit lists.  Included by engine.hip; entry points simmr_truth_plan /
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
// The bounds check and the window loads are the read walker below (walk_open / walk_window), which k_read_stats
// (stats_kernels.hip, included after this file) uses too.
#pragma once

namespace simmr {

#define TRUTH_LANES 16u       /* lanes per read: one DPP row */
#define TRUTH_WG_READS 16u    /* reads per 256-thread workgroup and iteration */
#define TRUTH_WGS_PER_CU 64u  /* the grid is capped at this many workgroups per CU; beyond it workgroups loop */

struct TruthReads {
  const uint8_t* seq;
  const uint8_t* qual;
  const uint64_t* seq_off;
  const uint64_t* start;
  const uint64_t* end;
  const uint32_t* contig;
  const uint32_t* genome;
  const uint8_t* flags;
  uint64_t seq_capacity;
  uint32_t slot16;
};

struct TruthCols {
  uint32_t* pos;
  uint8_t* ref;
  uint8_t* alt;
  uint8_t* qual;
};

typedef const __attribute__((address_space(1))) v4u32_unaligned* global_v4u32_unaligned_ptr;

// bit i = byte i of x is not zero
SIMMR_DEV uint32_t truth_nonzero_bytes(uint32_t x) {
  const uint32_t t = ((x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u) >> 7;
  return (t | (t >> 7) | (t >> 14) | (t >> 21)) & 0xfu;
}
// byte b (0..15) of four words, without indexing registers by a lane value
SIMMR_DEV uint32_t truth_byte(const v4u32 v, uint32_t b) {
  const uint32_t lo = (b & 4u) ? v.y : v.x, hi = (b & 4u) ? v.w : v.z;
  return (((b & 8u) ? hi : lo) >> ((b & 3u) * 8u)) & 0xffu;
}

// ---- the read walker: shared by k_truth and k_read_stats (stats_kernels.hip) ----------------------------------------
// Sixteen lanes (one DPP row) share a read.  walk_open checks a row's read once, walk_window loads one lane's 16 bases
// of it; between them they hold every rule that keeps a load inside the read, so both kernels answer to one copy.

// A row's read, opened: L bases of seq[] from byte `so`; output byte k is the reference's pos0 + k (forward) or pos0 - k,
// complemented (reverse): gather_piece.  A refused read, and a row past n_reads, has L = 0 and good = false.
struct ReadWalk {
  uint32_t L, rev;
  uint64_t so;
  int64_t pos0;
  GenomeDev G;
  bool good;
};
// The bounds check: genome staged, contig in range, so <= so1 <= seq_capacity, len <= so1 - so and MAX_L, coordinates
// inside the contig.  Every lane of a row reads the same columns (one address per row) and so takes the same branch:
// all-or-nothing per row, which keeps the DPP rows whole.  A refused read raises the caller's `errbit` in the caller's
// error word `err`, through the one lane of its row that has `raise` set.  (The atomic sits where the read is refused:
// raised by the caller after the checks have joined again, both kernels measured slower.)
template <uint64_t MAX_L>
SIMMR_DEV ReadWalk walk_open(const GenomeDev* __restrict__ genomes, uint32_t n_genomes, const TruthReads& rd, uint64_t r,
                             uint64_t n_reads, uint32_t* __restrict__ err, uint32_t errbit, bool raise) {
  uint32_t L = 0, rev = 0;
  uint64_t so = 0;
  int64_t pos0 = 0;
  bool good = false;
  GenomeDev G{};
  if (r < n_reads) {
    const uint64_t a = rd.start[r], b = rd.end[r];
    const uint64_t lo = a < b ? a : b, len = a < b ? b - a : a - b;
    const uint32_t g = rd.genome[r], c = rd.contig[r];
    so = rd.seq_off[r];
    const uint64_t so1 = rd.seq_off[r + 1];
    rev = rd.flags[r] & SIMMR_FLAG_REVCOMP;
    bool ok = g < n_genomes && len <= MAX_L && so <= so1 && so1 <= rd.seq_capacity && len <= so1 - so;
    if (ok) {
      G = genomes[g];
      ok = G.packed != nullptr && c < G.n_contigs;
    }
    if (ok) {
      const ContigDev C = G.contigs[c];
      ok = lo <= C.len && len <= C.len - lo;
      L = (uint32_t)len;
      pos0 = (int64_t)(C.base + lo) + (rev ? (int64_t)len - 1 : 0);
    }
    good = ok;
    if (!ok) {
      L = 0;
      if (raise) atomicOr(err, errbit);
    }
  }
  return ReadWalk{L, rev, so, pos0, G, good};
}

// Group `grp` (< ceil(L / 16)) of an opened read: bit b of keep = byte b of the window is base k + b and belongs to this
// group; have / qv = the 16 bytes of seq[] / qual[] (qv only with QUAL), want = what the reference holds there, diff =
// the kept bytes where they differ.
struct ReadWindow {
  uint32_t k, keep, diff;
  v4u32 have, qv, want;
};
template <bool QUAL>
SIMMR_DEV ReadWindow walk_window(const ReadWalk& w, uint32_t grp, const uint8_t* seq, const uint8_t* qual) {
  ReadWindow o{};
  const uint32_t k16 = grp * 16u, L = w.L;
  if (L >= 16u) {
    o.k = k16 + 16u <= L ? k16 : L - 16u;         // the last window ends at the read's end
    o.keep = (0xffffu << (k16 - o.k)) & 0xffffu;  // ... and owns only the bases no earlier window had
    o.have = __builtin_nontemporal_load((global_v4u32_unaligned_ptr)(seq + o.k));
    if (QUAL) o.qv = __builtin_nontemporal_load((global_v4u32_unaligned_ptr)(qual + o.k));
  } else {
    uint32_t h[4] = {0u, 0u, 0u, 0u}, q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++)
      if (j < L) {
        h[j >> 2] |= (uint32_t)seq[j] << ((j & 3u) * 8u);
        if (QUAL) q[j >> 2] |= (uint32_t)qual[j] << ((j & 3u) * 8u);
      }
    o.have = v4u32{h[0], h[1], h[2], h[3]};
    o.qv = v4u32{q[0], q[1], q[2], q[3]};
    o.keep = (1u << L) - 1u;
  }
  uint32_t codes, exc;
  gather_piece(w.G, PieceSrc{w.pos0, w.rev}, o.k, codes, exc);
  o.want = v4u32{expand4(codes & 0xffu, exc & 0xfu), expand4((codes >> 8) & 0xffu, (exc >> 4) & 0xfu),
                 expand4((codes >> 16) & 0xffu, (exc >> 8) & 0xfu), expand4(codes >> 24, (exc >> 12) & 0xfu)};
  o.diff = (truth_nonzero_bytes(o.have.x ^ o.want.x) | truth_nonzero_bytes(o.have.y ^ o.want.y) << 4 |
            truth_nonzero_bytes(o.have.z ^ o.want.z) << 8 | truth_nonzero_bytes(o.have.w ^ o.want.w) << 12) & o.keep;
  return o;
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
