// asmeval_front.hpp — the text-to-planes stage of a FASTA add, shared by asmeval.hip and asmmap.hip: the line index, the lines,
// the planes (k_asm_index / k_asm_scan / k_asm_lines / k_asm_chunks / k_asm_pack) and the genome of every truth record
// (k_asm_genomes).  The kernels live in asmeval.hip's translation unit alone; a second unit reaches them through the two launchers
// declared here, which asmeval.hip defines, and owns the buffers of its own front (AsmFront: host code, a copy per unit, as
// everything of host_support.hpp).  Internal to the library.  Include behind asmeval_kernels.hip (AsmLines, AsmPlane, MevText,
// MevNames, FSAM_TILE, ASM_*).
#pragma once
#include "host_support.hpp"

namespace simmr {

// where the front's sums go: words of a unit's 64-bit counts, and the bit of its error word that a malformed text sets
struct AsmFrontSums {
  unsigned long long* counts;
  uint32_t records_at, bases_at, invalid_at;
  uint32_t* err;
  uint32_t err_bit;
};

struct AsmFrontBufs {  // the device pointers of one AsmFront
  uint64_t *tile_sum, *tile_prefix, *chunk_sum, *chunk_prefix, *code;
  uint32_t *starts, *valid;
  AsmLines lines;
};

// index (count) -> scan -> index (write) -> lines (count) -> chunks -> lines (write) -> pack for text[0, n_bytes), n_bytes > 0,
// into buffers sized by AsmFront::ensure(n_bytes).  Only enqueues.
SIMMR_HIDDEN void asm_front_launch(simmr_engine* e, hipStream_t st, const uint8_t* text, uint64_t n_bytes, const AsmFrontBufs& B, const AsmFrontSums& S, MevText* W);
// rec_row[r] = the genome row of record r of the add (n_bytes / 2 + 1 entries of room); a header that names none sets ASM_ERR_TRUTH in *err
SIMMR_HIDDEN void asm_front_genomes(simmr_engine* e, hipStream_t st, const MevText& W, const AsmLines& L, const MevNames& N, uint32_t* rec_row, uint32_t* err);

namespace {

// the buffers of one add's front, everything sized from n_bytes: a line per two bytes, a record per line, a base per byte
struct AsmFront {
  DevBuf tile_sum, tile_prefix, starts, chunk_sum, chunk_prefix, line_base, rec_start, rec_hdr, tot, code, valid;
  bool ensure(uint64_t n_bytes) {
    const uint64_t n_tiles = (n_bytes + FSAM_TILE - 1) / FSAM_TILE, line_cap = n_bytes / 2 + 1, chunk_cap = line_cap / ASM_CHUNK + 1;
    const uint64_t word_cap = n_bytes / ASM_WORD + 1;
    return tile_sum.ensure(n_tiles * 8) && tile_prefix.ensure((n_tiles + 1) * 8) && starts.ensure(line_cap * 4) && chunk_sum.ensure(chunk_cap * 8) &&
           chunk_prefix.ensure((chunk_cap + 1) * 8) && line_base.ensure((line_cap + 1) * 4) && rec_start.ensure((line_cap + 1) * 4) &&
           rec_hdr.ensure(line_cap * 4) && tot.ensure(16) && code.ensure(word_cap * 8) && valid.ensure(word_cap * 4);
  }
  AsmLines lines() const { return AsmLines{line_base.as<uint32_t>(), rec_start.as<uint32_t>(), rec_hdr.as<uint32_t>(), tot.as<uint32_t>()}; }
  AsmPlane plane() const { return AsmPlane{code.as<const uint64_t>(), valid.as<const uint32_t>(), rec_start.as<const uint32_t>(), tot.as<const uint32_t>()}; }
  AsmFrontBufs bufs() const {
    return AsmFrontBufs{tile_sum.as<uint64_t>(), tile_prefix.as<uint64_t>(), chunk_sum.as<uint64_t>(), chunk_prefix.as<uint64_t>(), code.as<uint64_t>(),
                        starts.as<uint32_t>(), valid.as<uint32_t>(), lines()};
  }
};

}  // namespace
}  // namespace simmr
