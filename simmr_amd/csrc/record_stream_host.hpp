// record_stream_host.hpp — the host side the four record writers share (sam.hip, sam_sort.hip, bam.hip, bam_index.hip): one
// state, one plan call, one emit call and one timer, over the kernels each unit names.  Internal to the library; each unit that
// includes it (behind its kernels' file: the constants of sam_kernels.hip are used here) gets its own copy of the routines.
//
// A unit gives a traits struct F (RecordFormat below states the usual answers):
//   F::SORTED, F::WITH_END        coordinate order (the sort and the gather sit between the sizes and the scan), and whether
//                                 the ends ride along for the index;
//   F::PLAN, F::EMIT              the names of the unit's calls, for messages;
//   F::NOUN                       what the unit writes, for the allocation message ("sorted BAM");
//   F::SYNC_PLAN, SYNC_SIZE, SYNC_WRITE, TIMER   what a failed synchronisation of each call is reported under;
//   F::PLAN_REFUSAL               the plan's refusal of a read, whole (one %u: the longest read);
//   F::check_names(e, nt)         the format's own limit on the names table;
//   F::engine(c), F::state(c, create)   the engine and the state behind the call's first argument (an engine, or a handle);
//   F::size / gather / scan / offsets / write   launch the unit's kernels of those names.
#pragma once
#include "sam_names.hpp"

namespace simmr {
namespace {

struct RecordStreamState {
  SamNameTable nt;  // the names of the last plan (sam_names.hpp)
  DevBuf len, off, chunk_sum, chunk_prefix;
  DevBuf word;  // the error word
  // the sorted forms: the pairs, ping and pong (behind the sort the free key buffer holds the canonical keys and the free
  // index buffer the sorted lengths), the sort's counters, and for the index the ends per read and in sorted order
  DevBuf key[2], idx[2], hist, digit_total, end, send;
  const uint32_t* perm = nullptr;  // place -> read (nullptr: the identity, a key without bits)
  const uint64_t* ckey = nullptr;  // the canonical key of every place
  // what the plan was made for: every column and both capacities, as the kernels read them
  SamReads reads{};
  SamEdits edits{};
  uint32_t paired = 0;
  uint64_t n_reads = 0, total = 0, epoch = 0;
  bool ready = false;
  Spans<2> sp;  // plan, emit

  uint32_t* err_p() const { return word.as<uint32_t>(); }
};

struct RecordFormat {  // a format in read order, without limits of its own, on an engine
  static constexpr bool SORTED = false, WITH_END = false;
  static int check_names(simmr_engine*, const SamNameTable&) { return SIMMR_OK; }
  static simmr_engine* engine(simmr_engine* e) { return e; }
};

template <class F, class Ctx>
int record_plan(Ctx* c, const simmr_sam_names* names, const simmr_reads_out* reads, const simmr_truth_out* truth, uint64_t n_reads, int paired,
                uint64_t* total_bytes) {
  if (!c) return SIMMR_EINVAL;
  simmr_engine* e = F::engine(c);
  if (RecordStreamState* old = F::state(c, false)) { old->ready = false; old->sp.invalidate_from(1); }
  if (int rc = check_plan_args(e, names, reads, truth, n_reads, paired, total_bytes, F::PLAN)) return rc;
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  RecordStreamState* s = F::state(c, true);
  if (int rc = sync_check(e, F::SYNC_PLAN)) return rc;  // (an upload of an earlier plan that failed may still read the host copies)
  // ---- the names: a row per contig of every entry, the RNAMEs back to back
  if (int rc = s->nt.build(e, names)) return rc;
  if (int rc = F::check_names(e, s->nt)) return rc;
  uint32_t pos_bits = 0, row_bits = 0;
  if constexpr (F::SORTED)
    if (simmr_sam_sort_key_bits(s->nt.n_rows, s->nt.longest, &pos_bits, &row_bits) != SIMMR_OK)
      return eng_fail(e, SIMMR_ERANGE, "%s: %llu named contigs, the longest of %llu bases: the key takes at most 2^24 contigs of fewer than 2^40 bases",
                      F::PLAN, (unsigned long long)s->nt.n_rows, (unsigned long long)s->nt.longest);
  [[maybe_unused]] const uint32_t key_bits = pos_bits + row_bits;
  if (int rc = s->sp.create_missing(e)) return rc;
  const uint64_t n_chunks = (n_reads + SAM_CHUNK - 1) / SAM_CHUNK;
  [[maybe_unused]] const uint64_t n_tiles = (n_reads + SAMSORT_PAIRS_TILE - 1) / SAMSORT_PAIRS_TILE;
  const uint64_t n1 = std::max<uint64_t>(n_reads, 1);
  bool fits = s->nt.ensure(F::SORTED) && s->len.ensure(n1 * 4) && s->off.ensure((n_reads + 1) * 8) && s->chunk_sum.ensure(std::max<uint64_t>(n_chunks, 1) * 8) &&
              s->chunk_prefix.ensure((n_chunks + 1) * 8) && s->word.ensure(16);
  if constexpr (F::SORTED)
    fits = fits && s->key[0].ensure(n1 * 8) && s->key[1].ensure(n1 * 8) && s->idx[0].ensure(n1 * 4) && s->idx[1].ensure(n1 * 4) &&
           s->hist.ensure(std::max<uint64_t>(n_tiles, 1) * SAMSORT_PAIRS_DIGITS * 4) && s->digit_total.ensure(SAMSORT_PAIRS_DIGITS * 4) &&
           (!F::WITH_END || (s->end.ensure(n1 * 4) && s->send.ensure(n1 * 4)));
  if (!fits) return eng_fail(e, SIMMR_ENOMEM, "%s plan allocation failed (%llu reads)", F::NOUN, (unsigned long long)n_reads);
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, s->nt.upload(st, F::SORTED));
  HIP_TRY(e, hipMemsetAsync(s->word.p, 0, 16, st));
  HIP_TRY(e, s->sp.begin(0, st));
  const SamReads rd = sam_reads(reads);
  const SamEdits ed = sam_edits(truth);
  const uint32_t pr = paired ? 1u : 0u;
  if constexpr (F::SORTED) {
    // a workgroup per chunk (fewer than 2^21 of them): of the sorted grids only the writer's is capped
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, n_chunks);
    if (n_reads > 0) {
      F::size(st, grid, *s, rd, ed, n_reads, pr, pos_bits);
      uint64_t* const keys[2] = {s->key[0].as<uint64_t>(), s->key[1].as<uint64_t>()};
      uint32_t* const idxs[2] = {s->idx[0].as<uint32_t>(), s->idx[1].as<uint32_t>()};
      const int cur = samsort_sort_pairs(st, keys, idxs, s->hist.as<uint32_t>(), s->digit_total.as<uint32_t>(), n_reads, key_bits);
      s->perm = key_bits > 0u ? s->idx[cur].as<const uint32_t>() : nullptr;
      s->ckey = s->key[cur ^ 1].as<const uint64_t>();
      F::gather(st, grid, *s, n_reads, pos_bits, cur);  // key[cur ^ 1]: the canonical keys, idx[cur ^ 1]: the sorted lengths
      F::scan(st, *s, n_chunks);
      F::offsets(st, grid, *s, s->idx[cur ^ 1].as<const uint32_t>(), n_reads);
    } else {
      HIP_TRY(e, hipMemsetAsync(s->off.p, 0, 8, st));
    }
  } else {
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_chunks, (uint64_t)eng_cu_count(e) * SAM_WGS_PER_CU));
    if (n_reads > 0) F::size(st, grid, *s, rd, ed, n_reads, pr, 0u);
    F::scan(st, *s, n_chunks);
    F::offsets(st, grid, *s, s->len.as<const uint32_t>(), n_reads);
  }
  HIP_TRY(e, s->sp.end(0, st));
  uint64_t total = 0;
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(&total, s->off.as<uint64_t>() + n_reads, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, F::SYNC_SIZE)) return rc;
  s->sp.mark(0);
  if (F::SORTED && (errw & 2u))
    return eng_fail(e, SIMMR_EINVAL, "a read's genome / contig has no name, or the read ends behind its contig's staged length");
  if (errw) return eng_fail(e, SIMMR_EINVAL, F::PLAN_REFUSAL, SAM_MAX_L);
  s->reads = rd;
  s->edits = ed;
  s->paired = pr;
  s->n_reads = n_reads;
  s->total = total;
  s->epoch = eng_staging_epoch(e);
  s->ready = true;
  *total_bytes = total;
  return SIMMR_OK;
}

// key_out, off_out, end_out: the sorted forms' optional outputs (device pointers; nullptr: not wanted)
template <class F, class Ctx>
int record_emit(Ctx* c, const simmr_reads_out* reads, const simmr_truth_out* truth, uint8_t* dst, uint64_t dst_capacity, uint64_t* key_out,
                uint64_t* off_out, uint32_t* end_out) {
  if (!c) return SIMMR_EINVAL;
  simmr_engine* e = F::engine(c);
  if (!reads || !truth) return eng_fail(e, SIMMR_EINVAL, "%s: NULL argument", F::EMIT);
  RecordStreamState* s = F::state(c, false);
  if (s) s->sp.invalidate_from(1);
  SamReads now_r;  // (zeroed first, then field by field: the structs are compared as bytes, padding included)
  SamEdits now_e;
  std::memset(&now_r, 0, sizeof now_r);
  std::memset(&now_e, 0, sizeof now_e);
  assign_reads(&now_r, reads);
  assign_edits(&now_e, truth);
  if (!s || !s->ready || std::memcmp(&now_r, &s->reads, sizeof now_r) != 0 || std::memcmp(&now_e, &s->edits, sizeof now_e) != 0)
    return eng_fail(e, SIMMR_ESTATE, "%s called without a %s for these columns", F::EMIT, F::PLAN);
  if (s->epoch != eng_staging_epoch(e)) return eng_fail(e, SIMMR_ESTATE, "a genome was staged since %s: plan again", F::PLAN);
  if (int rc = check_columns(e, reads, truth, F::EMIT)) return rc;
  if (dst_capacity < s->total)
    return eng_fail(e, SIMMR_ERANGE, "dst_capacity %llu < %llu bytes planned", (unsigned long long)dst_capacity, (unsigned long long)s->total);
  if (s->total > 0 && !dst) return eng_fail(e, SIMMR_EINVAL, "%s: NULL dst", F::EMIT);
  HIP_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  HIP_TRY(e, s->sp.begin(1, st));
  if (s->n_reads > 0) {
    const uint64_t n_batches = (s->n_reads + SAM_WG_READS - 1) / SAM_WG_READS;
    F::write(st, (uint32_t)std::min<uint64_t>(n_batches, (uint64_t)eng_cu_count(e) * SAM_WGS_PER_CU), *s, dst);
    if constexpr (F::SORTED) {
      if (key_out) HIP_TRY(e, hipMemcpyAsync(key_out, s->ckey, s->n_reads * 8, hipMemcpyDeviceToDevice, st));
      if (F::WITH_END && end_out) HIP_TRY(e, hipMemcpyAsync(end_out, s->send.p, s->n_reads * 4, hipMemcpyDeviceToDevice, st));
    }
  }
  if constexpr (F::SORTED)
    if (off_out) HIP_TRY(e, hipMemcpyAsync(off_out, s->off.p, (s->n_reads + 1) * 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(e, s->sp.end(1, st));
  uint32_t errw = 0;
  HIP_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, F::SYNC_WRITE)) return rc;
  s->sp.mark(1);
  if (errw) {
    s->ready = false;
    return eng_fail(e, SIMMR_EINVAL, "the columns changed since %s: a read failed the bounds check of the write pass (no store left its record)", F::PLAN);
  }
  return SIMMR_OK;
}

// the device time of the last plan, and of the emit behind it if there was one
template <class F, class Ctx>
int record_ms(Ctx* c, float* ms) {
  if (!c || !ms) return SIMMR_EINVAL;
  simmr_engine* e = F::engine(c);
  RecordStreamState* s = F::state(c, false);
  if (!s || !s->sp.valid[0]) return eng_fail(e, SIMMR_ESTATE, "no %s yet", F::PLAN);
  return s->sp.total_ms(e, F::TIMER, ms);
}

}  // namespace
}  // namespace simmr
