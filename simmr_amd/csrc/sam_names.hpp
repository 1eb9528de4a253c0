// sam_names.hpp — what the units over the read columns share on the host beyond host_support.hpp: the names of a plan —
// per engine genome slot its rows, per row its RNAME in a blob (SamNames, sam_kernels.hip) and, for the sorted form's bound
// check, the row's staged length.  record_stream_host.hpp builds the record writers' plan and emit on it.  Internal to the
// library; each unit that includes it gets its own copy of the routines.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "host_support.hpp"

namespace simmr {
namespace {

// SAM's RNAME: [0-9A-Za-z!#$%&+./:;?@^_|~-][0-9A-Za-z!#$%&*+./:;=?@^_|~-]*
inline bool rname_legal(const char* s, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const unsigned char c = (unsigned char)s[i];
    const bool alnum = (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z');
    if (alnum || (c != 0 && std::strchr("!#$%&+./:;?@^_|~-", c))) continue;
    if (i > 0 && (c == '*' || c == '=')) continue;
    return false;
  }
  return true;
}

struct SamNameTable {
  DevBuf blob, g_cbase, g_ncontig, c_off, c_len, c_bases;
  uint32_t n_slots = 0;
  // the host copies: the uploads read them until the plan call has synchronised, whichever way it leaves
  std::vector<uint32_t> h_cbase, h_ncontig, h_off, h_len;
  std::vector<uint64_t> h_bases;  // staged length of every row (eng_contig_len)
  std::vector<uint8_t> h_blob;
  uint64_t n_rows = 0, longest = 0;  // of the names given (before the padding row of an empty set)

  SamNames names() const {
    return SamNames{blob.as<const uint8_t>(), g_cbase.as<const uint32_t>(), g_ncontig.as<const uint32_t>(), c_off.as<const uint32_t>(),
                    c_len.as<const uint32_t>(), n_slots};
  }
  // A row per contig of every entry, the RNAMEs back to back, into the host copies.  The caller has synchronised the stream.
  int build(simmr_engine* e, const simmr_sam_names* names) {
    const StagedRows staged = staged_rows(e);
    n_slots = staged.n_slots();
    h_cbase.assign(std::max(n_slots, 1u), 0u);
    h_ncontig.assign(std::max(n_slots, 1u), 0u);
    h_off.clear(); h_len.clear(); h_blob.clear(); h_bases.clear();
    longest = 0;
    size_t flat = 0;
    for (uint32_t i = 0; i < names->n_genomes; i++) {
      const uint32_t g = names->genome_idx[i], nc = names->n_contigs[i];
      if (g >= n_slots || staged.ncontig[g] == 0 || staged.ncontig[g] != nc)
        return eng_fail(e, SIMMR_EINVAL, "names entry %u: genome slot %u is not staged, or it does not have %u contigs", i, g, nc);
      h_cbase[g] = (uint32_t)h_off.size();
      h_ncontig[g] = nc;
      for (uint32_t c = 0; c < nc; c++, flat++) {
        const char* s = names->rname[flat];
        const size_t n = s ? std::strlen(s) : 0;
        if (n == 0 || n > SAM_RNAME_MAX)
          return eng_fail(e, SIMMR_ENOTSUP, "RNAME of contig %u of names entry %u is empty or longer than %u bytes", c, i, SAM_RNAME_MAX);
        if (!rname_legal(s, n)) return eng_fail(e, SIMMR_ENOTSUP, "RNAME '%s' (contig %u of names entry %u) is not a SAM reference name", s, c, i);
        h_off.push_back((uint32_t)h_blob.size());
        h_len.push_back((uint32_t)n);
        h_bases.push_back(staged.bases[staged.cbase[g] + c]);
        longest = std::max(longest, h_bases.back());
        h_blob.insert(h_blob.end(), s, s + n);
      }
    }
    n_rows = h_off.size();
    h_blob.resize(h_blob.size() + 8, 0);
    if (h_off.empty()) { h_off.push_back(0); h_len.push_back(0); h_bases.push_back(0); }
    return SIMMR_OK;
  }
  bool ensure(bool with_bases) {
    return blob.ensure(h_blob.size()) && g_cbase.ensure(h_cbase.size() * 4) && g_ncontig.ensure(h_ncontig.size() * 4) &&
           c_off.ensure(h_off.size() * 4) && c_len.ensure(h_len.size() * 4) && (!with_bases || c_bases.ensure(h_bases.size() * 8));
  }
  hipError_t upload(hipStream_t st, bool with_bases) {
    hipError_t s = hipMemcpyAsync(blob.p, h_blob.data(), h_blob.size(), hipMemcpyHostToDevice, st);
    if (s == hipSuccess) s = hipMemcpyAsync(g_cbase.p, h_cbase.data(), h_cbase.size() * 4, hipMemcpyHostToDevice, st);
    if (s == hipSuccess) s = hipMemcpyAsync(g_ncontig.p, h_ncontig.data(), h_ncontig.size() * 4, hipMemcpyHostToDevice, st);
    if (s == hipSuccess) s = hipMemcpyAsync(c_off.p, h_off.data(), h_off.size() * 4, hipMemcpyHostToDevice, st);
    if (s == hipSuccess) s = hipMemcpyAsync(c_len.p, h_len.data(), h_len.size() * 4, hipMemcpyHostToDevice, st);
    if (s == hipSuccess && with_bases) s = hipMemcpyAsync(c_bases.p, h_bases.data(), h_bases.size() * 8, hipMemcpyHostToDevice, st);
    return s;
  }
};

// field by field into zeroed memory: the emit calls compare these structs with the plan's as bytes
inline void assign_reads(SamReads* o, const simmr_reads_out* r) {
  o->seq = r->seq; o->qual = r->qual; o->seq_off = r->seq_off; o->start = r->start; o->end = r->end; o->contig = r->contig;
  o->genome = r->genome; o->read_id = r->read_id; o->flags = r->flags; o->seq_capacity = r->seq_capacity;
  o->slot16 = r->slot_bytes == SIMMR_SLOT16 ? 1u : 0u;
}
inline void assign_edits(SamEdits* o, const simmr_truth_out* t) {
  o->off = t->edit_off; o->pos = t->edit_pos; o->ref = t->edit_ref; o->capacity = t->edits_capacity;
}
inline SamReads sam_reads(const simmr_reads_out* r) {
  SamReads o;
  std::memset(&o, 0, sizeof o);
  assign_reads(&o, r);
  return o;
}
inline SamEdits sam_edits(const simmr_truth_out* t) {
  SamEdits o;
  std::memset(&o, 0, sizeof o);
  assign_edits(&o, t);
  return o;
}

inline int check_columns(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* truth, const char* who) {
  if (!reads->seq_off || !reads->start || !reads->end || !reads->contig || !reads->genome || !reads->read_id || !reads->flags ||
      !reads->seq || !reads->qual)
    return eng_fail(e, SIMMR_EINVAL, "%s needs every column of simmr_reads_out, read_id included", who);
  if (!truth->edit_off || !truth->edit_pos || !truth->edit_ref)
    return eng_fail(e, SIMMR_EINVAL, "%s needs edit_off, edit_pos and edit_ref of simmr_truth_out", who);
  return SIMMR_OK;
}

// the argument checks of a plan call that need no device (simmr_sam_plan, simmr_sam_sort_plan)
inline int check_plan_args(simmr_engine* e, const simmr_sam_names* names, const simmr_reads_out* reads, const simmr_truth_out* truth,
                           uint64_t n_reads, int paired, const uint64_t* total_bytes, const char* who) {
  if (!names || !reads || !truth || !total_bytes) return eng_fail(e, SIMMR_EINVAL, "%s: NULL argument", who);
  if (int rc = check_columns(e, reads, truth, who)) return rc;
  if (reads->slot_bytes > 1u && reads->slot_bytes != SIMMR_SLOT16) return eng_fail(e, SIMMR_EINVAL, "reads->slot_bytes is 0 (compact) or 16");
  if (reads->qual_offset != 33u) return eng_fail(e, SIMMR_EINVAL, "%s needs qualities emitted with qual_offset 33", who);
  if (paired && (n_reads & 1u)) return eng_fail(e, SIMMR_EINVAL, "%s: paired with an odd number of reads", who);
  if (n_reads >= (1ull << 31)) return eng_fail(e, SIMMR_ERANGE, "%s takes fewer than 2^31 reads a call", who);
  if (names->n_genomes > 0 && (!names->genome_idx || !names->n_contigs || !names->rname))
    return eng_fail(e, SIMMR_EINVAL, "%s: NULL names column", who);
  return SIMMR_OK;
}

}  // namespace
}  // namespace simmr
