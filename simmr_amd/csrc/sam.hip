// sam.hip — the true alignments as SAM text (include/simmr_hip.h: simmr_sam_*): the entry points over sam_kernels.hip.
// The sixth translation unit of libsimmr_hip.so; it sees an engine through engine_internal.hpp only — the device, the
// stream, which slots are staged and the staging epoch: the pass reads the caller's columns, never the genome planes —
// and keeps its state in the engine's opaque slot (freed by simmr_engine_destroy through the hook given there).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "sam_kernels.hip"
#include "engine_internal.hpp"

using namespace simmr;

namespace {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;  // bytes
  bool ensure(size_t bytes) {
    if (bytes <= cap) return true;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; }
    cap = bytes;
    return true;
  }
  template <class T> T* as() const { return (T*)p; }
};

struct SamState {
  // the names of the last plan: per engine genome slot its rows, per row its RNAME in the blob
  DevBuf blob, g_cbase, g_ncontig, c_off, c_len;
  uint32_t n_slots = 0;
  DevBuf len, off, chunk_sum, chunk_prefix;
  DevBuf word;  // the total (64 bits), then the error word
  // their host copies: the uploads read them until the plan call has synchronised, whichever way it leaves
  std::vector<uint32_t> h_cbase, h_ncontig, h_off, h_len;
  std::vector<uint8_t> h_blob;
  // what the plan was made for: every column and both capacities, as the kernels read them
  SamReads reads{};
  SamEdits edits{};
  uint32_t paired = 0;
  uint64_t n_reads = 0, total = 0, epoch = 0;
  bool ready = false, planned_once = false, emitted = false;
  hipEvent_t ev[4] = {};

  SamNames names() const {
    return SamNames{blob.as<const uint8_t>(), g_cbase.as<const uint32_t>(), g_ncontig.as<const uint32_t>(), c_off.as<const uint32_t>(),
                    c_len.as<const uint32_t>(), n_slots};
  }
  uint32_t* err_p() const { return (uint32_t*)(word.as<char>() + 8); }
};

void sam_destroy(void* q) {
  SamState* s = (SamState*)q;
  for (DevBuf* b : {&s->blob, &s->g_cbase, &s->g_ncontig, &s->c_off, &s->c_len, &s->len, &s->off, &s->chunk_sum, &s->chunk_prefix, &s->word})
    if (b->p) (void)hipFree(b->p);
  for (hipEvent_t ev : s->ev)
    if (ev) (void)hipEventDestroy(ev);
  delete s;
}

SamState* state_of(simmr_engine* e, bool create) {
  void** slot = eng_ext_slot(e, ENG_EXT_SAM, sam_destroy);
  if (!*slot && create) *slot = new SamState();
  return (SamState*)*slot;
}

#define SAM_TRY(e, call)                                                                    \
  do {                                                                                      \
    hipError_t _s = (call);                                                                 \
    if (_s != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "%s failed: %s", #call, hipGetErrorString(_s)); \
  } while (0)

int sync_check(simmr_engine* e, const char* what) {
  hipError_t s = hipStreamSynchronize(eng_stream(e));
  if (s == hipSuccess) s = hipGetLastError();
  if (s != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "%s: %s", what, hipGetErrorString(s));
  return SIMMR_OK;
}

// SAM's RNAME: [0-9A-Za-z!#$%&+./:;?@^_|~-][0-9A-Za-z!#$%&*+./:;=?@^_|~-]*
bool rname_legal(const char* s, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const unsigned char c = (unsigned char)s[i];
    const bool alnum = (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z');
    if (alnum || (c != 0 && std::strchr("!#$%&+./:;?@^_|~-", c))) continue;
    if (i > 0 && (c == '*' || c == '=')) continue;
    return false;
  }
  return true;
}

// field by field into zeroed memory: simmr_sam_emit compares these structs with the plan's as bytes
void assign_reads(SamReads* o, const simmr_reads_out* r) {
  o->seq = r->seq; o->qual = r->qual; o->seq_off = r->seq_off; o->start = r->start; o->end = r->end; o->contig = r->contig;
  o->genome = r->genome; o->read_id = r->read_id; o->flags = r->flags; o->seq_capacity = r->seq_capacity;
  o->slot16 = r->slot_bytes == SIMMR_SLOT16 ? 1u : 0u;
}
void assign_edits(SamEdits* o, const simmr_truth_out* t) {
  o->off = t->edit_off; o->pos = t->edit_pos; o->ref = t->edit_ref; o->capacity = t->edits_capacity;
}
SamReads sam_reads(const simmr_reads_out* r) {
  SamReads o;
  std::memset(&o, 0, sizeof o);
  assign_reads(&o, r);
  return o;
}
SamEdits sam_edits(const simmr_truth_out* t) {
  SamEdits o;
  std::memset(&o, 0, sizeof o);
  assign_edits(&o, t);
  return o;
}

int check_columns(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* truth, const char* who) {
  if (!reads->seq_off || !reads->start || !reads->end || !reads->contig || !reads->genome || !reads->read_id || !reads->flags ||
      !reads->seq || !reads->qual)
    return eng_fail(e, SIMMR_EINVAL, "%s needs every column of simmr_reads_out, read_id included", who);
  if (!truth->edit_off || !truth->edit_pos || !truth->edit_ref)
    return eng_fail(e, SIMMR_EINVAL, "%s needs edit_off, edit_pos and edit_ref of simmr_truth_out", who);
  return SIMMR_OK;
}

}  // namespace

extern "C" {

int simmr_sam_plan(simmr_engine* e, const simmr_sam_names* names, const simmr_reads_out* reads, const simmr_truth_out* truth,
                   uint64_t n_reads, int paired, uint64_t* total_bytes) {
  if (!e) return SIMMR_EINVAL;
  if (SamState* old = state_of(e, false)) old->ready = old->emitted = false;
  if (!names || !reads || !truth || !total_bytes) return eng_fail(e, SIMMR_EINVAL, "simmr_sam_plan: NULL argument");
  if (int rc = check_columns(e, reads, truth, "simmr_sam_plan")) return rc;
  if (reads->slot_bytes > 1u && reads->slot_bytes != SIMMR_SLOT16) return eng_fail(e, SIMMR_EINVAL, "reads->slot_bytes is 0 (compact) or 16");
  if (reads->qual_offset != 33u) return eng_fail(e, SIMMR_EINVAL, "simmr_sam_plan needs qualities emitted with qual_offset 33");
  if (paired && (n_reads & 1u)) return eng_fail(e, SIMMR_EINVAL, "simmr_sam_plan: paired with an odd number of reads");
  if (n_reads >= (1ull << 31)) return eng_fail(e, SIMMR_ERANGE, "simmr_sam_plan takes fewer than 2^31 reads a call");
  if (names->n_genomes > 0 && (!names->genome_idx || !names->n_contigs || !names->rname))
    return eng_fail(e, SIMMR_EINVAL, "simmr_sam_plan: NULL names column");
  // ---- the names: a row per contig of every entry, the RNAMEs back to back
  const uint32_t n_slots = eng_genome_slots(e);
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  SamState* s = state_of(e, true);
  if (int rc = sync_check(e, "SAM plan")) return rc;  // (an upload of an earlier plan that failed may still read the vectors)
  std::vector<uint32_t>&g_cbase = s->h_cbase, &g_ncontig = s->h_ncontig, &c_off = s->h_off, &c_len = s->h_len;
  std::vector<uint8_t>& blob = s->h_blob;
  g_cbase.assign(std::max(n_slots, 1u), 0u);
  g_ncontig.assign(std::max(n_slots, 1u), 0u);
  c_off.clear(); c_len.clear(); blob.clear();
  size_t flat = 0;
  for (uint32_t i = 0; i < names->n_genomes; i++) {
    const uint32_t g = names->genome_idx[i], nc = names->n_contigs[i];
    if (g >= n_slots || eng_contig_count(e, g) == 0 || eng_contig_count(e, g) != nc)
      return eng_fail(e, SIMMR_EINVAL, "names entry %u: genome slot %u is not staged, or it does not have %u contigs", i, g, nc);
    g_cbase[g] = (uint32_t)c_off.size();
    g_ncontig[g] = nc;
    for (uint32_t c = 0; c < nc; c++, flat++) {
      const char* s = names->rname[flat];
      const size_t n = s ? std::strlen(s) : 0;
      if (n == 0 || n > SAM_RNAME_MAX)
        return eng_fail(e, SIMMR_ENOTSUP, "RNAME of contig %u of names entry %u is empty or longer than %u bytes", c, i, SAM_RNAME_MAX);
      if (!rname_legal(s, n)) return eng_fail(e, SIMMR_ENOTSUP, "RNAME '%s' (contig %u of names entry %u) is not a SAM reference name", s, c, i);
      c_off.push_back((uint32_t)blob.size());
      c_len.push_back((uint32_t)n);
      blob.insert(blob.end(), s, s + n);
    }
  }
  blob.resize(blob.size() + 8, 0);
  if (c_off.empty()) { c_off.push_back(0); c_len.push_back(0); }
  for (hipEvent_t& ev : s->ev)
    if (!ev) SAM_TRY(e, hipEventCreate(&ev));
  const uint64_t n_chunks = (n_reads + SAM_CHUNK - 1) / SAM_CHUNK;
  if (!s->blob.ensure(blob.size()) || !s->g_cbase.ensure(g_cbase.size() * 4) || !s->g_ncontig.ensure(g_ncontig.size() * 4) ||
      !s->c_off.ensure(c_off.size() * 4) || !s->c_len.ensure(c_len.size() * 4) || !s->len.ensure(std::max<uint64_t>(n_reads, 1) * 4) ||
      !s->off.ensure((n_reads + 1) * 8) || !s->chunk_sum.ensure(std::max<uint64_t>(n_chunks, 1) * 8) ||
      !s->chunk_prefix.ensure((n_chunks + 1) * 8) || !s->word.ensure(16))
    return eng_fail(e, SIMMR_ENOMEM, "SAM plan allocation failed (%llu reads)", (unsigned long long)n_reads);
  hipStream_t st = eng_stream(e);
  SAM_TRY(e, hipMemcpyAsync(s->blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
  SAM_TRY(e, hipMemcpyAsync(s->g_cbase.p, g_cbase.data(), g_cbase.size() * 4, hipMemcpyHostToDevice, st));
  SAM_TRY(e, hipMemcpyAsync(s->g_ncontig.p, g_ncontig.data(), g_ncontig.size() * 4, hipMemcpyHostToDevice, st));
  SAM_TRY(e, hipMemcpyAsync(s->c_off.p, c_off.data(), c_off.size() * 4, hipMemcpyHostToDevice, st));
  SAM_TRY(e, hipMemcpyAsync(s->c_len.p, c_len.data(), c_len.size() * 4, hipMemcpyHostToDevice, st));
  SAM_TRY(e, hipMemsetAsync(s->word.p, 0, 16, st));
  s->n_slots = n_slots;
  SAM_TRY(e, hipEventRecord(s->ev[0], st));
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_chunks, (uint64_t)eng_cu_count(e) * SAM_WGS_PER_CU));
  if (n_reads > 0)
    hipLaunchKernelGGL(k_sam_size, dim3(grid), dim3(256), 0, st, sam_reads(reads), sam_edits(truth), s->names(), n_reads, paired ? 1u : 0u,
                       s->len.as<uint32_t>(), s->chunk_sum.as<uint64_t>(), s->err_p());
  hipLaunchKernelGGL(k_sam_scan, dim3(1), dim3(256), 0, st, s->chunk_sum.as<const uint64_t>(), s->chunk_prefix.as<uint64_t>(), n_chunks);
  hipLaunchKernelGGL(k_sam_offsets, dim3(grid), dim3(256), 0, st, s->len.as<const uint32_t>(), s->chunk_prefix.as<const uint64_t>(), n_reads,
                     s->off.as<uint64_t>());
  SAM_TRY(e, hipEventRecord(s->ev[1], st));
  uint64_t total = 0;
  uint32_t errw = 0;
  SAM_TRY(e, hipMemcpyAsync(&total, s->off.as<uint64_t>() + n_reads, 8, hipMemcpyDeviceToHost, st));
  SAM_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "SAM size pass")) return rc;
  s->planned_once = true;
  if (errw)
    return eng_fail(e, SIMMR_EINVAL, "a read's genome / contig has no name, its bytes leave seq[], it is longer than %u bases, its edit_off "
                                     "decreases or leaves edits_capacity, or its edit_pos do not ascend inside the read", SAM_MAX_L);
  s->reads = sam_reads(reads);
  s->edits = sam_edits(truth);
  s->paired = paired ? 1u : 0u;
  s->n_reads = n_reads;
  s->total = total;
  s->epoch = eng_staging_epoch(e);
  s->ready = true;
  *total_bytes = total;
  return SIMMR_OK;
}

int simmr_sam_emit(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* truth, uint8_t* dst, uint64_t dst_capacity) {
  if (!e) return SIMMR_EINVAL;
  if (!reads || !truth) return eng_fail(e, SIMMR_EINVAL, "simmr_sam_emit: NULL argument");
  SamState* s = state_of(e, false);
  if (s) s->emitted = false;
  SamReads now_r{};  // (zeroed first: the structs are compared as bytes, padding included)
  SamEdits now_e{};
  std::memset(&now_r, 0, sizeof now_r);
  std::memset(&now_e, 0, sizeof now_e);
  assign_reads(&now_r, reads);
  assign_edits(&now_e, truth);
  if (!s || !s->ready || std::memcmp(&now_r, &s->reads, sizeof now_r) != 0 || std::memcmp(&now_e, &s->edits, sizeof now_e) != 0)
    return eng_fail(e, SIMMR_ESTATE, "simmr_sam_emit called without a simmr_sam_plan for these columns");
  if (s->epoch != eng_staging_epoch(e)) return eng_fail(e, SIMMR_ESTATE, "a genome was staged since simmr_sam_plan: plan again");
  if (int rc = check_columns(e, reads, truth, "simmr_sam_emit")) return rc;
  if (dst_capacity < s->total)
    return eng_fail(e, SIMMR_ERANGE, "dst_capacity %llu < %llu bytes planned", (unsigned long long)dst_capacity, (unsigned long long)s->total);
  if (s->total > 0 && !dst) return eng_fail(e, SIMMR_EINVAL, "simmr_sam_emit: NULL dst");
  SAM_TRY(e, hipSetDevice(eng_device(e)));
  hipStream_t st = eng_stream(e);
  SAM_TRY(e, hipEventRecord(s->ev[2], st));
  if (s->n_reads > 0) {
    const uint64_t n_batches = (s->n_reads + SAM_WG_READS - 1) / SAM_WG_READS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_batches, (uint64_t)eng_cu_count(e) * SAM_WGS_PER_CU);
    hipLaunchKernelGGL(k_sam_write, dim3(grid), dim3(256), 0, st, s->reads, s->edits, s->names(), s->n_reads, s->paired,
                       s->off.as<const uint64_t>(), dst, s->err_p());
  }
  SAM_TRY(e, hipEventRecord(s->ev[3], st));
  uint32_t errw = 0;
  SAM_TRY(e, hipMemcpyAsync(&errw, s->err_p(), 4, hipMemcpyDeviceToHost, st));
  if (int rc = sync_check(e, "SAM write pass")) return rc;
  s->emitted = true;
  if (errw) {
    s->ready = false;
    return eng_fail(e, SIMMR_EINVAL, "the columns changed since simmr_sam_plan: a read failed the bounds check of the write pass (no store "
                                     "left its record)");
  }
  return SIMMR_OK;
}

int simmr_last_sam_ms(simmr_engine* e, float* ms) {
  if (!e || !ms) return SIMMR_EINVAL;
  SamState* s = state_of(e, false);
  if (!s || !s->planned_once) return eng_fail(e, SIMMR_ESTATE, "no simmr_sam_plan yet");
  if (int rc = sync_check(e, "sam")) return rc;
  float a = 0.f, b = 0.f;
  SAM_TRY(e, hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
  if (s->emitted) SAM_TRY(e, hipEventElapsedTime(&b, s->ev[2], s->ev[3]));
  *ms = a + b;
  return SIMMR_OK;
}

}  // extern "C"
