// host_support.hpp — the host plumbing every translation unit of libsimmr_hip.so shares (engine.hip included): the owning
// device buffer, the check of a HIP call, the synchronisation check, an owning set of events, the spans that time a unit's calls, the
// accessor of a unit's state in its engine slot, and the dense table of the staged rows.  Host code only; internal to the library, and each unit that includes
// it gets its own copy of the routines.  Whatever owns device memory or events here frees them in its destructor: a state is a
// struct of such members and needs no destroy code of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "engine_internal.hpp"

// returns eng_fail's SIMMR_ENODEV from the calling function when `call` fails; the message names the call as it is written
#define HIP_TRY(e, call)                                                                    \
  do {                                                                                      \
    hipError_t _s = (call);                                                                 \
    if (_s != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "%s failed: %s", #call, hipGetErrorString(_s)); \
  } while (0)

namespace simmr {
namespace {

// A device buffer that grows on demand and is freed with its owner.  It moves and does not copy.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;  // bytes
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p; cap = o.cap;
      o.p = nullptr; o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  // Room for `bytes`.  A buffer that has to grow is freed (what it held is gone) and allocated anew with `want` bytes; a failed
  // allocation leaves it empty and no HIP error pending.
  bool ensure(size_t bytes, size_t want) {
    if (bytes <= cap) return true;
    release();
    if (hipMalloc(&p, want) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; }
    cap = want;
    return true;
  }
  bool ensure(size_t bytes) { return ensure(bytes, bytes); }
  // the engine's buffers, which are asked for a little more shard after shard: an eighth and 256 bytes of slack
  bool ensure_slack(size_t bytes) { return ensure(bytes, bytes + bytes / 8 + 256); }
  // Room for `bytes` in a column that is appended to: a buffer that has to grow gets half as much again, and the first `keep`
  // bytes of what it held are copied over on `st` (the free of the old one waits for the work enqueued on it, the copy included).
  bool grow_keep(size_t bytes, size_t keep, hipStream_t st) {
    if (bytes <= cap) return true;
    DevBuf nb;
    if (!nb.ensure(bytes, bytes + bytes / 2)) return false;
    if (p && keep > 0 && hipMemcpyAsync(nb.p, p, std::min(keep, cap), hipMemcpyDeviceToDevice, st) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    *this = std::move(nb);
    return true;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <class T> T* as() const { return (T*)p; }
};

// N events (begin / end pairs of a unit's calls), made on first use and destroyed with their owner
template <int N> struct Events {
  hipEvent_t v[N] = {};
  Events() = default;
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  Events(Events&& o) noexcept {
    for (int i = 0; i < N; i++) { v[i] = o.v[i]; o.v[i] = nullptr; }
  }
  ~Events() {
    for (hipEvent_t ev : v)
      if (ev) (void)hipEventDestroy(ev);
  }
  hipEvent_t& operator[](size_t i) { return v[i]; }
  hipEvent_t operator[](size_t i) const { return v[i]; }
  int create_missing(simmr_engine* e) {
    for (hipEvent_t& ev : v)
      if (!ev) HIP_TRY(e, hipEventCreate(&ev));
    return SIMMR_OK;
  }
};

inline int sync_check(simmr_engine* e, const char* what) {
  hipError_t s = hipStreamSynchronize(eng_stream(e));
  if (s == hipSuccess) s = hipGetLastError();
  if (s != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "%s: %s", what, hipGetErrorString(s));
  return SIMMR_OK;
}

// The device time of a unit's calls: N spans (pair i: events 2i and 2i + 1 around what call i enqueues) and which of them
// count.  Recording an event marks nothing: a unit marks a span where its call has succeeded and unmarks the spans a new
// call makes stale; total_ms adds up the marked ones.
template <int N> struct Spans {
  Events<2 * N> ev;
  bool valid[N] = {};
  int create_missing(simmr_engine* e) { return ev.create_missing(e); }
  hipError_t begin(int i, hipStream_t st) { return hipEventRecord(ev[2 * i], st); }
  hipError_t end(int i, hipStream_t st) { return hipEventRecord(ev[2 * i + 1], st); }
  void mark(int i, bool on = true) { valid[i] = on; }
  void invalidate_from(int i) {
    for (; i < N; i++) valid[i] = false;
  }
  int total_ms(simmr_engine* e, const char* what, float* ms) const {
    if (int rc = sync_check(e, what)) return rc;
    float sum = 0.f;
    for (int i = 0; i < N; i++) {
      float one = 0.f;
      if (valid[i]) HIP_TRY(e, hipEventElapsedTime(&one, ev[2 * i], ev[2 * i + 1]));
      sum += one;
    }
    *ms = sum;
    return SIMMR_OK;
  }
};

// The state of type T that a unit keeps in its slot W of the engine (nullptr: none yet and `create` is false).
// simmr_engine_destroy deletes it through the hook given here; T's members free what they own.
template <class T, EngExt W> T* unit_state(simmr_engine* e, bool create) {
  void** slot = eng_ext_slot(e, W, [](void* q) { delete static_cast<T*>(q); });
  if (!*slot && create) *slot = new T();
  return static_cast<T*>(*slot);
}

// The staged contigs as dense rows, in the order of the genome slots: per slot its first row and its contigs (0: not staged),
// per row its staged length and, with `origin`, its slot and contig; first[r] is the position of row r's first base when the
// rows lie back to back (n_rows + 1 entries).
struct StagedRows {
  std::vector<uint32_t> cbase, ncontig, genome, contig;
  std::vector<uint64_t> bases, first;
  uint64_t longest = 0;
  uint32_t n_slots() const { return (uint32_t)cbase.size(); }
  uint64_t n_rows() const { return bases.size(); }
};
inline StagedRows staged_rows(const simmr_engine* e, bool origin = false) {
  StagedRows r;
  const uint32_t n_slots = eng_genome_slots(e);
  r.cbase.assign(n_slots, 0u);
  r.ncontig.assign(n_slots, 0u);
  r.first.assign(1, 0ull);
  for (uint32_t g = 0; g < n_slots; g++) {
    const uint32_t nc = eng_contig_count(e, g);
    r.cbase[g] = (uint32_t)r.bases.size();
    r.ncontig[g] = nc;
    for (uint32_t c = 0; c < nc; c++) {
      r.bases.push_back(eng_contig_len(e, g, c));
      r.first.push_back(r.first.back() + r.bases.back());
      r.longest = std::max(r.longest, r.bases.back());
      if (origin) { r.genome.push_back(g); r.contig.push_back(c); }
    }
  }
  return r;
}

}  // namespace
}  // namespace simmr
