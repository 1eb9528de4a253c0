// scorer_host.hpp — the host scaffold of the scorer units (mapeval, ovleval, vcfeval, taxeval, asmeval, bineval, correval,
// asmmap): the bit length and the grid of a launch, the checks of an add's text, the spans of a scorer folded into a sum, the
// create and destroy of a scorer's object, the sorted name table of a reset, the line index of an add and the pair sort.  What
// launches or hands out a kernel's argument (LineIndex::enqueue, PairSort::sort, DeviceNames::names) is there behind
// mapeval_kernels.hip alone (#ifdef MEV_WG: MevText, MevNames, FSAM_WG), which every scorer's kernels include; sam_sort.hip and
// bam_index.hip take the rest without it.  Host code only; internal to the library, and each unit that includes it gets its own
// copy, as with host_support.hpp.  Plain structs and functions: a unit calls what it takes.
#pragma once
#include <algorithm>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "host_support.hpp"

namespace simmr {
namespace {

inline uint32_t bits_of(uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }

// the workgroups of a launch over `items`, `per_wg` of them a workgroup: at least one, at most `most`
inline uint32_t grid_capped(uint64_t items, uint32_t per_wg, uint64_t most) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + per_wg - 1) / per_wg, most));
}
// ... at most wgs_per_cu a CU: beyond them the workgroups loop
inline uint32_t grid_for(simmr_engine* e, uint64_t items, uint32_t per_wg, uint32_t wgs_per_cu) {
  return grid_capped(items, per_wg, (uint64_t)std::max(eng_cu_count(e), 1) * wgs_per_cu);
}

// a column with room for `want` entries of `width` bytes; what it held stays and the new part is zero
inline bool grow_zero(DevBuf* b, uint64_t want, uint64_t held, uint32_t width, hipStream_t st) {
  if (!b->grow_keep(want * width, held * width, st)) return false;
  return hipMemsetAsync((uint8_t*)b->p + held * width, 0, (want - held) * width, st) == hipSuccess;
}

// what every add checks of its text, in this order: a reset has been, the text is there, it is not too long
inline int check_add_text(simmr_engine* e, bool reset_once, const uint8_t* text, uint64_t n_bytes, uint64_t max_bytes, const char* who,
                          const char* reset_name, const char* cut_hint) {
  if (!reset_once) return eng_fail(e, SIMMR_ESTATE, "%s called before %s", who, reset_name);
  if (!text && n_bytes > 0) return eng_fail(e, SIMMR_EINVAL, "%s: NULL text", who);
  if (n_bytes > max_bytes)
    return eng_fail(e, SIMMR_ENOTSUP, "%s: %llu bytes in one add (at most %llu: %s)", who, (unsigned long long)n_bytes, (unsigned long long)max_bytes,
                    cut_hint);
  return SIMMR_OK;
}

// The device time of a scorer: N spans folded into a sum.  Span 0 is the adds': the adds of either side only enqueue, so the first
// begins it and every one ends it anew, and a run of adds is one span.  A call that synchronises anyway (a plan, a read, last_ms)
// folds the spans that count into the sum and closes them, so no stretch of the stream is counted twice.
template <int N> struct FoldedSpans {
  Spans<N> sp;
  bool open = false;  // the span of the adds has begun and is not folded yet
  float done_ms = 0.f;

  int reset(simmr_engine* e) {
    sp.invalidate_from(0);
    open = false;
    done_ms = 0.f;
    return sp.create_missing(e);
  }
  // the span `which` runs from here, unless it is the adds' and open already
  int begin(simmr_engine* e, int which, hipStream_t st) {
    if (which == 0 && open) return SIMMR_OK;
    HIP_TRY(e, sp.begin(which, st));
    return SIMMR_OK;
  }
  // ... and ends behind what was enqueued; a launch that failed leaves the span as it was
  int end(simmr_engine* e, int which, hipStream_t st, const char* what) {
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return eng_fail(e, SIMMR_ENODEV, "%s launch failed: %s", what, hipGetErrorString(rc));
    HIP_TRY(e, sp.end(which, st));
    if (which == 0) open = true;
    sp.mark(which);
    return SIMMR_OK;
  }
  // the spans that count into the sum, and closed.  Synchronises.
  int fold(simmr_engine* e, const char* label) {
    float now = 0.f;
    if (int rc = sp.total_ms(e, label, &now)) return rc;
    done_ms += now;
    sp.invalidate_from(0);
    open = false;
    return SIMMR_OK;
  }
  int last_ms(simmr_engine* e, const char* label, float* ms) {
    if (int rc = fold(e, label)) return rc;  // (the next add of either side begins a new span)
    *ms = done_ms;
    return SIMMR_OK;
  }
};

// A scorer's object T (a member `e`), which the caller creates on an engine and destroys before the engine: the engine's slot
// enum is full.  T's members free what they own.
template <class T> int scorer_create(simmr_engine* e, T** out, const char* who) {
  if (!e) return SIMMR_EINVAL;
  if (!out) return eng_fail(e, SIMMR_EINVAL, "%s: NULL out", who);
  *out = nullptr;
  T* h = new (std::nothrow) T();
  if (!h) return eng_fail(e, SIMMR_ENOMEM, "%s: out of memory", who);
  h->e = e;
  *out = h;
  return SIMMR_OK;
}
template <class T> void scorer_destroy(T* h) {
  if (!h) return;
  if (hipSetDevice(eng_device(h->e)) == hipSuccess) (void)hipStreamSynchronize(eng_stream(h->e));
  delete h;  // (its buffers and events go with it)
  (void)hipGetLastError();
}

// The name table of a reset on the host: the n names sorted bytewise as unsigned bytes (a prefix before the longer name, as
// mev_compare orders them), back to back in a blob with eight zero bytes behind them, off[i] .. off[i + 1] the bytes of sorted
// name i, and order[i] its place among the names given.
struct SortedNames {
  std::vector<uint8_t> blob;
  std::vector<uint32_t> off, order;
};
// `label`: what a name is called in a refusal; `legal`: the names the unit takes, `illegal`: what follows the label and the place
// of a name it does not take ("... %u <illegal>"), or nullptr for "'<name>' (<label> %u) is not a SAM reference name".
inline int sorted_names(simmr_engine* e, const char* const* names, uint32_t n, uint32_t max_len, bool (*legal)(const char*, size_t), const char* label,
                        const char* illegal, SortedNames* out) {
  std::vector<std::string> given;
  given.reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    const char* s = names[i];
    const size_t len = s ? std::strlen(s) : 0;
    if (len == 0 || len > max_len) return eng_fail(e, SIMMR_ENOTSUP, "%s %u is empty or longer than %u bytes", label, i, max_len);
    if (!legal(s, len))
      return illegal ? eng_fail(e, SIMMR_ENOTSUP, "%s %u %s", label, i, illegal)
                     : eng_fail(e, SIMMR_ENOTSUP, "'%s' (%s %u) is not a SAM reference name", s, label, i);
    given.emplace_back(s, len);
  }
  out->order.resize(n);
  std::iota(out->order.begin(), out->order.end(), 0u);
  std::sort(out->order.begin(), out->order.end(), [&](uint32_t a, uint32_t b) {
    return std::lexicographical_compare(given[a].begin(), given[a].end(), given[b].begin(), given[b].end(),
                                        [](char x, char y) { return (unsigned char)x < (unsigned char)y; });
  });
  for (uint32_t i = 1; i < n; i++)
    if (given[out->order[i]] == given[out->order[i - 1]]) return eng_fail(e, SIMMR_EINVAL, "%s '%s' is given twice", label, given[out->order[i]].c_str());
  std::vector<uint8_t>& blob = out->blob;
  blob.clear();
  out->off.assign(1, 0u);
  for (uint32_t i = 0; i < n; i++) {
    const std::string& s = given[out->order[i]];
    blob.insert(blob.end(), s.begin(), s.end());
    out->off.push_back((uint32_t)blob.size());
  }
  blob.resize(blob.size() + 8, 0);  // (what a reader of eight bytes at a name's end runs into)
  return SIMMR_OK;
}

// ... and on the device.  The uploads read the host vectors: they live until the reset has synchronised.
struct DeviceNames {
  DevBuf blob, name_off;
  bool room(const SortedNames& s) { return blob.ensure(s.blob.size()) && name_off.ensure(s.off.size() * 4); }
  int upload(simmr_engine* e, const SortedNames& s, hipStream_t st) {
    HIP_TRY(e, hipMemcpyAsync(blob.p, s.blob.data(), s.blob.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(e, hipMemcpyAsync(name_off.p, s.off.data(), s.off.size() * 4, hipMemcpyHostToDevice, st));
    return SIMMR_OK;
  }
#ifdef MEV_WG
  // the first n of them: the unit keeps the count, which holds where its reset has succeeded
  MevNames names(uint32_t n) const { return MevNames{blob.as<const uint8_t>(), name_off.as<const uint32_t>(), n}; }
#endif
};

// The buffers of a pair sort (the ping and the pong of keys and indexes, the histograms) over samsort_sort_pairs.  The unit writes
// the n keys into key[0] between room and sort.
struct PairSort {
  DevBuf key[2], idx[2], hist, digit_total;
  struct Sorted {
    const uint64_t* keys;
    const uint32_t* perm;  // nullptr where no bit was sorted over: the order is the identity and no index was written
  };
  bool room(uint64_t n) {
    const uint64_t n_tiles = std::max<uint64_t>((n + SAMSORT_PAIRS_TILE - 1) / SAMSORT_PAIRS_TILE, 1);
    return key[0].ensure(n * 8) && key[1].ensure(n * 8) && idx[0].ensure(n * 4) && idx[1].ensure(n * 4) &&
           hist.ensure(n_tiles * SAMSORT_PAIRS_DIGITS * 4) && digit_total.ensure(SAMSORT_PAIRS_DIGITS * 4);
  }
#ifdef MEV_WG
  Sorted sort(hipStream_t st, uint64_t n, uint32_t bits) {
    uint64_t* const keys[2] = {key[0].as<uint64_t>(), key[1].as<uint64_t>()};
    uint32_t* const idxs[2] = {idx[0].as<uint32_t>(), idx[1].as<uint32_t>()};
    const int cur = samsort_sort_pairs(st, keys, idxs, hist.as<uint32_t>(), digit_total.as<uint32_t>(), n, bits);
    return Sorted{keys[cur], bits > 0u ? idxs[cur] : nullptr};
  }
#endif
};

// The line index of one add: the sums and the prefixes of the tiles and the line starts, through the unit's own two kernels.
struct LineIndex {
  DevBuf tile_sum, tile_prefix, starts;
  bool room(uint64_t n_tiles, uint64_t start_cap) { return tile_sum.ensure(n_tiles * 8) && tile_prefix.ensure((n_tiles + 1) * 8) && starts.ensure(start_cap * 4); }
#ifdef MEV_WG
  using IndexKernel = void (*)(const uint8_t*, uint64_t, uint64_t, uint64_t*, const uint64_t*, uint32_t*, uint64_t);
  using ScanKernel = void (*)(const uint64_t*, uint64_t*, uint64_t);
  // count -> scan -> write over text[0, n_bytes) (n_bytes > 0) in tiles of `tile` bytes, into buffers with room(n_tiles, start_cap)
  void enqueue(hipStream_t st, IndexKernel index_kernel, ScanKernel scan_kernel, const uint8_t* text, uint64_t n_bytes, uint32_t tile, uint32_t tile_grid,
               uint64_t start_cap, MevText* W) {
    const uint64_t n_tiles = (n_bytes + tile - 1) / tile;
    uint64_t* const sum = tile_sum.as<uint64_t>();
    uint64_t* const prefix = tile_prefix.as<uint64_t>();
    hipLaunchKernelGGL(index_kernel, dim3(tile_grid), dim3(FSAM_WG), 0, st, text, n_bytes, n_tiles, sum, (const uint64_t*)nullptr, (uint32_t*)nullptr, 0ull);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(256), 0, st, (const uint64_t*)sum, prefix, n_tiles);
    hipLaunchKernelGGL(index_kernel, dim3(tile_grid), dim3(FSAM_WG), 0, st, text, n_bytes, n_tiles, sum, (const uint64_t*)prefix, starts.as<uint32_t>(), start_cap);
    *W = MevText{text, n_bytes, (const uint64_t*)prefix + n_tiles, starts.as<const uint32_t>()};
  }
#endif
};

}  // namespace
}  // namespace simmr
