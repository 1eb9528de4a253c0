// fit_device.hpp — what the two model-fitting units share on the device: the tables' layout, the class codes and the pair
// table's insert.  Plain device routines and constants, no kernel: fit_kernels.hip (the columns of a run) and
// fit_sam_kernels.hip (SAM text) both add into one FitTables, each from a translation unit of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simmr_hip.h"
#include "read_walk.hpp"

namespace simmr {

#define FIT_LANES 16u            /* lanes per read: one DPP row */
#define FIT_WG 512u              /* threads per workgroup of k_fit_add */
#define FIT_WG_READS 32u         /* reads per workgroup and batch */
#define FIT_FLUSH_BATCHES 512u   /* a workgroup adds its LDS tables to HBM after this many batches */
#define FIT_MAX_L 65535u         /* longest read taken */
#define FIT_Q_STRIDE 96u         /* LDS words per offset of the quality table */
#define FIT_LDS_POS 160u         /* offsets whose quality counts are privatised in LDS */
#define FIT_LDS_LEN 1024u        /* lengths and inserts below this are privatised in LDS */
#define FIT_LDS_K 7u             /* largest k whose dense table is privatised in LDS */
#define FIT_DENSE_LDS 16384u     /* 4^FIT_LDS_K */
#define FIT_MAX_PROBE 256u       /* slots an insert looks at before the pair table counts as full */
#define FIT_LDS_WORDS (FIT_DENSE_LDS + FIT_LDS_POS * FIT_Q_STRIDE + 2u * FIT_LDS_LEN)
#define FIT_ERR_READ 1u          /* a read failed the walker's bounds check */
#define FIT_ERR_QUAL 2u          /* a quality above SIMMR_FIT_MAX_Q */
#define FIT_ERR_FULL 4u          /* the pair table is full */
#define FIT_ERR_SAM 8u           /* a malformed SAM record (simmr_fit_add_sam) */
#define FIT_DENSITY_WG 256u
#define FIT_EMPTY_KEY (~0ull)

static_assert(FIT_LDS_WORDS * 4u == 135168u && FIT_LDS_WORDS * 4u <= 163840u, "one workgroup per CU: the image fits the CU's 160 KB");
static_assert(2ull * FIT_MAX_L * FIT_WG_READS * FIT_FLUSH_BATCHES < (1ull << 32), "a 32-bit partial must not wrap");
static_assert(FIT_LANES * FIT_WG_READS == FIT_WG && SIMMR_FIT_MAX_Q < FIT_Q_STRIDE && FIT_DENSE_LDS == 1u << (2u * FIT_LDS_K), "");
static_assert(SIMMR_FIT_MAX_L == FIT_MAX_L, "the header states the kernel's bound");

struct FitTables {
  unsigned long long* dense;  // [4^k], by 2-bit code
  unsigned long long* hkey;   // [hmask + 1], FIT_EMPTY_KEY = free
  unsigned long long* hcnt;
  unsigned long long* qhist;  // [FIT_MAX_L][SIMMR_FIT_QUALS]
  unsigned long long* lhist;  // [FIT_MAX_L + 1]
  unsigned long long* ihist;  // [SIMMR_FIT_MAX_INSERT + 1]
  uint32_t* err;
  uint32_t hmask, k;
};

// A C G T -> 0 1 2 3; otherwise `gap` for 'N' and '-' and `other` for every other byte
SIMMR_DEV uint32_t fit_class(uint32_t x, uint32_t gap, uint32_t other) {
  const uint32_t d = x - 0x41u, c = (x >> 1) & 3u;  // (x >> 1) & 3: A 0, C 1, T 2, G 3
  if (d < 20u && ((0x80045u >> d) & 1u)) return c ^ (c >> 1);
  return (x == 'N' || x == '-') ? gap : other;
}
// byte B (a constant) of four words
#define FIT_BYTE(v, B) (((v)[(B) >> 2] >> (((B) & 3u) * 8u)) & 0xffu)

// count[ref][alt] += 1 for a changed window.  Linear probing from a multiplicative hash; a slot is claimed by the CAS that
// turns FIT_EMPTY_KEY into the key (keys never leave), and the count is added after the claim is seen.
SIMMR_DEV void fit_pair_add(const FitTables& T, uint64_t key) {
  uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & T.hmask;
  const uint32_t probes = T.hmask + 1u < FIT_MAX_PROBE ? T.hmask + 1u : FIT_MAX_PROBE;
  for (uint32_t p = 0; p < probes; p++, h = (h + 1u) & T.hmask) {
    unsigned long long cur = __hip_atomic_load(T.hkey + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == FIT_EMPTY_KEY) cur = atomicCAS(T.hkey + h, FIT_EMPTY_KEY, (unsigned long long)key);
    if (cur == FIT_EMPTY_KEY || cur == key) {
      atomicAdd(T.hcnt + h, 1ull);
      return;
    }
  }
  atomicOr(T.err, FIT_ERR_FULL);
}

// ---- what fit.hip lends fit_sam.hip (defined in fit.hip, hidden): the tables of the engine's fit state -------------------
#define FIT_SAM_COUNTS 15u  /* the entries of simmr_fit_sam_counts, in its order */
struct FitShare {
  FitTables T;
  unsigned long long* counts;  // [FIT_SAM_COUNTS], zeroed by simmr_fit_reset
  hipEvent_t ev[2];            // what simmr_last_fit_ms reads
};
// false: no simmr_fit_reset yet
__attribute__((visibility("hidden"))) bool fit_share(simmr_engine* e, FitShare* out);
// an add was enqueued: the plan is stale, the events are set
__attribute__((visibility("hidden"))) void fit_share_added(simmr_engine* e);

}  // namespace simmr
