// host_support_main.cpp — simmr_amd/csrc/host_support.hpp and the parts of scorer_host.hpp that stand without a unit's kernels (everything
// but LineIndex::enqueue, PairSort::sort and DeviceNames::names) on a machine without a GPU: the HIP entry points and the engine
// accessors the headers use are counting stubs over malloc and free, with a switch that makes the next allocation (or event)
// fail.  Links no HIP library.  The exit status is the number of device allocations and events still alive at the end (0: every
// owner freed what it owned), or 101 when a check failed (the failed checks go to stderr).
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -fsanitize=address,undefined tests/host_support_main.cpp
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../simmr_amd/csrc/host_support.hpp"
#include "../simmr_amd/csrc/scorer_host.hpp"

// ---- the stubs -------------------------------------------------------------------------------------------------------
static long g_live_bufs = 0, g_live_events = 0, g_mallocs = 0, g_frees = 0, g_event_creates = 0, g_syncs = 0;
static bool g_fail_next_malloc = false, g_fail_next_event = false;
static hipError_t g_pending = hipSuccess;  // the sticky error hipGetLastError reads and clears
static size_t g_last_malloc_bytes = 0;
static std::map<hipEvent_t, float> g_span_ms;  // what hipEventElapsedTime answers for a pair, by its begin event
static std::vector<hipEvent_t> g_recorded;     // the events recorded, in order
static long g_elapsed_calls = 0;
static bool g_fail_next_elapsed = false;

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) {
  if (g_fail_next_malloc) {
    g_fail_next_malloc = false;
    *ptr = (void*)0x1;  // (a failed call may leave anything behind)
    return g_pending = hipErrorOutOfMemory;
  }
  *ptr = malloc(size ? size : 1);
  g_last_malloc_bytes = size;
  g_mallocs++;
  g_live_bufs++;
  return hipSuccess;
}
hipError_t hipFree(void* ptr) {
  if (ptr) { free(ptr); g_frees++; g_live_bufs--; }
  return hipSuccess;
}
hipError_t hipGetLastError(void) {
  const hipError_t s = g_pending;
  g_pending = hipSuccess;
  return s;
}
hipError_t hipEventCreate(hipEvent_t* event) {
  if (g_fail_next_event) { g_fail_next_event = false; return g_pending = hipErrorOutOfMemory; }
  *event = (hipEvent_t)malloc(1);
  g_event_creates++;
  g_live_events++;
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event) {
  free((void*)event);
  g_live_events--;
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { g_syncs++; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t event, hipStream_t) { g_recorded.push_back(event); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t start, hipEvent_t stop) {
  g_elapsed_calls++;
  if (g_fail_next_elapsed) { g_fail_next_elapsed = false; return hipErrorNotReady; }
  if (!start || !stop || !g_span_ms.count(start)) return hipErrorInvalidHandle;
  *ms = g_span_ms[start];
  return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) { memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) { memset(dst, value, bytes); return hipSuccess; }
const char* hipGetErrorString(hipError_t s) { return s == hipSuccess ? "no error" : "stub error"; }
}

struct simmr_engine {
  void* slot[simmr::ENG_EXT_COUNT] = {};
  void (*destroy[simmr::ENG_EXT_COUNT])(void*) = {};
  std::vector<std::vector<uint64_t>> genomes;  // per slot the lengths of its contigs (none: not staged)
  std::string err;
  int cus = 4;
};

namespace simmr {
hipStream_t eng_stream(const simmr_engine*) { return nullptr; }
int eng_device(const simmr_engine*) { return 0; }
int eng_cu_count(const simmr_engine* e) { return e->cus; }
uint32_t eng_genome_slots(const simmr_engine* e) { return (uint32_t)e->genomes.size(); }
uint32_t eng_contig_count(const simmr_engine* e, uint32_t slot) { return slot < e->genomes.size() ? (uint32_t)e->genomes[slot].size() : 0u; }
uint64_t eng_contig_len(const simmr_engine* e, uint32_t slot, uint32_t contig) { return e->genomes[slot][contig]; }
int eng_fail(simmr_engine* e, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  e->err = buf;
  return code;
}
void** eng_ext_slot(simmr_engine* e, EngExt which, void (*destroy)(void*)) {
  e->destroy[which] = destroy;
  return &e->slot[which];
}
}  // namespace simmr

using namespace simmr;

static int g_failed = 0;
#define CHECK(cond)                                                             \
  do {                                                                          \
    if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); g_failed++; } \
  } while (0)

static long live() { return g_live_bufs + g_live_events; }

// ---- the checks ------------------------------------------------------------------------------------------------------
static void ensure_keeps_grows_and_fails() {
  DevBuf b;
  CHECK(b.p == nullptr && b.cap == 0);
  CHECK(b.ensure(100) && b.p && b.cap == 100 && g_mallocs == 1);
  void* const first = b.p;
  CHECK(b.ensure(50) && b.ensure(100) && b.p == first && b.cap == 100 && g_mallocs == 1 && g_frees == 0);  // large enough: kept
  CHECK(b.ensure(101) && b.cap == 101 && g_mallocs == 2 && g_frees == 1 && g_live_bufs == 1);              // grows: freed, allocated anew
  CHECK(b.as<char>() == (char*)b.p);
  g_fail_next_malloc = true;
  CHECK(!b.ensure(400));
  CHECK(b.p == nullptr && b.cap == 0 && g_live_bufs == 0);
  CHECK(g_pending == hipSuccess);  // no error left for the next sync_check to report
  CHECK(b.ensure(8) && b.cap == 8);
  b.release();
  CHECK(b.p == nullptr && b.cap == 0 && g_live_bufs == 0);
  b.release();  // (twice is once)
  CHECK(g_live_bufs == 0);
}

static void growth_rules() {
  DevBuf b;
  CHECK(b.ensure_slack(0) && b.ensure(0) && b.p == nullptr && b.cap == 0);  // nothing asked, nothing allocated
  for (size_t bytes : {(size_t)1, (size_t)7, (size_t)1000, (size_t)65537}) {
    b.release();
    CHECK(b.ensure_slack(bytes) && b.cap == bytes + bytes / 8 + 256 && g_last_malloc_bytes == b.cap);
  }
  const long mallocs = g_mallocs;
  CHECK(b.ensure_slack(65537 + 65537 / 8 + 256) && g_mallocs == mallocs);  // the slack is room: kept
  CHECK(b.ensure_slack(65537 + 65537 / 8 + 257) && g_mallocs == mallocs + 1);
  DevBuf c;
  CHECK(c.ensure(100, 125) && c.cap == 125 && g_last_malloc_bytes == 125);  // a caller's own rule
  CHECK(c.ensure(125, 999) && c.cap == 125);
  DevBuf d;
  CHECK(d.ensure(64) && d.cap == 64 && g_last_malloc_bytes == 64);  // exactly what is asked
}

static void one_owner() {
  DevBuf a;
  CHECK(a.ensure(32));
  void* const pa = a.p;
  DevBuf b(std::move(a));
  CHECK(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 32 && g_live_bufs == 1);
  DevBuf c;
  CHECK(c.ensure(16));
  void* const pc = c.p;
  CHECK(g_live_bufs == 2);
  c = std::move(b);  // what c held is freed
  CHECK(b.p == nullptr && b.cap == 0 && c.p == pa && c.cap == 32 && g_live_bufs == 1);
  (void)pc;
  DevBuf& self = c;
  c = std::move(self);
  CHECK(c.p == pa && c.cap == 32 && g_live_bufs == 1);
  DevBuf d;
  CHECK(d.ensure(48));
  void* const pd = d.p;
  std::swap(c, d);
  CHECK(c.p == pd && c.cap == 48 && d.p == pa && d.cap == 32 && g_live_bufs == 2);
  static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "a DevBuf does not copy");
  static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_assignable<DevBuf>::value, "and moves without throwing");
}

struct Holder {  // as the engine's GenomeHost: buffers inside a vector's element
  int tag = 0;
  DevBuf x, y;
};

static void vector_of_holders() {
  const long before = g_live_bufs;
  {
    std::vector<Holder> v(2);
    for (int i = 0; i < 2; i++) { v[i].tag = i; CHECK(v[i].x.ensure(10 + i) && v[i].y.ensure(20 + i)); }
    void* const x1 = v[1].x.p;
    v.resize(40);  // reallocates: the elements move
    CHECK(g_live_bufs == before + 4 && v[1].x.p == x1 && v[1].tag == 1 && v[1].y.cap == 21 && v[39].x.p == nullptr);
    CHECK(v[39].x.ensure(5));
    v.erase(v.begin());  // every later element moves down by one; the first one's buffers are freed
    CHECK(g_live_bufs == before + 3 && v[0].tag == 1 && v[0].x.p == x1 && v[38].x.cap == 5);
    v.resize(1);
    CHECK(g_live_bufs == before + 2);
  }
  CHECK(g_live_bufs == before);
}

static void events_set(simmr_engine* e) {
  const long before = g_live_events;
  {
    Events<4> ev;
    CHECK(ev[0] == nullptr && ev[3] == nullptr);
    CHECK(hipEventCreate(&ev[1]) == hipSuccess);
    hipEvent_t const had = ev[1];
    const long creates = g_event_creates;
    CHECK(ev.create_missing(e) == SIMMR_OK && g_event_creates == creates + 3 && ev[1] == had && ev[0] && ev[2] && ev[3]);
    CHECK(ev.create_missing(e) == SIMMR_OK && g_event_creates == creates + 3);  // none is missing
    CHECK(g_live_events == before + 4);
    Events<2> two;
    g_fail_next_event = true;
    CHECK(two.create_missing(e) == SIMMR_ENODEV && e->err == "hipEventCreate(&ev) failed: stub error");
    (void)hipGetLastError();
    CHECK(two.create_missing(e) == SIMMR_OK && g_live_events == before + 6);
  }
  CHECK(g_live_events == before);
}

// Spans: only the marked pairs are read and summed; recording marks nothing; a failure is reported with the call's text
static void spans(simmr_engine* e) {
  const long before = g_live_events;
  {
    Spans<3> sp;
    CHECK(hipEventCreate(&sp.ev[3]) == hipSuccess);
    hipEvent_t const had = sp.ev[3];
    long creates = g_event_creates;
    g_fail_next_event = true;  // the first missing one cannot be made: reported, nothing made, the one that was there kept
    CHECK(sp.create_missing(e) == SIMMR_ENODEV && e->err == "hipEventCreate(&ev) failed: stub error" && g_event_creates == creates);
    CHECK(sp.ev[0] == nullptr && sp.ev[3] == had && g_live_events == before + 1);
    (void)hipGetLastError();
    CHECK(sp.create_missing(e) == SIMMR_OK && g_event_creates == creates + 5 && sp.ev[3] == had && g_live_events == before + 6);
    CHECK(sp.create_missing(e) == SIMMR_OK && g_event_creates == creates + 5);  // none is missing
    for (int i = 0; i < 3; i++) CHECK(!sp.valid[i]);
    hipStream_t st = nullptr;
    g_recorded.clear();
    for (int i = 0; i < 3; i++) CHECK(sp.begin(i, st) == hipSuccess && sp.end(i, st) == hipSuccess);
    CHECK(g_recorded.size() == 6);
    for (int i = 0; i < 6; i++) CHECK(g_recorded[i] == sp.ev[i]);  // pair i is events 2i and 2i + 1
    for (int i = 0; i < 3; i++) CHECK(!sp.valid[i]);               // recording marks nothing
    g_span_ms[sp.ev[0]] = 1.5f;
    g_span_ms[sp.ev[2]] = 0.25f;
    g_span_ms[sp.ev[4]] = 8.f;
    float ms = -1.f;
    long calls = g_elapsed_calls, syncs = g_syncs;
    CHECK(sp.total_ms(e, "spans", &ms) == SIMMR_OK && ms == 0.f && g_elapsed_calls == calls && g_syncs == syncs + 1);  // none marked, none read
    sp.mark(0);
    CHECK(sp.total_ms(e, "spans", &ms) == SIMMR_OK && ms == 1.5f && g_elapsed_calls == calls + 1);
    sp.mark(2);
    CHECK(sp.total_ms(e, "spans", &ms) == SIMMR_OK && ms == 9.5f && g_elapsed_calls == calls + 3);  // 0 and 2, not 1
    sp.mark(1);
    CHECK(sp.total_ms(e, "spans", &ms) == SIMMR_OK && ms == 9.75f);
    sp.mark(2, false);
    CHECK(sp.total_ms(e, "spans", &ms) == SIMMR_OK && ms == 1.75f);
    sp.mark(2);
    sp.invalidate_from(1);
    CHECK(sp.valid[0] && !sp.valid[1] && !sp.valid[2]);
    CHECK(sp.total_ms(e, "spans", &ms) == SIMMR_OK && ms == 1.5f);
    sp.invalidate_from(3);  // from behind the last: nothing
    CHECK(sp.valid[0]);
    // the synchronisation is checked first, under the caller's name
    g_pending = hipErrorOutOfMemory;
    calls = g_elapsed_calls;
    ms = -1.f;
    CHECK(sp.total_ms(e, "spans", &ms) == SIMMR_ENODEV && e->err == "spans: stub error" && ms == -1.f && g_elapsed_calls == calls);
    g_fail_next_elapsed = true;
    CHECK(sp.total_ms(e, "spans", &ms) == SIMMR_ENODEV && ms == -1.f);
    CHECK(e->err == "hipEventElapsedTime(&one, ev[2 * i], ev[2 * i + 1]) failed: stub error");
    sp.invalidate_from(0);
    CHECK(sp.total_ms(e, "spans", &ms) == SIMMR_OK && ms == 0.f);
    // a state moves with its events: what it is moved from destroys nothing
    sp.mark(0);
    Spans<3> to(std::move(sp));
    for (int i = 0; i < 6; i++) CHECK(sp.ev[i] == nullptr && to.ev[i] != nullptr);
    CHECK(to.ev[3] == had && to.valid[0] && !to.valid[1] && g_live_events == before + 6);
    CHECK(to.total_ms(e, "spans", &ms) == SIMMR_OK && ms == 1.5f);
    static_assert(!std::is_copy_constructible<Spans<3>>::value && !std::is_copy_assignable<Spans<3>>::value, "a set of spans does not copy");
    Spans<1> one;  // never used: owns nothing
  }
  CHECK(g_live_events == before);
  g_span_ms.clear();
  g_recorded.clear();
}

struct UnitState {  // as a unit's state: buffers, an array of buffers, events, host members
  DevBuf a, b[2];
  Events<4> ev;
  Spans<2> sp;
  std::vector<uint64_t> host = {1, 2, 3};
};

static void state_in_a_slot(simmr_engine* e) {
  const long before = live();
  CHECK((unit_state<UnitState, ENG_EXT_STRAIN>(e, false)) == nullptr && e->slot[ENG_EXT_STRAIN] == nullptr);
  UnitState* s = unit_state<UnitState, ENG_EXT_STRAIN>(e, true);
  CHECK(s && e->slot[ENG_EXT_STRAIN] == s && e->destroy[ENG_EXT_STRAIN]);
  CHECK((unit_state<UnitState, ENG_EXT_STRAIN>(e, true)) == s && (unit_state<UnitState, ENG_EXT_STRAIN>(e, false)) == s);
  CHECK((unit_state<UnitState, ENG_EXT_DEPTH>(e, false)) == nullptr);  // another unit's slot
  CHECK(s->a.ensure(100) && s->b[0].ensure(200) && s->b[1].ensure_slack(300) && s->ev.create_missing(e) == SIMMR_OK && s->sp.create_missing(e) == SIMMR_OK);
  CHECK(live() == before + 3 + 4 + 4);
  // what simmr_engine_destroy does with a slot
  e->destroy[ENG_EXT_STRAIN](e->slot[ENG_EXT_STRAIN]);
  e->slot[ENG_EXT_STRAIN] = nullptr;
  CHECK(live() == before);
}

static void sync_and_macro(simmr_engine* e) {
  const long syncs = g_syncs;
  CHECK(sync_check(e, "a pass") == SIMMR_OK && g_syncs == syncs + 1);
  g_pending = hipErrorOutOfMemory;  // an error some earlier call left behind
  CHECK(sync_check(e, "a pass") == SIMMR_ENODEV && e->err == "a pass: stub error" && g_pending == hipSuccess);
  auto through_macro = [](simmr_engine* e, hipError_t s) -> int {
    HIP_TRY(e, hipGetErrorString(s) ? s : s);
    return SIMMR_OK;
  };
  CHECK(through_macro(e, hipSuccess) == SIMMR_OK);
  CHECK(through_macro(e, hipErrorOutOfMemory) == SIMMR_ENODEV && e->err == "hipGetErrorString(s) ? s : s failed: stub error");
}

static void rows(simmr_engine* e) {
  using V32 = std::vector<uint32_t>;
  using V64 = std::vector<uint64_t>;
  StagedRows none = staged_rows(e, true);
  CHECK(none.n_slots() == 0 && none.n_rows() == 0 && none.first == V64{0} && none.longest == 0 && none.cbase.empty());
  e->genomes = {{5, 7}, {}, {3}, {}};  // slots 1 and 3 are not staged
  StagedRows r = staged_rows(e, true);
  CHECK(r.n_slots() == 4 && r.n_rows() == 3 && r.longest == 7);
  CHECK((r.cbase == V32{0, 2, 2, 3}) && (r.ncontig == V32{2, 0, 1, 0}));
  CHECK((r.bases == V64{5, 7, 3}) && (r.first == V64{0, 5, 12, 15}));
  CHECK((r.genome == V32{0, 0, 2}) && (r.contig == V32{0, 1, 0}));
  StagedRows plain = staged_rows(e);
  CHECK(plain.genome.empty() && plain.contig.empty() && plain.bases == r.bases && plain.first == r.first && plain.cbase == r.cbase);
}

// ---- scorer_host.hpp -------------------------------------------------------------------------------------------------
static void bits_and_grids(simmr_engine* e) {
  CHECK(bits_of(0) == 0 && bits_of(1) == 1 && bits_of(0xffffffffull) == 32 && bits_of(1ull << 32) == 33 && bits_of(~0ull) == 64);
  CHECK(grid_for(e, 0, 256, 2) == 1);         // nothing to do: one workgroup all the same
  CHECK(grid_for(e, 256, 256, 2) == 1 && grid_for(e, 257, 256, 2) == 2);  // one item more than a workgroup
  CHECK(grid_for(e, 1ull << 40, 256, 2) == 8 && grid_for(e, 9, 1, 2) == 8 && grid_for(e, 8, 1, 2) == 8 && grid_for(e, 7, 1, 2) == 7);  // past the cap: 4 CUs
  e->cus = 0;  // (an engine that could not tell counts as one CU)
  CHECK(grid_for(e, 1000, 1, 16) == 16);
  e->cus = 4;
  CHECK(grid_capped(0, 64, 3) == 1 && grid_capped(65, 64, 3) == 2 && grid_capped(1000, 64, 3) == 3);
}

static void grown_columns_are_zero() {
  DevBuf b;
  CHECK(grow_zero(&b, 4, 0, 4, nullptr) && b.cap >= 16);
  for (int i = 0; i < 4; i++) { CHECK(b.as<uint32_t>()[i] == 0); b.as<uint32_t>()[i] = 7u + i; }
  CHECK(grow_zero(&b, 100, 4, 4, nullptr) && b.cap >= 400);
  for (int i = 0; i < 100; i++) CHECK(b.as<uint32_t>()[i] == (i < 4 ? 7u + i : 0u));
  g_fail_next_malloc = true;
  CHECK(!grow_zero(&b, 1000, 100, 4, nullptr) && b.as<uint32_t>()[3] == 10u);  // what it held stays where it cannot grow
}

static void add_text_checks(simmr_engine* e) {
  const uint8_t text[4] = {'a', '\n', 'b', '\n'};
  // the three refusals in their order: every one with all three wrong, then with the earlier ones right
  CHECK(check_add_text(e, false, nullptr, 9, 8, "simmr_x_add", "simmr_x_reset", "cut it") == SIMMR_ESTATE && e->err == "simmr_x_add called before simmr_x_reset");
  CHECK(check_add_text(e, true, nullptr, 9, 8, "simmr_x_add", "simmr_x_reset", "cut it") == SIMMR_EINVAL && e->err == "simmr_x_add: NULL text");
  CHECK(check_add_text(e, true, text, 9, 8, "simmr_x_add", "simmr_x_reset", "cut it") == SIMMR_ENOTSUP);
  CHECK(e->err == "simmr_x_add: 9 bytes in one add (at most 8: cut it)");
  CHECK(check_add_text(e, true, text, 1ull << 33, (1ull << 33) - 1, "w", "r", "cut the text at a line's end") == SIMMR_ENOTSUP);
  CHECK(e->err == "w: 8589934592 bytes in one add (at most 8589934591: cut the text at a line's end)");
  e->err = "kept";
  CHECK(check_add_text(e, true, text, 4, 8, "w", "r", "c") == SIMMR_OK && check_add_text(e, true, text, 8, 8, "w", "r", "c") == SIMMR_OK);
  CHECK(check_add_text(e, true, nullptr, 0, 8, "w", "r", "c") == SIMMR_OK && e->err == "kept");  // no bytes need no text
}

static void folded_spans(simmr_engine* e) {
  const long before = g_live_events;
  {
    FoldedSpans<3> f;
    hipStream_t st = nullptr;
    CHECK(f.reset(e) == SIMMR_OK && g_live_events == before + 6 && !f.open && f.done_ms == 0.f);
    float ms = -1.f;
    long calls = g_elapsed_calls, syncs = g_syncs;
    CHECK(f.last_ms(e, "unit", &ms) == SIMMR_OK && ms == 0.f && g_elapsed_calls == calls && g_syncs == syncs + 1);  // a reset and no add
    // two adds are one span, from the first one's begin to the last one's end
    g_recorded.clear();
    CHECK(f.begin(e, 0, st) == SIMMR_OK && !f.open && !f.sp.valid[0]);
    CHECK(f.end(e, 0, st, "unit add") == SIMMR_OK && f.open && f.sp.valid[0]);
    CHECK(f.begin(e, 0, st) == SIMMR_OK && f.end(e, 0, st, "unit add") == SIMMR_OK);
    CHECK(g_recorded.size() == 3 && g_recorded[0] == f.sp.ev[0] && g_recorded[1] == f.sp.ev[1] && g_recorded[2] == f.sp.ev[1]);
    // a span of its own beside it; span 2 is never run and never read
    CHECK(f.begin(e, 1, st) == SIMMR_OK && f.end(e, 1, st, "unit plan") == SIMMR_OK && f.sp.valid[1] && !f.sp.valid[2]);
    CHECK(g_recorded.size() == 5 && g_recorded[3] == f.sp.ev[2] && g_recorded[4] == f.sp.ev[3]);
    g_span_ms[f.sp.ev[0]] = 2.f;
    g_span_ms[f.sp.ev[2]] = 0.5f;
    g_span_ms[f.sp.ev[4]] = 64.f;
    // a fold adds the marked spans once and closes them
    calls = g_elapsed_calls;
    CHECK(f.fold(e, "unit") == SIMMR_OK && f.done_ms == 2.5f && g_elapsed_calls == calls + 2 && !f.open && !f.sp.valid[0] && !f.sp.valid[1]);
    CHECK(f.fold(e, "unit") == SIMMR_OK && f.done_ms == 2.5f && g_elapsed_calls == calls + 2);
    CHECK(f.last_ms(e, "unit", &ms) == SIMMR_OK && ms == 2.5f);
    // a begin after a fold opens a new span
    g_recorded.clear();
    CHECK(f.begin(e, 0, st) == SIMMR_OK && g_recorded.size() == 1 && g_recorded[0] == f.sp.ev[0] && !f.open);
    // a launch that failed (the error it left pending) leaves the span as it was: not ended, not open, not marked
    g_pending = hipErrorOutOfMemory;
    CHECK(f.end(e, 0, st, "unit add") == SIMMR_ENODEV && e->err == "unit add launch failed: stub error");
    CHECK(g_recorded.size() == 1 && !f.open && !f.sp.valid[0] && g_pending == hipSuccess);
    CHECK(f.last_ms(e, "unit", &ms) == SIMMR_OK && ms == 2.5f);
    // ... and an open one open and marked, with the end it had
    CHECK(f.begin(e, 0, st) == SIMMR_OK && f.end(e, 0, st, "unit add") == SIMMR_OK && g_recorded.size() == 3 && f.open);
    g_pending = hipErrorOutOfMemory;
    CHECK(f.begin(e, 0, st) == SIMMR_OK && f.end(e, 0, st, "unit add") == SIMMR_ENODEV && g_recorded.size() == 3 && f.open && f.sp.valid[0]);
    g_span_ms[f.sp.ev[0]] = 4.f;
    // the fold's synchronisation is checked under the unit's name, and a fold that failed has folded nothing
    g_pending = hipErrorOutOfMemory;
    CHECK(f.fold(e, "unit") == SIMMR_ENODEV && e->err == "unit: stub error" && f.done_ms == 2.5f && f.open && f.sp.valid[0]);
    CHECK(f.last_ms(e, "unit", &ms) == SIMMR_OK && ms == 6.5f && !f.open);
    // reset zeroes the sum and makes no event anew
    CHECK(f.begin(e, 0, st) == SIMMR_OK && f.end(e, 0, st, "unit add") == SIMMR_OK);
    const long creates = g_event_creates;
    CHECK(f.reset(e) == SIMMR_OK && g_event_creates == creates && !f.open && f.done_ms == 0.f && !f.sp.valid[0]);
    CHECK(f.last_ms(e, "unit", &ms) == SIMMR_OK && ms == 0.f);
  }
  CHECK(g_live_events == before);
  g_span_ms.clear();
  g_recorded.clear();
}

static bool no_blank(const char* s, size_t n) { return !memchr(s, ' ', n); }

static void sorted_name_tables(simmr_engine* e) {
  SortedNames t;
  CHECK(sorted_names(e, nullptr, 0, 254, no_blank, "genome name", nullptr, &t) == SIMMR_OK);
  CHECK(t.blob == std::vector<uint8_t>(8, 0) && t.off == std::vector<uint32_t>{0} && t.order.empty());
  // the refusals, with the texts of the units
  const std::string longest(254, 'x'), too_long(255, 'x');
  const char* empty[] = {"a", ""};
  CHECK(sorted_names(e, empty, 2, 254, no_blank, "genome name", nullptr, &t) == SIMMR_ENOTSUP && e->err == "genome name 1 is empty or longer than 254 bytes");
  const char* null_name[] = {nullptr};
  CHECK(sorted_names(e, null_name, 1, 254, no_blank, "contig name", nullptr, &t) == SIMMR_ENOTSUP && e->err == "contig name 0 is empty or longer than 254 bytes");
  const char* lengths[] = {longest.c_str(), "b", too_long.c_str()};
  CHECK(sorted_names(e, lengths, 2, 254, no_blank, "reference name", nullptr, &t) == SIMMR_OK);
  CHECK(sorted_names(e, lengths, 3, 254, no_blank, "reference name", nullptr, &t) == SIMMR_ENOTSUP && e->err == "reference name 2 is empty or longer than 254 bytes");
  const char* illegal[] = {"ok", "a b"};
  CHECK(sorted_names(e, illegal, 2, 254, no_blank, "reference name", nullptr, &t) == SIMMR_ENOTSUP && e->err == "'a b' (reference name 1) is not a SAM reference name");
  CHECK(sorted_names(e, illegal, 2, 254, no_blank, "genome id", "holds a tab or a newline", &t) == SIMMR_ENOTSUP && e->err == "genome id 1 holds a tab or a newline");
  CHECK(sorted_names(e, illegal, 1, 254, no_blank, "genome id", "holds a tab or a newline", &t) == SIMMR_OK);
  const char* twice[] = {"chr2", "chr1", "chr10", "chr1"};
  CHECK(sorted_names(e, twice, 4, 254, no_blank, "reference name", nullptr, &t) == SIMMR_EINVAL && e->err == "reference name 'chr1' is given twice");
  CHECK(sorted_names(e, twice, 3, 254, no_blank, "reference name", nullptr, &t) == SIMMR_OK);
  // a prefix sorts first; bytes from 128 on sort as unsigned, behind every ASCII byte
  const char* given[] = {"b", "ab", "a", "\xc3\xa9", "z", "a\xff", "aa"};
  const uint32_t n = 7;
  CHECK(sorted_names(e, given, n, 254, no_blank, "genome id", "x", &t) == SIMMR_OK);
  CHECK((t.order == std::vector<uint32_t>{2, 6, 1, 5, 0, 4, 3}));
  CHECK((t.off == std::vector<uint32_t>{0, 1, 3, 5, 7, 8, 9, 11}) && t.blob.size() == 11 + 8);
  CHECK(std::string(t.blob.begin(), t.blob.begin() + 11) == "aaaaba\xff" "bz\xc3\xa9");
  for (size_t i = 11; i < t.blob.size(); i++) CHECK(t.blob[i] == 0);  // the padding a device reader may run into
  std::vector<bool> seen(n, false);
  for (uint32_t i = 0; i < n; i++) {  // order is a permutation, and sorted name i is the name given at order[i]
    CHECK(t.order[i] < n && !seen[t.order[i]]);
    seen[t.order[i]] = true;
    CHECK(std::string(t.blob.begin() + t.off[i], t.blob.begin() + t.off[i + 1]) == given[t.order[i]]);
  }
  // what the units did before (std::sort over std::string) is the same order for names a unit takes: bytes below 128
  std::vector<std::string> ascii = {"chr10", "chr1", "chrX", "chr", "Chr1", "chr1_alt", "chr1.1", "chr1|a", "~", "!", "9", "chr1-", "A"};
  std::vector<const char*> ptrs;
  for (const std::string& a : ascii) ptrs.push_back(a.c_str());
  CHECK(sorted_names(e, ptrs.data(), (uint32_t)ptrs.size(), 254, no_blank, "reference name", nullptr, &t) == SIMMR_OK);
  std::vector<std::string> was = ascii;
  std::sort(was.begin(), was.end());
  for (size_t i = 0; i < was.size(); i++) CHECK(std::string(t.blob.begin() + t.off[i], t.blob.begin() + t.off[i + 1]) == was[i]);
  // the device copy
  const long before = g_live_bufs;
  {
    DeviceNames d;
    CHECK(d.room(t) && g_live_bufs == before + 2 && d.blob.cap == t.blob.size() && d.name_off.cap == t.off.size() * 4);
    CHECK(d.upload(e, t, nullptr) == SIMMR_OK && !memcmp(d.blob.p, t.blob.data(), t.blob.size()) && !memcmp(d.name_off.p, t.off.data(), t.off.size() * 4));
    g_fail_next_malloc = true;
    SortedNames larger = t;
    larger.blob.resize(4096, 0);
    CHECK(!d.room(larger));
  }
  CHECK(g_live_bufs == before);
}

struct Scorer {  // as a scorer's object: the engine, buffers, spans
  simmr_engine* e = nullptr;
  LineIndex index;
  PairSort order;
  FoldedSpans<2> sp;
};

static void scorer_objects(simmr_engine* e) {
  const long before = live();
  Scorer* h = (Scorer*)0x1;
  CHECK(scorer_create<Scorer>(nullptr, &h, "simmr_x_create") == SIMMR_EINVAL && h == (Scorer*)0x1);
  CHECK(scorer_create<Scorer>(e, nullptr, "simmr_x_create") == SIMMR_EINVAL && e->err == "simmr_x_create: NULL out");
  CHECK(scorer_create(e, &h, "simmr_x_create") == SIMMR_OK && h && h != (Scorer*)0x1 && h->e == e && live() == before);
  CHECK(h->index.room(3, 100) && h->index.tile_sum.cap == 24 && h->index.tile_prefix.cap == 32 && h->index.starts.cap == 400);
  CHECK(h->order.room(1) && h->order.key[0].cap == 8 && h->order.key[1].cap == 8 && h->order.idx[0].cap == 4 && h->order.idx[1].cap == 4);
  CHECK(h->order.hist.cap == SAMSORT_PAIRS_DIGITS * 4 && h->order.digit_total.cap == SAMSORT_PAIRS_DIGITS * 4);
  CHECK(h->order.room(SAMSORT_PAIRS_TILE + 1) && h->order.hist.cap == 2 * SAMSORT_PAIRS_DIGITS * 4 && h->order.key[1].cap == (SAMSORT_PAIRS_TILE + 1) * 8);
  CHECK(h->sp.reset(e) == SIMMR_OK && live() == before + 3 + 6 + 4);
  const long syncs = g_syncs;
  g_pending = hipErrorOutOfMemory;  // what a failed call of the caller's left behind goes with the object
  scorer_destroy(h);
  CHECK(live() == before && g_syncs == syncs + 1 && g_pending == hipSuccess);
  scorer_destroy<Scorer>(nullptr);
  CHECK(g_syncs == syncs + 1);
}

int main() {
  simmr_engine e;
  ensure_keeps_grows_and_fails();
  growth_rules();
  one_owner();
  vector_of_holders();
  events_set(&e);
  spans(&e);
  state_in_a_slot(&e);
  sync_and_macro(&e);
  rows(&e);
  bits_and_grids(&e);
  grown_columns_are_zero();
  add_text_checks(&e);
  folded_spans(&e);
  sorted_name_tables(&e);
  scorer_objects(&e);
  if (g_failed) return 101;
  printf("ok: %ld allocations, %ld events, %ld alive\n", g_mallocs, g_event_creates, live());
  return live() > 100 ? 100 : (int)live();
}
