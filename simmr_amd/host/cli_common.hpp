// cli_common.hpp — what main.cpp and eval_cli.cpp both need: the three message lines, the number formatter, the growing device
// buffer and the holder of a command's engines.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "simmr_host.hpp"

inline void info(const std::string& msg) { fprintf(stderr, " INFO simmr-hip: %s\n", msg.c_str()); }
inline void warn(const std::string& msg) { fprintf(stderr, " WARN simmr-hip: %s\n", msg.c_str()); }
inline int die(const std::string& msg) { fprintf(stderr, "ERROR simmr-hip: %s\n", msg.c_str()); return 1; }
inline std::string n(uint64_t v) { return std::to_string((unsigned long long)v); }  // a count, in an info line

// A buffer that grows to the largest size asked of it, with a sixteenth to spare so that sizes creeping up do not allocate
// every time: device memory, or pinned host memory.
struct GrowBuf {
  bool pinned = false;
  void* p = nullptr;
  uint64_t cap = 0;
  ~GrowBuf() { release(); }
  void release() { if (p) (void)(pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
  // room for `bytes`, or nullptr if there is none; what the buffer held is gone when it grows
  uint8_t* room(uint64_t bytes) {
    if (cap < bytes) {
      release();
      const uint64_t want = bytes + bytes / 16 + 256;
      if ((pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want)) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return nullptr; }
      cap = want;
    }
    return (uint8_t*)p;
  }
};

struct Engines {  // released on every way out of run_main
  std::vector<simmr_engine*> v;
  simmr_bam_sort* bam_sort = nullptr;  // --bam-sorted: its state lives on an engine and goes before it
  ~Engines() {
    simmr_bam_sort_destroy(bam_sort);
    for (simmr_engine* en : v) simmr_engine_destroy(en);
  }
};
