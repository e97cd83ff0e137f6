// What the host-side translation units of libnode_hip.so share: the error text of the C ABI, the bump allocator of the
// workspace plans, the environment switches, the HIP-event profiler and the pinned host staging.  Host-only: no
// kernels_*.hip includes it.
#pragma once
#include "node_internal.h"
#include "../../include/node_hip.h"

#include <cstdlib>
#include <mutex>
#include <vector>

namespace node {

// ----------------------------------------------------------------------------
// error plumbing: the thread-local text behind node_last_error(); returns `code`
// ----------------------------------------------------------------------------
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) return fail(NODE_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
  } while (0)
#define TRY(expr)              \
  do {                         \
    int _rc = (expr);          \
    if (_rc != NODE_OK) return _rc; \
  } while (0)

// (the environment switches' one reader, env_int: node_internal.h -- the kernel units' launchers read switches too)

// the tiling geometry of a shape (dims.hip); refuses what no kernel is instantiated for
int dims_for(const node_shape* sh, Dims* out);

// carves 256-byte aligned arrays out of a workspace; base == nullptr: sizes only
struct Bump {
  char* base;
  size_t off;
  explicit Bump(void* b) : base((char*)b), off(0) {}
  template <typename T>
  T* take(size_t count) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? (T*)(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
};

// ----------------------------------------------------------------------------
// profiling (HIP events around the GEMM-class launches, on the caller's stream)
// ----------------------------------------------------------------------------
struct ProfRec { hipEvent_t a, b; int cls; double flops; };
struct Profiler {
  bool on = false;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> pool;
  std::mutex mu;
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
  }
};
extern Profiler g_prof;     // host_common.hip: switched by node_profile_begin / node_profile_end

struct ProfScope {
  bool active;
  ProfRec r;
  hipStream_t s;
  ProfScope(int cls, double flops, hipStream_t st) : active(g_prof.on), s(st) {
    if (!active) return;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    r.a = g_prof.get();
    r.b = g_prof.get();
    r.cls = cls;
    r.flops = flops;
    (void)hipEventRecord(r.a, s);
  }
  ~ProfScope() {
    if (!active) return;
    (void)hipEventRecord(r.b, s);
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.recs.push_back(r);
  }
};

// pinned host staging: the mirror of Ctrl for the read-backs and the small lists that travel to / from the device
// (target times, replay list, dt log).  One per host thread; every solve ends with a stream synchronisation, so
// the staging is free again when the next solve of this thread starts.  (Here and not with the solver: the generic
// solver of api_flat.hip stages through it too.)
struct HostStage {
  Ctrl* ctrl = nullptr;
  double* lists = nullptr;
  size_t cap = 0;      // doubles
};
int get_stage(size_t doubles, HostStage** out);

}  // namespace node
