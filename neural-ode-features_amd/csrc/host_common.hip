// The one home of the C ABI's error text, the profiler state and the pinned host staging (host_common.h).
#include "host_common.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace node {

static thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
// the same thread-local message for the kernel translation units, which do not see host_common.h (node_internal.h)
int set_error(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}

Profiler g_prof;

static thread_local HostStage g_stage;

int get_stage(size_t doubles, HostStage** out) {
  if (!g_stage.ctrl) HIP_TRY(hipHostMalloc((void**)&g_stage.ctrl, sizeof(Ctrl), hipHostMallocDefault));
  if (g_stage.cap < doubles) {
    if (g_stage.lists) (void)hipHostFree(g_stage.lists);
    g_stage.lists = nullptr;
    g_stage.cap = 0;
    const size_t want = doubles < 16384 ? 16384 : doubles;
    HIP_TRY(hipHostMalloc((void**)&g_stage.lists, want * sizeof(double), hipHostMallocDefault));
    g_stage.cap = want;
  }
  *out = &g_stage;
  return NODE_OK;
}

}  // namespace node

using namespace node;

extern "C" {

int node_abi_version(void) { return NODE_ABI_VERSION; }
const char* node_last_error(void) { return g_err; }

int node_profile_begin(void) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  for (auto& r : g_prof.recs) { g_prof.pool.push_back(r.a); g_prof.pool.push_back(r.b); }
  g_prof.recs.clear();
  g_prof.on = true;
  return NODE_OK;
}

int node_profile_end(node_profile* out) {
  if (!out) return fail(NODE_ERR_NULL, "out is NULL");
  std::lock_guard<std::mutex> lk(g_prof.mu);
  g_prof.on = false;
  memset(out, 0, sizeof(*out));
  for (auto& r : g_prof.recs) {
    if (hipEventSynchronize(r.b) != hipSuccess) return fail(NODE_ERR_HIP, "hipEventSynchronize failed");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return fail(NODE_ERR_HIP, "hipEventElapsedTime failed");
    out->launches[r.cls] += 1;
    out->total_ms[r.cls] += ms;
    out->flops[r.cls] += r.flops;
    g_prof.pool.push_back(r.a);
    g_prof.pool.push_back(r.b);
  }
  g_prof.recs.clear();
  return NODE_OK;
}

}  // extern "C"
