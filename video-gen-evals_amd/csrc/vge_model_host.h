// Host-side helpers shared by every extractor model loader (vge_hmr.cpp: TokenHMR, vge_dwpose.cpp: RTMPose,
// vge_yolox.cpp: YOLOX, vge_frcnn.cpp: the gate detector): error returns, the device allocations a model owns,
// state_dict lookups with shape checks, the reserve()-sized workspace and per-call event-pair profiling.  The conv
// parts (BatchNorm folding, weight packing, the conv launch wrapper) are in vge_cnn_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/vge.h"
#include "vge_error.h"

namespace vge {
namespace host {

inline int fail(int code, const std::string& msg) {
  set_last_error(msg);
  return code;
}

inline int hip_status(hipError_t e, const char* what) {
  return e == hipSuccess ? VGE_OK : fail(VGE_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// VGE_RC: return a VGE_* status that is not VGE_OK to the caller; VGE_HIP(expr): a hipError_t as such a status, with
// the expression's text as the message; VGE_HIPCHK = both
#define VGE_RC(x)                                   \
  do {                                              \
    if (const int rc_ = (x); rc_ != VGE_OK) return rc_; \
  } while (0)
#define VGE_HIP(expr) ::vge::host::hip_status((expr), #expr)
#define VGE_HIPCHK(expr) VGE_RC(::vge::host::hip_status((expr), #expr))

inline hipStream_t S(vge_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline int rup(int x, int a) { return (x + a - 1) / a * a; }
inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline int pow2_at_least(int v, int lo) {
  int p = lo;
  while (p < v) p <<= 1;
  return p;
}
inline uint16_t to_bf16(float f) {  // round to nearest even (torch .to(bfloat16))
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

struct DevAllocs {
  std::vector<void*> allocs;
  DevAllocs() = default;
  DevAllocs(const DevAllocs&) = delete;
  DevAllocs& operator=(const DevAllocs&) = delete;
  ~DevAllocs() { release(); }
  void release() {
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
  }
  void* dmalloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(bytes, 256)) != hipSuccess) return nullptr;
    allocs.push_back(p);
    return p;
  }
};

template <class T>
bool upload(DevAllocs& d, const std::vector<T>& h, T** out) {
  *out = static_cast<T*>(d.dmalloc(h.size() * sizeof(T)));
  return *out && hipMemcpy(*out, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
}

struct WeightMap {
  std::unordered_map<std::string, const vge_tensor_view*> m;
  std::string missing, badshape;
  WeightMap(const vge_tensor_view* w, int n) {
    for (int i = 0; i < n; ++i)
      if (w[i].name) m[w[i].name] = &w[i];
  }
  const vge_tensor_view* get(const std::string& k, std::initializer_list<int64_t> shape) {
    auto it = m.find(k);
    if (it == m.end()) {
      if (missing.empty()) missing = k;
      return nullptr;
    }
    const vge_tensor_view* v = it->second;
    bool ok = v->ndim == (int)shape.size() && v->data;
    int i = 0;
    for (int64_t s : shape) ok = ok && v->shape[i++] == s;
    if (!ok && badshape.empty()) badshape = k;
    return ok ? v : nullptr;
  }
  int status(const std::string& who) const {
    if (!missing.empty()) return fail(VGE_ERR_MISSING_WEIGHT, who + ": missing weight " + missing);
    if (!badshape.empty()) return fail(VGE_ERR_WEIGHT_SHAPE, who + ": wrong shape for " + badshape);
    return fail(VGE_ERR_HIP, who + ": device allocation / upload failed");
  }
};

// The buffers a model's *_reserve sizes, owned apart from the weights.  reserve() replaces the whole set: the
// superseded buffers are freed once every kernel that may still read them has completed, then each new buffer is
// allocated, zeroed (pad rows stay finite) and assigned.  After a failure the set is incomplete, so callers clear
// their reserved size before the call and set it after.
struct Workspace {
  struct Buf {
    void** p;
    size_t bytes;
  };
  DevAllocs dev;
  int reserve(const std::string& who, const std::vector<Buf>& bufs) {
    if (!dev.allocs.empty()) {
      (void)hipDeviceSynchronize();
      dev.release();
    }
    for (const Buf& b : bufs) {
      void* p = dev.dmalloc(b.bytes);
      if (!p) return fail(VGE_ERR_NOMEM, who + ": hipMalloc failed");
      VGE_HIPCHK(hipMemset(p, 0, b.bytes));
      *b.p = p;
    }
    return VGE_OK;
  }
};

// event pairs around launches, by kind (per-call profiling of a model's forward)
struct Profiler {
  std::vector<hipEvent_t> ev;
  std::vector<int> kind;
  int max_calls = 0, calls = 0, per_call = 0;
  size_t pair = 0;
  bool on = false;
  double flops = 0;  // algorithmic GEMM FLOPs of the recorded calls (calls differ in size: a pass's tail)
  ~Profiler() {
    for (auto e : ev) (void)hipEventDestroy(e);
  }
  int begin(int n_calls, int pairs_per_call) {
    for (auto e : ev) (void)hipEventDestroy(e);
    per_call = pairs_per_call;
    ev.assign((size_t)n_calls * per_call * 2, nullptr);
    kind.assign((size_t)n_calls * per_call, -1);
    for (auto& e : ev) VGE_HIPCHK(hipEventCreate(&e));
    max_calls = n_calls;
    calls = 0;
    flops = 0;
    return VGE_OK;
  }
  void start_call() {
    on = calls < max_calls;
    pair = on ? (size_t)calls * per_call : 0;
  }
  void end_call(double call_flops) {
    if (on) ++calls, flops += call_flops;
    on = false;
  }
  double flops_per_call(double fallback) const { return calls ? flops / calls : fallback; }
  // pairs past a call's share of the event array are dropped
  int beg(int k, hipStream_t s) {
    if (on && pair < (size_t)(calls + 1) * per_call) {
      kind[pair] = k;
      VGE_HIPCHK(hipEventRecord(ev[2 * pair], s));
    }
    return VGE_OK;
  }
  int end(hipStream_t s) {
    if (on && pair < (size_t)(calls + 1) * per_call) VGE_HIPCHK(hipEventRecord(ev[2 * pair++ + 1], s));
    return VGE_OK;
  }
  int read(double* ms, int n_kinds, int* n_calls) {
    for (int i = 0; i < n_kinds; ++i) ms[i] = 0;
    for (size_t p = 0; p < (size_t)calls * per_call; ++p) {
      if (kind[p] < 0) continue;
      float t;
      VGE_HIPCHK(hipEventSynchronize(ev[2 * p + 1]));
      VGE_HIPCHK(hipEventElapsedTime(&t, ev[2 * p], ev[2 * p + 1]));
      ms[kind[p]] += t;
    }
    *n_calls = calls;
    return VGE_OK;
  }
};

// one event pair of `kind` around expr, which evaluates to a VGE_* status (a launcher's hipError_t: VGE_HIP(expr))
#define VGE_STAGE(prof, stream, kind, expr) \
  do {                                      \
    VGE_RC((prof).beg(kind, stream));       \
    VGE_RC(expr);                           \
    VGE_RC((prof).end(stream));             \
  } while (0)

}  // namespace host
}  // namespace vge
