// Host helpers of the training nodes' C entries (vge_timelayer.hip, vge_linear.hip, vge_fusion.hip): the error return,
// and the null / alignment / aliasing checks that run before the first HIP call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/vge.h"
#include "vge_error.h"

namespace {

inline int fail(int code, const std::string& msg) {
  vge::set_last_error(msg);
  return code;
}

inline hipStream_t tl_stream(vge_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

struct Span {
  const void* p;
  size_t bytes;
  const char* name;
  bool optional;
  bool float_aligned = false;  // 4-byte alignment is enough (an operand read in place from a wider tensor)
};

inline bool overlap(const Span& a, const Span& b) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
  return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// null, alignment and aliasing of the listed buffers: the first n_in are inputs (they may alias each other), the
// rest outputs (they may alias nothing); optional entries may be null
inline int tl_buffers(const char* fn, const Span* sp, int n_in, int n) {
  for (int i = 0; i < n; ++i) {
    if (!sp[i].p) {
      if (sp[i].optional) continue;
      return fail(VGE_ERR_ARG, std::string(fn) + ": null " + sp[i].name);
    }
    if (reinterpret_cast<uintptr_t>(sp[i].p) & (sp[i].float_aligned ? 3 : 15))
      return fail(VGE_ERR_ARG, std::string(fn) + ": " + sp[i].name + " must be " +
                  (sp[i].float_aligned ? "4" : "16") + "-byte aligned");
  }
  for (int i = n_in; i < n; ++i)
    for (int k = 0; k < i; ++k)
      if (sp[i].p && sp[k].p && overlap(sp[i], sp[k]))
        return fail(VGE_ERR_ARG, std::string(fn) + ": " + sp[i].name + " must not alias " + sp[k].name);
  return VGE_OK;
}

#define HIPCHK(expr)                                                                                    \
  do {                                                                                                  \
    hipError_t _e = (expr);                                                                             \
    if (_e != hipSuccess) return fail(VGE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

}  // namespace
