// What all the device frame decoders share (vge_png.hip, vge_gif.hip, vge_webp.hip, vge_apng.hip): the workgroup sizes,
// the end of an entry function, and the gather kernel of those that read a stream cut into pieces (vge_png.hip: IDAT
// chunks; vge_gif.hip: data sub-blocks; vge_apng.hip: IDAT and fdAT chunks): one workgroup per segment copies a payload
// to its place in the frame's gathered run of the workspace, so that the bit reader sees one contiguous stream however
// the writer cut it.
//
// Route supplies the call's argument struct and its descriptor check:
//   Route::Args          with data, descs, segs, n_segs, n_descs, ws; descriptors with file_off, file_bytes, gat_off,
//                        gat_bytes and frame; segments of vge_png_segment's shape
//   Route::check_desc    0: run it; < 0: an unused slot (nobody to report to); > 0: the code to report
//   Route::fail          report a code for a frame (the first failure wins)
//   Route::ERR_ARG       the code of a segment that does not lie inside its file and its gathered run
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "vge_error.h"

namespace vge_gather {

constexpr int WAVE = 64;   // threads of the per-frame workgroups: one wavefront
constexpr int WIDE = 256;  // threads of the gather, Adler and compose workgroups

// For an entry function after its memset and its launches: HIP's last error, which this clears, as the entry's
// message.  False when there is none.
inline bool hip_failed(const char* entry) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) vge::set_last_error(std::string(entry) + ": " + hipGetErrorString(e));
  return e != hipSuccess;
}

template <class Route>
__global__ __launch_bounds__(WIDE) void gather_kernel(typename Route::Args A) {
  if ((int64_t)blockIdx.x >= A.n_segs) return;
  const auto g = A.segs[blockIdx.x];
  if (g.desc < 0 || g.desc >= A.n_descs) return;  // nobody to report to
  const auto d = A.descs[g.desc];
  const int chk = Route::check_desc(A, d);
  if (chk < 0) return;
  if (chk > 0) return Route::fail(A, d.frame, chk);
  if (g.bytes < 0 || g.src_off < d.file_off || g.src_off - d.file_off > d.file_bytes ||
      g.bytes > d.file_bytes - (g.src_off - d.file_off) || g.dst_off < d.gat_off ||
      g.dst_off - d.gat_off > d.gat_bytes || g.bytes > d.gat_bytes - (g.dst_off - d.gat_off))
    return Route::fail(A, d.frame, Route::ERR_ARG);
  const uint8_t* src = A.data + g.src_off;
  uint8_t* dst = A.ws + g.dst_off;
  for (int64_t k = threadIdx.x; k < g.bytes; k += WIDE) dst[k] = src[k];
}

}  // namespace vge_gather
