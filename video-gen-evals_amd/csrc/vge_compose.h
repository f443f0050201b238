// The file walk and the compose kernel of the device decoders whose files are chains of delta frames (vge_gif.hip,
// vge_webp.hip, vge_apng.hip).  The plan emits a file's descriptors next to each other, index 0 first, and the files
// in increasing order of their owner field.
//
//   compose   a row of workgroups per file (the file's first descriptor is found by a binary search on the owner
//             field), a lane per canvas pixel: it walks the file's frames in order with the format's Pixel in
//             registers (the canvas value and what the previous frame's disposal puts back; the step is the host
//             decoder's call) and stores RGB for every frame.  It stops at the first frame whose status is set and
//             gives the later frames that status.
//
// Hard rules, the same as in vge_png_kernels.h:
//   - every descriptor is checked against the sizes the host passed (Route::check_desc) before anything is read or
//     written through it; a descriptor order the plan does not emit is refused by the format's first per-frame kernel
//     (reachable), so that no frame is left with status 0 and no pixels;
//   - a frame reads only its own slot and file bytes, writes only its own output frame;
//   - every loop consumes descriptors or produces output;
//   - a frame that fails, or follows one that did, gets that status (atomicCAS from 0: the first failure wins);
//   - no workgroup waits for another.
//
// Route supplies:
//   Route::Args          with descs, n_descs, n_files, n_frames, width, height, rgb, status; descriptors with file,
//                        index and frame
//   Route::check_desc    0: run it; < 0: an unused slot (nobody to report to); > 0: the code to report
//   Route::ERR_ARG       the status of the frames behind an unused slot inside a file
//   Route::Pixel         the canvas pixel's state, with canvas = R | G << 8 | B << 16
//   Route::first_pixel   that state in front of a file's first descriptor
//   Route::step          one canvas pixel (px, py) through frame d, whose predecessor in the file is prev (d itself
//                        for the first)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vge_gather.h"

namespace vge_compose {

using vge_gather::WIDE;

// The first descriptor whose file is not below f; n_descs when there is none.
template <class Args>
__device__ int lower_bound_file(const Args& A, int f) {
  int lo = 0, hi = A.n_descs;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (A.descs[mid].file < f) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Descriptor k continues the chain of k - 1: the same file, the next frame index.
template <class Desc>
__device__ inline bool continues(const Desc& prev, const Desc& d) {
  return prev.file == d.file && d.index > 0 && prev.index == d.index - 1;
}

// The compose kernel reaches descriptor k when the chain it belongs to starts at index 0 and that start is where the
// search for its file lands.
template <class Args>
__device__ bool reachable(const Args& A, int k) {
  int j = k;
  while (j > 0 && continues(A.descs[j - 1], A.descs[j])) --j;  // at most `index` steps
  const auto h = A.descs[j];
  return h.index == 0 && h.file >= 0 && h.file < A.n_files && lower_bound_file(A, h.file) == j;
}

template <class Route>
__global__ __launch_bounds__(WIDE) void compose_kernel(typename Route::Args A) {
  const int64_t npix = (int64_t)A.width * A.height;
  const int64_t pix = (int64_t)blockIdx.x * WIDE + threadIdx.x;
  const bool active = pix < npix;
  const int px = (int)(pix % A.width), py = (int)(pix / A.width);
  const bool reporter = blockIdx.x == 0 && threadIdx.x == 0;
  for (int f = blockIdx.y; f < A.n_files; f += gridDim.y) {  // a row of workgroups per file
    const int k0 = lower_bound_file(A, f);
    if (k0 >= A.n_descs) continue;
    const auto d0 = A.descs[k0];
    if (d0.file != f || d0.index != 0) continue;  // a file without frames; a headless chain was refused before
    typename Route::Pixel P = Route::first_pixel(d0);
    int carried = 0;
    auto prev = d0;
    for (int k = k0; k < A.n_descs; ++k) {
      const auto d = A.descs[k];
      if (k > k0 && !continues(A.descs[k - 1], d)) break;
      const int chk = Route::check_desc(A, d);
      if (chk < 0) {  // an unused slot inside a file: nobody to report to, and the later frames are deltas on it
        if (carried == 0) carried = Route::ERR_ARG;
        continue;
      }
      if (carried == 0) carried = chk > 0 ? chk : A.status[d.frame];
      if (carried != 0) {
        if (reporter) atomicCAS(&A.status[d.frame], 0, carried);
        continue;
      }
      if (active) {
        Route::step(P, A, d, prev, px, py);
        uint8_t* o = A.rgb + ((int64_t)d.frame * npix + pix) * 3;
        o[0] = (uint8_t)P.canvas;
        o[1] = (uint8_t)(P.canvas >> 8);
        o[2] = (uint8_t)(P.canvas >> 16);
      }
      prev = d;
    }
  }
}

}  // namespace vge_compose
