// The device half of the APNG video front end (include/vge_apng.h): APNG files in device memory -> uint8 RGB frames,
// from the host's plan (csrc/vge_apng.cpp: one descriptor per frame, one segment per IDAT / fdAT payload) and the file
// bytes alone.
//
//   gather    vge_gather.h's kernel: each frame's payloads (the plan has stepped over the fdAT sequence numbers) into
//             one run of the workspace.
//   inflate, adler, unfilter
//             vge_png_kernels.h's, which states the scheme and the hard rules; a frame is its rectangle, with its own
//             count h * (1 + w * bytes_per_pixel).  The inflate kernel refuses what the compose kernel does not reach.
//             The unfilter puts every reconstructed byte back over its filtered byte, so that the slot holds the raw
//             pixels of the file's colour type, alpha included.
//   compose   vge_compose.h's kernel and rules, with vge_apng_px.h's compose_pixel, the host's call.
#include <hip/hip_runtime.h>

#include "../../include/vge_apng.h"
#include "vge_apng_px.h"
#include "vge_compose.h"
#include "vge_error.h"
#include "vge_gather.h"
#include "vge_png_kernels.h"

namespace {

using namespace vge_png_kernels;
using vge::set_last_error;
using vge_apng::bytes_per_pixel;

struct Args {
  const uint8_t* data;
  int64_t data_bytes;
  const vge_apng_desc* descs;
  const vge_apng_segment* segs;
  int64_t n_segs;
  uint8_t* ws;
  int64_t ws_bytes;
  uint8_t* rgb;
  int32_t* status;
  int32_t n_descs, n_frames, n_files, width, height, color_type;
};

// What the shared kernels (vge_gather.h, vge_png_kernels.h, vge_compose.h) need of this route.
struct Route {
  using Args = ::Args;
  using Pixel = vge_apng::Pixel;
  static constexpr int ERR_ARG = VGE_APNG_ERR_ARG, ERR_IO = VGE_APNG_ERR_IO;

  // 0: run it; -1: an unused slot (or nobody to report to); else the plan's code, or the code of a descriptor that
  // does not fit the call.
  static __device__ int check_desc(const Args& A, const vge_apng_desc& d) {
    if (d.frame < 0 || d.frame >= A.n_frames) return -1;
    if (d.plan_status != 0) return d.plan_status > 0 ? d.plan_status : VGE_APNG_ERR_ARG;
    if (d.file_off < 0 || d.file_bytes < 0 || d.file_off > A.data_bytes || d.file_bytes > A.data_bytes - d.file_off)
      return VGE_APNG_ERR_ARG;
    if (d.w < 1 || d.h < 1 || d.x < 0 || d.y < 0 || d.w > A.width || d.h > A.height || d.x > A.width - d.w ||
        d.y > A.height - d.h || d.index < 0 || d.color_type != A.color_type)
      return VGE_APNG_ERR_ARG;
    const int64_t raw = (int64_t)d.h * (1 + (int64_t)d.w * bytes_per_pixel(A.color_type));
    if (d.raw_bytes != raw || raw >= (1ll << 31)) return VGE_APNG_ERR_ARG;
    const int64_t lo = align16((int64_t)A.n_descs * (int64_t)sizeof(Record));
    if (d.gat_off < lo || d.gat_bytes < 0 || d.gat_bytes >= (1ll << 28) || d.gat_off > A.ws_bytes ||
        d.gat_bytes > A.ws_bytes - d.gat_off)
      return VGE_APNG_ERR_ARG;
    const int64_t padded = (raw + 3) & ~(int64_t)3;
    if (d.slot_off < lo || (d.slot_off & 15) || d.slot_off > A.ws_bytes || padded > A.ws_bytes - d.slot_off)
      return VGE_APNG_ERR_ARG;
    return 0;
  }
  static __device__ void fail(const Args& A, int frame, int code) {
    if (threadIdx.x == 0) atomicCAS(&A.status[frame], 0, code);
  }
  static __device__ bool runs(const Args& A, int k) { return vge_compose::reachable(A, k); }
  static __device__ Pixel first_pixel(const vge_apng_desc&) { return Pixel{0, 0, 0}; }
  static __device__ void step(Pixel& P, const Args& A, const vge_apng_desc& d, const vge_apng_desc&, int px, int py) {
    vge_apng::compose_pixel(P, d, px, py, A.ws + d.slot_off);
  }
};

// The unfilter's sink: every pixel's bytes back into the slot.
struct SlotSink {
  int bpp;
  __device__ void operator()(int, int64_t, uint32_t px, uint8_t* bytes, bool) const {
    for (int c = 0; c < bpp; ++c) bytes[c] = (uint8_t)(px >> (8 * c));
  }
};

__global__ __launch_bounds__(WAVE) void unfilter_kernel(Args A) {
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_apng_desc d = A.descs[blockIdx.x];
  if (Route::check_desc(A, d) != 0 || vge_inflate::uni((uint32_t)A.status[d.frame]) != 0) return;
  const int bpp = bytes_per_pixel(A.color_type);
  unfilter_bands<Route>(A, d.frame, d.w, d.h, bpp, A.ws + d.slot_off, SlotSink{bpp});
}

}  // namespace

// For tools/bench_frames.py, which times the kernels one by one: bit 0 gather, 1 inflate, 2 adler, 3 unfilter,
// 4 compose.  Returns the previous mask; a negative mask only reads it.
static int g_stage_mask = 31;
extern "C" int vge_debug_apng_stage_mask(int mask) {
  const int prev = g_stage_mask;
  if (mask >= 0) g_stage_mask = mask & 31;
  return prev;
}

extern "C" int vge_apng_decode_device(const uint8_t* data, int64_t data_bytes, const vge_apng_desc* descs, int n_descs,
                                      const vge_apng_segment* segs, int64_t n_segs, int n_frames, int n_files, int width,
                                      int height, int color_type, void* workspace, int64_t workspace_bytes, uint8_t* rgb,
                                      int32_t* status, void* stream) {
  if (n_descs < 0 || n_segs < 0 || n_segs >= (1ll << 31) || n_frames < 0 || data_bytes < 0 || workspace_bytes < 0 ||
      n_files < 0 || width < 1 || height < 1 ||
      !(color_type == 0 || color_type == 2 || color_type == 4 || color_type == 6)) {
    set_last_error("vge_apng_decode_device: bad argument (count, size or layout)");
    return VGE_APNG_ERR_ARG;
  }
  if (n_frames == 0) return VGE_APNG_OK;
  if (!status || ((uintptr_t)status & 3)) {
    set_last_error("vge_apng_decode_device: bad argument (null or misaligned status)");
    return VGE_APNG_ERR_ARG;
  }
  if (n_descs > 0 && (!data || !descs || !workspace || !rgb || (n_segs > 0 && !segs) || ((uintptr_t)descs & 7) ||
                      ((uintptr_t)segs & 7) || ((uintptr_t)workspace & 15))) {
    set_last_error("vge_apng_decode_device: bad argument (null or misaligned buffer)");
    return VGE_APNG_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, (size_t)n_frames * 4, s) != hipSuccess) {
    vge_gather::hip_failed("vge_apng_decode_device");
    return VGE_APNG_ERR_HIP;
  }
  if (n_descs == 0) return VGE_APNG_OK;
  Args A;
  A.data = data;
  A.data_bytes = data_bytes;
  A.descs = descs;
  A.segs = segs;
  A.n_segs = n_segs;
  A.ws = static_cast<uint8_t*>(workspace);
  A.ws_bytes = workspace_bytes;
  A.rgb = rgb;
  A.status = status;
  A.n_descs = n_descs;
  A.n_frames = n_frames;
  A.n_files = n_files;
  A.width = width;
  A.height = height;
  A.color_type = color_type;
  const int stages = g_stage_mask;
  const int64_t pix_groups = ((int64_t)width * height + WIDE - 1) / WIDE;
  if (pix_groups >= (1ll << 31)) {
    set_last_error("vge_apng_decode_device: bad argument (a canvas of 2^39 pixels or more)");
    return VGE_APNG_ERR_ARG;
  }
  if (n_segs > 0 && (stages & 1))
    hipLaunchKernelGGL(vge_gather::gather_kernel<Route>, dim3((unsigned)n_segs), dim3(WIDE), 0, s, A);
  if (stages & 2) hipLaunchKernelGGL(inflate_kernel<Route>, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  if (stages & 4) hipLaunchKernelGGL(adler_kernel<Route>, dim3((unsigned)n_descs), dim3(WIDE), 0, s, A);
  if (stages & 8) hipLaunchKernelGGL(unfilter_kernel, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  if ((stages & 16) && n_files > 0)
    hipLaunchKernelGGL(vge_compose::compose_kernel<Route>,
                       dim3((unsigned)pix_groups, (unsigned)(n_files < 65535 ? n_files : 65535)), dim3(WIDE), 0, s, A);
  return vge_gather::hip_failed("vge_apng_decode_device") ? VGE_APNG_ERR_HIP : VGE_APNG_OK;
}
