// The device half of the PNG frame front end (include/vge_png.h): PNG files in device memory -> uint8 RGB frames, from
// the host's plan (csrc/vge_png.cpp: one descriptor per frame, one segment per IDAT chunk) and the file bytes alone.
//
//   gather    vge_gather.h's kernel: each frame's IDAT payloads into one run of the workspace (Pillow cuts a stream
//             every 64 KiB, libpng every 8 KiB).
//   inflate, adler, unfilter
//             vge_png_kernels.h's, which states the scheme and the hard rules; a frame is the whole image.  The
//             unfilter stores every pixel as RGB in the frame's output rows; only a band's last row is written back
//             over its filtered bytes in the slot, alpha included, for the next band to read.
#include <hip/hip_runtime.h>

#include "../../include/vge_png.h"
#include "vge_error.h"
#include "vge_gather.h"
#include "vge_png_kernels.h"

namespace {

using namespace vge_png_kernels;
using vge::set_last_error;

struct Args {
  const uint8_t* data;
  int64_t data_bytes;
  const vge_png_desc* descs;
  const vge_png_segment* segs;
  int64_t n_segs;
  uint8_t* ws;
  int64_t ws_bytes;
  uint8_t* rgb;
  int32_t* status;
  int32_t n_descs, n_frames, width, height, color_type;
};

__host__ __device__ inline int bytes_per_pixel(int ct) { return ct == 0 ? 1 : ct == 2 ? 3 : ct == 4 ? 2 : 4; }

// What the shared kernels (vge_gather.h, vge_png_kernels.h) need of this route.
struct Route {
  using Args = ::Args;
  static constexpr int ERR_ARG = VGE_PNG_ERR_ARG, ERR_IO = VGE_PNG_ERR_IO;

  // 0: run it; -1: an unused slot (or nobody to report to); else the code of a descriptor that does not fit the call.
  static __device__ int check_desc(const Args& A, const vge_png_desc& d) {
    if (d.frame < 0 || d.frame >= A.n_frames) return -1;
    const int64_t lo = align16((int64_t)A.n_descs * (int64_t)sizeof(Record));
    const int64_t raw = (int64_t)A.height * (1 + (int64_t)A.width * bytes_per_pixel(A.color_type));
    if (d.color_type != A.color_type || d.raw_bytes != raw || raw >= (1ll << 31)) return VGE_PNG_ERR_ARG;
    if (d.file_off < 0 || d.file_bytes < 0 || d.file_off > A.data_bytes || d.file_bytes > A.data_bytes - d.file_off)
      return VGE_PNG_ERR_ARG;
    if (d.gat_off < lo || d.gat_bytes < 0 || d.gat_bytes >= (1ll << 28) || d.gat_off > A.ws_bytes ||
        d.gat_bytes > A.ws_bytes - d.gat_off)
      return VGE_PNG_ERR_ARG;
    const int64_t padded = (raw + 3) & ~(int64_t)3;
    if (d.slot_off < lo || (d.slot_off & 15) || d.slot_off > A.ws_bytes || padded > A.ws_bytes - d.slot_off)
      return VGE_PNG_ERR_ARG;
    return 0;
  }
  static __device__ void fail(const Args& A, int frame, int code) {
    if (threadIdx.x == 0) atomicCAS(&A.status[frame], 0, code);
  }
  static __device__ bool runs(const Args&, int) { return true; }  // a frame stands alone
};

// The unfilter's sink: the pixel as RGB into the frame's output row, and a carried row's bytes back into the slot.
struct RgbSink {
  uint8_t* out_frame;
  int W, bpp;
  __device__ void operator()(int row, int64_t x, uint32_t px, uint8_t* bytes, bool carry) const {
    if (carry)
      for (int c = 0; c < bpp; ++c) bytes[c] = (uint8_t)(px >> (8 * c));
    const bool grey = bpp < 3;
    uint8_t* o = out_frame + ((int64_t)row * W + x) * 3;
    o[0] = (uint8_t)px;
    o[1] = (uint8_t)(grey ? px : px >> 8);
    o[2] = (uint8_t)(grey ? px : px >> 16);
  }
};

__global__ __launch_bounds__(WAVE) void unfilter_kernel(Args A) {
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_png_desc d = A.descs[blockIdx.x];
  if (Route::check_desc(A, d) != 0 || vge_inflate::uni((uint32_t)A.status[d.frame]) != 0) return;
  const int W = A.width, H = A.height, bpp = bytes_per_pixel(A.color_type);
  unfilter_bands<Route>(A, d.frame, W, H, bpp, A.ws + d.slot_off, RgbSink{A.rgb + (int64_t)d.frame * H * W * 3, W, bpp});
}

}  // namespace

extern "C" int vge_png_decode_device_band_rows(void) { return BAND; }

// For tools/bench_frames.py, which times the kernels one by one: bit 0 gather, 1 inflate, 2 adler, 3 unfilter.
// Returns the previous mask; a negative mask only reads it.
static int g_stage_mask = 15;
extern "C" int vge_debug_png_stage_mask(int mask) {
  const int prev = g_stage_mask;
  if (mask >= 0) g_stage_mask = mask & 15;
  return prev;
}

extern "C" int vge_png_decode_device(const uint8_t* data, int64_t data_bytes, const vge_png_desc* descs, int n_descs,
                                     const vge_png_segment* segs, int64_t n_segs, int n_frames, int width, int height,
                                     int color_type, void* workspace, int64_t workspace_bytes, uint8_t* rgb,
                                     int32_t* status, void* stream) {
  if (n_descs < 0 || n_segs < 0 || n_segs >= (1ll << 31) || n_frames < 0 || data_bytes < 0 || workspace_bytes < 0 ||
      width < 1 || height < 1 || !(color_type == 0 || color_type == 2 || color_type == 4 || color_type == 6)) {
    set_last_error("vge_png_decode_device: bad argument (count, size or layout)");
    return VGE_PNG_ERR_ARG;
  }
  if (n_frames == 0) return VGE_PNG_OK;
  if (!status || ((uintptr_t)status & 3)) {
    set_last_error("vge_png_decode_device: bad argument (null or misaligned status)");
    return VGE_PNG_ERR_ARG;
  }
  if (n_descs > 0 && (!data || !descs || !workspace || !rgb || (n_segs > 0 && !segs) || ((uintptr_t)descs & 7) ||
                      ((uintptr_t)segs & 7) || ((uintptr_t)workspace & 15))) {
    set_last_error("vge_png_decode_device: bad argument (null or misaligned buffer)");
    return VGE_PNG_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, (size_t)n_frames * 4, s) != hipSuccess) {
    vge_gather::hip_failed("vge_png_decode_device");
    return VGE_PNG_ERR_HIP;
  }
  if (n_descs == 0) return VGE_PNG_OK;
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
  A.width = width;
  A.height = height;
  A.color_type = color_type;
  const int stages = g_stage_mask;
  if (n_segs > 0 && (stages & 1))
    hipLaunchKernelGGL(vge_gather::gather_kernel<Route>, dim3((unsigned)n_segs), dim3(WIDE), 0, s, A);
  if (stages & 2) hipLaunchKernelGGL(inflate_kernel<Route>, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  if (stages & 4) hipLaunchKernelGGL(adler_kernel<Route>, dim3((unsigned)n_descs), dim3(WIDE), 0, s, A);
  if (stages & 8) hipLaunchKernelGGL(unfilter_kernel, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  return vge_gather::hip_failed("vge_png_decode_device") ? VGE_PNG_ERR_HIP : VGE_PNG_OK;
}
