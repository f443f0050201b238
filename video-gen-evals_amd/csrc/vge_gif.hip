// The device half of the GIF video front end (include/vge_gif.h): GIF files in device memory -> uint8 RGB frames, from
// the host's plan (csrc/vge_gif.cpp: one descriptor per frame, one segment per data sub-block) and the file bytes alone.
//
//   gather    vge_gather.h's kernel: each frame's sub-blocks into one run of the workspace.
//   lzw       one wave per frame, the dictionary (4096 entries of 8 bytes) in LDS.  A batch is the next 64 codes: their
//             widths depend only on how many codes were read since the last clear code, so lane l knows the width of
//             code l, a wave scan gives its bit position, and all 64 are read at once.  A ballot finds the first clear
//             or end code (or the end of the data) and cuts the batch there.  The codes in front of the cut then go
//             through the shared per-code step (vge_gif_lzw.h: validity, entry insertion) one after the other, the
//             same call the host decoder makes, executed by the whole wave on wave-uniform values; its running sum of
//             string lengths is each code's output position.  Then every lane expands its own code: it walks the
//             (prefix, suffix) chain backwards from LDS and stores the string's bytes last to first.
//   compose   vge_compose.h's kernel, with vge_gif_lzw.h's compose_pixel, the host's call, which looks colours up in
//             the file bytes; a file's canvas starts as its first descriptor's first_rgb.
//
// The hard rules are vge_compose.h's, and hold for the LZW kernel as well: a frame reads only its own gathered run and
// writes only its own slot, every loop consumes input bits or produces output (the chain walk is bounded by the
// string's length), and a bad code sets the frame's status and ends the frame.
#include <hip/hip_runtime.h>

#include "../../include/vge_gif.h"
#include "vge_compose.h"
#include "vge_error.h"
#include "vge_gather.h"
#include "vge_gif_lzw.h"

namespace {

using namespace vge_gif;
using vge::set_last_error;

using vge_compose::reachable;
using vge_gather::WAVE;
using vge_gather::WIDE;

struct Args {
  const uint8_t* data;
  int64_t data_bytes;
  const vge_gif_desc* descs;
  const vge_gif_segment* segs;
  int64_t n_segs;
  uint8_t* ws;
  int64_t ws_bytes;
  uint8_t* rgb;
  int32_t* status;
  int32_t n_descs, n_frames, n_files, width, height;
};

// 0: run it; -1: an unused slot (or nobody to report to); else the plan's code, or the code of a descriptor that does
// not fit the call.
__device__ int check_desc(const Args& A, const vge_gif_desc& d) {
  if (d.frame < 0 || d.frame >= A.n_frames) return -1;
  if (d.plan_status != 0) return d.plan_status > 0 ? d.plan_status : VGE_GIF_ERR_ARG;
  if (d.file_off < 0 || d.file_bytes < 0 || d.file_bytes >= (1ll << 28) || d.file_off > A.data_bytes ||
      d.file_bytes > A.data_bytes - d.file_off)
    return VGE_GIF_ERR_ARG;
  if (d.w < 1 || d.h < 1 || d.x < 0 || d.y < 0 || d.w > A.width || d.h > A.height || d.x > A.width - d.w ||
      d.y > A.height - d.h)
    return VGE_GIF_ERR_ARG;
  if (d.min_code_size < 2 || d.min_code_size > 8 || d.transparent < -1 || d.transparent > 255 || d.index < 0)
    return VGE_GIF_ERR_ARG;
  if (d.ct_size < 1 || d.ct_size > 256 || d.ct_off < 0 || d.ct_off > d.file_bytes ||
      (int64_t)d.ct_size * 3 > d.file_bytes - d.ct_off)
    return VGE_GIF_ERR_ARG;
  if (d.gat_off < 0 || d.gat_bytes < 0 || d.gat_bytes >= (1ll << 28) || d.gat_off > A.ws_bytes ||
      d.gat_bytes > A.ws_bytes - d.gat_off)
    return VGE_GIF_ERR_ARG;
  const int64_t plane = (int64_t)d.w * d.h;
  if (plane >= (1ll << 31) || d.slot_off < 0 || (d.slot_off & 15) || d.slot_off > A.ws_bytes ||
      plane > A.ws_bytes - d.slot_off)
    return VGE_GIF_ERR_ARG;
  return 0;
}

__device__ inline void fail(const Args& A, int frame, int code) {
  if (threadIdx.x == 0) atomicCAS(&A.status[frame], 0, code);
}

// What the shared kernels (vge_gather.h, vge_compose.h) need of this route.
struct Route {
  using Args = ::Args;
  using Pixel = vge_gif::Pixel;
  static constexpr int ERR_ARG = VGE_GIF_ERR_ARG;
  static __device__ int check_desc(const Args& A, const vge_gif_desc& d) { return ::check_desc(A, d); }
  static __device__ void fail(const Args& A, int frame, int code) { ::fail(A, frame, code); }
  static __device__ Pixel first_pixel(const vge_gif_desc& d0) { return Pixel{d0.first_rgb, 0, 0}; }
  static __device__ void step(Pixel& P, const Args& A, const vge_gif_desc& d, const vge_gif_desc&, int px, int py) {
    compose_pixel(P, d, px, py, A.ws + d.slot_off, A.data + d.file_off + d.ct_off);
  }
};

__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ __launch_bounds__(WAVE) void lzw_kernel(Args A) {
  __shared__ Entry table[TABLE];
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_gif_desc d = A.descs[blockIdx.x];
  const int chk = check_desc(A, d);
  if (chk < 0) return;
  if (chk > 0) return fail(A, d.frame, chk);
  if (!reachable(A, (int)blockIdx.x)) return fail(A, d.frame, VGE_GIF_ERR_ARG);
  if (uni(A.status[d.frame]) != 0) return;  // a segment of the frame was refused
  const int lane = threadIdx.x;
  const int mcs = d.min_code_size, clear = clear_code(mcs);
  for (int k = lane; k < clear + 2; k += WAVE) table[k] = initial_entry(mcs, k);
  __syncthreads();

  const uint8_t* g = A.ws + d.gat_off;
  const int64_t gbytes = d.gat_bytes;
  const uint32_t total_bits = (uint32_t)(gbytes * 8);  // gat_bytes < 2^28
  uint8_t* out = A.ws + d.slot_off;
  const int64_t count = (int64_t)d.w * d.h;
  Lzw L{mcs, 0, -1, 0, 0};
  uint32_t bitpos = 0;
  int64_t o = 0;
  while (o < count) {
    // the batch: lane l reads the l-th next code as if no clear code came before it in the batch
    const int width = code_width(mcs, L.since + lane);
    int end = width;  // inclusive scan of the widths
    for (int s = 1; s < WAVE; s <<= 1) {
      const int up = __shfl_up(end, s);
      if (lane >= s) end += up;
    }
    const uint32_t at = bitpos + (uint32_t)(end - width);  // < 2^31 + 768
    const bool have = at + (uint32_t)width <= total_bits;
    int code = -1;
    if (have) {
      const int64_t b = at >> 3;
      uint32_t v = g[b];
      if (b + 1 < gbytes) v |= (uint32_t)g[b + 1] << 8;
      if (b + 2 < gbytes) v |= (uint32_t)g[b + 2] << 16;
      code = (int)((v >> (at & 7)) & ((1u << width) - 1));
    }
    const unsigned long long cut = __ballot(!have || code == clear || code == clear + 1);
    const int m = cut ? __ffsll(cut) - 1 : WAVE;  // codes in front of the cut

    // the shared step, code after code, on wave-uniform values: every lane does the same and keeps its own code's result
    int my_code = -1, my_len = 0;
    int64_t my_out = 0;
    bool bad = false;
    for (int i = 0; i < m && o < count; ++i) {
      const int ci = __shfl(code, i);
      int len;
      if (lzw_step(L, table, ci, &len) != STEP_DATA) {
        bad = true;
        break;
      }
      if (i == lane) {
        my_code = ci;
        my_len = len;
        my_out = o;
      }
      o += len;
    }
    __syncthreads();
    if (bad) return fail(A, d.frame, VGE_GIF_ERR_IO);
    // expansion: the chain from LDS, last byte first; at most my_len <= 4096 links
    if (my_code >= 0) {
      int c = my_code;
      for (int k = my_len - 1; k >= 0; --k) {
        const Entry e = table[c & (TABLE - 1)];
        if (my_out + k < count) out[my_out + k] = e.suffix;
        c = e.prefix;
      }
    }
    __syncthreads();
    if (o >= count) break;
    if (m == WAVE) {
      bitpos += (uint32_t)__shfl(end, WAVE - 1);
      continue;
    }
    // the code at the cut: a clear code goes on, an end code or the end of the data before the count is the frame's end
    const int cm = __shfl(code, m);
    if (cm != clear) return fail(A, d.frame, VGE_GIF_ERR_IO);
    int len;
    lzw_step(L, table, cm, &len);
    bitpos += (uint32_t)__shfl(end, m);
  }
}

}  // namespace

// For tools/bench_frames.py, which times the kernels one by one: bit 0 gather, 1 lzw, 2 compose.
// Returns the previous mask; a negative mask only reads it.
static int g_stage_mask = 7;
extern "C" int vge_debug_gif_stage_mask(int mask) {
  const int prev = g_stage_mask;
  if (mask >= 0) g_stage_mask = mask & 7;
  return prev;
}

extern "C" int vge_gif_decode_device(const uint8_t* data, int64_t data_bytes, const vge_gif_desc* descs, int n_descs,
                                     const vge_gif_segment* segs, int64_t n_segs, int n_frames, int n_files, int width,
                                     int height, void* workspace, int64_t workspace_bytes, uint8_t* rgb, int32_t* status,
                                     void* stream) {
  if (n_descs < 0 || n_segs < 0 || n_segs >= (1ll << 31) || n_frames < 0 || data_bytes < 0 || workspace_bytes < 0 ||
      n_files < 0 || width < 1 || height < 1 || width > 65535 || height > 65535) {
    set_last_error("vge_gif_decode_device: bad argument (count, size or screen)");
    return VGE_GIF_ERR_ARG;
  }
  if (n_frames == 0) return VGE_GIF_OK;
  if (!status || ((uintptr_t)status & 3)) {
    set_last_error("vge_gif_decode_device: bad argument (null or misaligned status)");
    return VGE_GIF_ERR_ARG;
  }
  if (n_descs > 0 && (!data || !descs || !workspace || !rgb || (n_segs > 0 && !segs) || ((uintptr_t)descs & 7) ||
                      ((uintptr_t)segs & 7) || ((uintptr_t)workspace & 15))) {
    set_last_error("vge_gif_decode_device: bad argument (null or misaligned buffer)");
    return VGE_GIF_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, (size_t)n_frames * 4, s) != hipSuccess) {
    vge_gather::hip_failed("vge_gif_decode_device");
    return VGE_GIF_ERR_HIP;
  }
  if (n_descs == 0) return VGE_GIF_OK;
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
  const int stages = g_stage_mask;
  const unsigned pix_groups = (unsigned)(((int64_t)width * height + WIDE - 1) / WIDE);
  if (n_segs > 0 && (stages & 1))
    hipLaunchKernelGGL(vge_gather::gather_kernel<Route>, dim3((unsigned)n_segs), dim3(WIDE), 0, s, A);
  if (stages & 2) hipLaunchKernelGGL(lzw_kernel, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  if ((stages & 4) && n_files > 0)
    hipLaunchKernelGGL(vge_compose::compose_kernel<Route>,
                       dim3(pix_groups, (unsigned)(n_files < 65535 ? n_files : 65535)), dim3(WIDE), 0, s, A);
  return vge_gather::hip_failed("vge_gif_decode_device") ? VGE_GIF_ERR_HIP : VGE_GIF_OK;
}
