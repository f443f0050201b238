// The device half of the APNG video front end (include/vge_apng.h): APNG files in device memory -> uint8 RGB frames,
// from the host's plan (csrc/vge_apng.cpp: one descriptor per frame, one segment per IDAT / fdAT payload) and the file
// bytes alone.
//
//   gather    vge_gather.h's kernel, shared with the PNG and GIF routes: each frame's payloads (the plan has stepped
//             over the fdAT sequence numbers) into one run of the workspace.
//   inflate   one wave per frame: the zlib header, then the shared core (vge_inflate_core.h) through its LDS ring into
//             the frame's slot, with the frame's own count h * (1 + w * bytes_per_pixel).  As in vge_png.hip it reads
//             on past the count and records whether a whole trailer follows a final block that ended at the count.
//   adler     one workgroup per frame whose trailer is to be checked, as in vge_png.hip.
//   unfilter  one wave per frame, lane l on row r0 + l of a 64-row band, one pixel behind lane l - 1 (vge_png.hip
//             explains the scheme).  Width, height and stride are the rectangle's; every reconstructed byte goes back
//             over its filtered byte, so that the slot holds the raw pixels of the file's colour type, alpha included.
//   compose   a row of workgroups per file (the file's first descriptor is found by a binary search on the owner
//             field), a lane per canvas pixel: it walks the file's frames in order with the canvas value and the value
//             that dispose PREVIOUS / BACKGROUND puts back in registers (vge_apng_px.h compose_pixel, the host's call)
//             and stores RGB for every frame.  It stops at the first frame whose status is set and gives the later
//             frames that status.
//
// Hard rules, the same as in vge_png.hip and vge_gif.hip:
//   - every descriptor and segment is checked against the sizes the host passed (data_bytes, workspace_bytes, n_frames,
//     the canvas, the colour type) before anything is read or written through it;
//   - a frame reads only its own file bytes and gathered run, writes only its own slot and its own output frame;
//   - every loop consumes input or produces output;
//   - a frame that fails sets its own status (atomicCAS from 0: the first failure wins);
//   - no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vge_apng.h"
#include "vge_apng_px.h"
#include "vge_error.h"
#include "vge_gather.h"
#include "vge_inflate_core.h"

namespace {

using namespace vge_inflate;
using vge::set_last_error;
using vge_apng::bytes_per_pixel;

constexpr int BAND = WAVE;              // rows per unfilter band: one per lane
constexpr int WIDE = vge_gather::WIDE;  // threads of the gather, Adler and compose workgroups
constexpr uint32_t ADLER_MOD = 65521;

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

// What the inflate kernel leaves for the Adler kernel, one per descriptor at the start of the workspace.
struct Record {
  uint32_t check;     // 1: the trailer is whole and directly follows a final block that ended at the count
  uint32_t expected;  // its value
};

__host__ __device__ inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// 0: run it; -1: an unused slot (or nobody to report to); else the plan's code, or the code of a descriptor that does
// not fit the call.
__device__ int check_desc(const Args& A, const vge_apng_desc& d) {
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

__device__ inline void fail(const Args& A, int frame, int code) {
  if (threadIdx.x == 0) atomicCAS(&A.status[frame], 0, code);
}

struct Route {
  using Args = ::Args;
  static constexpr int ERR_ARG = VGE_APNG_ERR_ARG;
  static __device__ int check_desc(const Args& A, const vge_apng_desc& d) { return ::check_desc(A, d); }
  static __device__ void fail(const Args& A, int frame, int code) { ::fail(A, frame, code); }
};

// The first descriptor whose file is not below f (the plan emits files in increasing order); n_descs when there is none.
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
__device__ inline bool continues(const vge_apng_desc& prev, const vge_apng_desc& d) {
  return prev.file == d.file && d.index > 0 && prev.index == d.index - 1;
}

// The compose kernel reaches descriptor k when the chain it belongs to starts at index 0 and that start is where the
// search for its file lands.  Anything else is a descriptor array the plan does not emit: the frame is refused by the
// inflate kernel, so that no frame is left with status 0 and no pixels.
__device__ bool reachable(const Args& A, int k) {
  int j = k;
  while (j > 0 && continues(A.descs[j - 1], A.descs[j])) --j;  // at most `index` steps
  const vge_apng_desc h = A.descs[j];
  return h.index == 0 && h.file >= 0 && h.file < A.n_files && lower_bound_file(A, h.file) == j;
}

__global__ __launch_bounds__(WAVE) void inflate_kernel(Args A) {
  __shared__ Shared S;
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_apng_desc d = A.descs[blockIdx.x];
  const int chk = check_desc(A, d);
  if (chk < 0) return;
  if (chk > 0) return fail(A, d.frame, chk);
  if (!reachable(A, (int)blockIdx.x)) return fail(A, d.frame, VGE_APNG_ERR_ARG);
  if (uni((uint32_t)A.status[d.frame]) != 0) return;  // a segment of the frame was refused
  Record* rec = reinterpret_cast<Record*>(A.ws) + blockIdx.x;
  if (threadIdx.x == 0) *rec = Record{0, 0};
  const uint8_t* g = A.ws + d.gat_off;
  if (d.gat_bytes < 2) return fail(A, d.frame, VGE_APNG_ERR_IO);
  const uint32_t cmf = g[0], flg = g[1];
  if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20))
    return fail(A, d.frame, VGE_APNG_ERR_IO);

  Reader R;
  R.src = g + 2;
  R.csize = (int32_t)(d.gat_bytes - 2);
  R.bp = 0;
  R.cached = false;
  R.cbit = 0;
  R.cache = 0;
  uint32_t* slot = reinterpret_cast<uint32_t*>(A.ws + d.slot_off);
  const int64_t total = d.raw_bytes;
  int64_t flushed;
  const int end = inflate_stream<true>(R, S, DwordSink{slot, 0}, total, &flushed);
  if (end == STREAM_FAIL) return fail(A, d.frame, VGE_APNG_ERR_IO);
  if (threadIdx.x == 0) {
    if (flushed < total)  // the last 1-3 bytes: one dword, zero beyond the count (the slot is padded)
      slot[flushed >> 2] = ring_dword(S, (uint32_t)flushed) & (0xffffffffu >> (8 * (4 - (int)(total - flushed))));
    const int64_t tb = ((int64_t)R.bp + 7) >> 3;
    if (end == STREAM_ENDED && tb + 4 <= R.csize) {
      const uint8_t* t = R.src + tb;
      *rec = Record{1, ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | (uint32_t)t[3]};
    }
  }
}

__global__ __launch_bounds__(WIDE) void adler_kernel(Args A) {
  __shared__ uint64_t sa[WIDE], sb[WIDE];
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_apng_desc d = A.descs[blockIdx.x];
  if (check_desc(A, d) != 0 || A.status[d.frame] != 0) return;
  const Record rec = reinterpret_cast<const Record*>(A.ws)[blockIdx.x];
  if (rec.check != 1) return;
  const uint32_t* slot = reinterpret_cast<const uint32_t*>(A.ws + d.slot_off);
  const int64_t n = d.raw_bytes, n_dw = (n + 3) >> 2;
  uint64_t a = 0, b = 0;
  for (int64_t k = threadIdx.x; k < n_dw; k += WIDE) {
    const uint32_t v = slot[k];
    for (int j = 0; j < 4; ++j) {
      const int64_t i = 4 * k + j;
      if (i < n) {
        const uint32_t byte = (v >> (8 * j)) & 255u;
        a += byte;
        b += (uint64_t)((n - i) % ADLER_MOD) * byte;
      }
    }
  }
  sa[threadIdx.x] = a;
  sb[threadIdx.x] = b % ADLER_MOD;
  __syncthreads();
  for (int w = WIDE / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      sa[threadIdx.x] += sa[threadIdx.x + w];
      sb[threadIdx.x] += sb[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const uint32_t fa = (uint32_t)((1 + sa[0]) % ADLER_MOD), fb = (uint32_t)(((uint64_t)n + sb[0]) % ADLER_MOD);
    if (((fb << 16) | fa) != rec.expected) atomicCAS(&A.status[d.frame], 0, VGE_APNG_ERR_IO);
  }
}

__device__ inline int paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

__global__ __launch_bounds__(WAVE) void unfilter_kernel(Args A) {
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_apng_desc d = A.descs[blockIdx.x];
  if (check_desc(A, d) != 0 || uni((uint32_t)A.status[d.frame]) != 0) return;
  const int lane = threadIdx.x, W = d.w, H = d.h, bpp = bytes_per_pixel(A.color_type);
  const int64_t stride = 1 + (int64_t)W * bpp;
  uint8_t* slot = A.ws + d.slot_off;
  for (int r0 = 0; r0 < H; r0 += BAND) {
    const int row = r0 + lane;
    const bool active = row < H;
    uint8_t* rowp = slot + (active ? row : 0) * stride;
    const int ft = active ? rowp[0] : 0;
    if (__any(ft > 4)) return fail(A, d.frame, VGE_APNG_ERR_IO);
    const uint8_t* carried = r0 > 0 ? slot + (int64_t)(r0 - 1) * stride + 1 : nullptr;  // the band above's last row
    uint32_t left = 0, up = 0, last = 0;  // pixels, channel c in bits [8c, 8c + 8)
    const int64_t steps = (int64_t)W + BAND - 1;
    for (int64_t s = 0; s < steps; ++s) {
      const int64_t x = s - lane;
      const bool on = active && x >= 0 && x < W;
      uint32_t above = __shfl_up(last, 1);
      if (lane == 0) {
        above = 0;
        if (on && carried)
          for (int c = 0; c < bpp; ++c) above |= (uint32_t)carried[x * bpp + c] << (8 * c);
      }
      uint32_t upleft = up;
      up = above;
      if (!on) continue;
      if (x == 0) {
        upleft = 0;
        left = 0;
      }
      uint32_t px = 0;
      for (int c = 0; c < bpp; ++c) {
        const int a = (left >> (8 * c)) & 255, b = (up >> (8 * c)) & 255, cc = (upleft >> (8 * c)) & 255;
        const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, cc);
        const uint32_t v = (uint32_t)(rowp[1 + x * bpp + c] + pred) & 255u;
        px |= v << (8 * c);
        rowp[1 + x * bpp + c] = (uint8_t)v;
      }
      left = px;
      last = px;
    }
    __syncthreads();  // the band's last row is in memory before lane 0 of the next band reads it
  }
}

__global__ __launch_bounds__(WIDE) void compose_kernel(Args A) {
  const int64_t npix = (int64_t)A.width * A.height;
  const int64_t pix = (int64_t)blockIdx.x * WIDE + threadIdx.x;
  const bool active = pix < npix;
  const int px = (int)(pix % A.width), py = (int)(pix / A.width);
  const bool reporter = blockIdx.x == 0 && threadIdx.x == 0;
  for (int f = blockIdx.y; f < A.n_files; f += gridDim.y) {  // a row of workgroups per file
    const int k0 = lower_bound_file(A, f);
    if (k0 >= A.n_descs) continue;
    const vge_apng_desc d0 = A.descs[k0];
    // a file without frames; a headless chain was refused by the inflate kernel
    if (d0.file != f || d0.index != 0) continue;
    vge_apng::Pixel P{0, 0, 0};
    int carried = 0;
    for (int k = k0; k < A.n_descs; ++k) {
      const vge_apng_desc d = A.descs[k];
      if (k > k0 && !continues(A.descs[k - 1], d)) break;
      const int chk = check_desc(A, d);
      if (chk < 0) {  // an unused slot inside a file: nobody to report to, and the later frames are deltas on it
        if (carried == 0) carried = VGE_APNG_ERR_ARG;
        continue;
      }
      if (carried == 0) carried = chk > 0 ? chk : A.status[d.frame];
      if (carried != 0) {
        if (reporter) atomicCAS(&A.status[d.frame], 0, carried);
        continue;
      }
      if (!active) continue;
      vge_apng::compose_pixel(P, d, px, py, A.ws + d.slot_off);
      uint8_t* o = A.rgb + ((int64_t)d.frame * npix + pix) * 3;
      o[0] = (uint8_t)P.canvas;
      o[1] = (uint8_t)(P.canvas >> 8);
      o[2] = (uint8_t)(P.canvas >> 16);
    }
  }
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
    set_last_error(std::string("vge_apng_decode_device: ") + hipGetErrorString(hipGetLastError()));
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
  if (stages & 2) hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  if (stages & 4) hipLaunchKernelGGL(adler_kernel, dim3((unsigned)n_descs), dim3(WIDE), 0, s, A);
  if (stages & 8) hipLaunchKernelGGL(unfilter_kernel, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  if ((stages & 16) && n_files > 0)
    hipLaunchKernelGGL(compose_kernel, dim3((unsigned)pix_groups, (unsigned)(n_files < 65535 ? n_files : 65535)),
                       dim3(WIDE), 0, s, A);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error(std::string("vge_apng_decode_device: ") + hipGetErrorString(e));
    return VGE_APNG_ERR_HIP;
  }
  return VGE_APNG_OK;
}
