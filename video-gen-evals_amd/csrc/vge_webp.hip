// The device half of the lossless WebP front end (include/vge_webp.h): WebP files in device memory -> uint8 RGB
// frames, from the host's plan (csrc/vge_webp.cpp: one descriptor per frame, pointing at the frame's VP8L payload inside
// its file) and the file bytes alone.  There is no gather: a payload is contiguous.
//
//   entropy     one wave per frame.  The stream is read by the shared decoder of vge_webp_vp8l.h, the host's call,
//               with the colour cache, the code lengths being read and the current group's code headers in LDS and
//               the groups' tables, the transform data and the entropy image in the frame's slot.  VP8L's symbols
//               depend on each other through the prefix codes, the colour cache and the unbounded copy window, so the
//               stream is walked by one lane; a copy reads the slot the same lane wrote, so its loads follow its own
//               stores in program order and need no fence.  The group is looked up again at every tile boundary and
//               after every copy, the cache is updated pixel by pixel in stream order.  This is the plain form of the
//               kernel: correct on every stream the host accepts, and the part of the route that a batched decode
//               would speed up.
//   transforms  one wave per frame, the frame's transforms last to first.  The predictor runs a lane per row of a
//               64-row band, each lane two pixels behind the lane above: a lane keeps its last three pixels in
//               registers and hands them down as top-right, top and top-left by a shuffle, so no lane reads memory
//               another lane of the band wrote; the band's first row reads the last row of the band before it from
//               the slot, after a block fence and barrier.  The rightmost column's top-right is the row's own first
//               pixel.  Cross-colour, add-green and palette unbundling are pointwise.
//   compose     vge_compose.h's kernel, with vge_webp_vp8l.h's compose_pixel, the host's call, on an RGBA canvas
//               pixel; it is the step that needs the frame before, whose disposal it applies.
//
// The hard rules are vge_compose.h's, and hold for the entropy and transform kernels as well: a frame reads only its
// own payload and writes only its own slot, every loop consumes input bits or produces output, a bad stream sets the
// frame's status and ends the frame, and what the entropy kernel leaves for the transforms is checked again before it
// is used.
#include <hip/hip_runtime.h>

#include "../../include/vge_webp.h"
#include "vge_compose.h"
#include "vge_error.h"
#include "vge_webp_vp8l.h"

namespace {

using namespace vge_webp;
using vge::set_last_error;

using vge_compose::reachable;
using vge_gather::WAVE;
using vge_gather::WIDE;

struct Args {
  const uint8_t* data;
  int64_t data_bytes;
  const vge_webp_desc* descs;
  uint8_t* ws;
  int64_t ws_bytes;
  uint8_t* rgb;
  int32_t* status;
  int32_t n_descs, n_frames, n_files, width, height;
};

// 0: run it; -1: an unused slot (or nobody to report to); else the plan's code, or the code of a descriptor that does
// not fit the call.
__device__ int check_desc(const Args& A, const vge_webp_desc& d) {
  if (d.frame < 0 || d.frame >= A.n_frames) return -1;
  if (d.plan_status != 0) return d.plan_status > 0 ? d.plan_status : VGE_WEBP_ERR_ARG;
  if (d.file_off < 0 || d.file_bytes < 0 || d.file_bytes >= (1ll << 28) || d.file_off > A.data_bytes ||
      d.file_bytes > A.data_bytes - d.file_off)
    return VGE_WEBP_ERR_ARG;
  if (d.pay_off < 0 || d.pay_bytes < 0 || d.pay_off > d.file_bytes || d.pay_bytes > d.file_bytes - d.pay_off)
    return VGE_WEBP_ERR_ARG;
  if (d.w < 1 || d.h < 1 || d.x < 0 || d.y < 0 || d.w > A.width || d.h > A.height || d.x > A.width - d.w ||
      d.y > A.height - d.h || d.index < 0)
    return VGE_WEBP_ERR_ARG;
  const int64_t bytes = slot_layout(d.w, d.h).bytes;
  if (d.slot_off < 0 || (d.slot_off & 15) || d.slot_off > A.ws_bytes || bytes > A.ws_bytes - d.slot_off)
    return VGE_WEBP_ERR_ARG;
  return 0;
}

__device__ inline void fail(const Args& A, int frame, int code) {
  if (threadIdx.x == 0) atomicCAS(&A.status[frame], 0, code);
}

// What the shared compose kernel (vge_compose.h) needs of this route.
struct Route {
  using Args = ::Args;
  using Pixel = vge_webp::Pixel;
  static constexpr int ERR_ARG = VGE_WEBP_ERR_ARG;
  static __device__ int check_desc(const Args& A, const vge_webp_desc& d) { return ::check_desc(A, d); }
  static __device__ Pixel first_pixel(const vge_webp_desc&) { return Pixel{0, 0}; }
  static __device__ void step(Pixel& P, const Args& A, const vge_webp_desc& d, const vge_webp_desc& prev, int px,
                              int py) {
    compose_pixel(P, d, prev, px, py, reinterpret_cast<const uint32_t*>(A.ws + d.slot_off));
  }
};

__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ __launch_bounds__(WAVE) void entropy_kernel(Args A) {
  __shared__ Scratch S;
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_webp_desc d = A.descs[blockIdx.x];
  const int chk = check_desc(A, d);
  if (chk < 0) return;
  if (chk > 0) return fail(A, d.frame, chk);
  if (!reachable(A, (int)blockIdx.x)) return fail(A, d.frame, VGE_WEBP_ERR_ARG);
  if (threadIdx.x != 0) return;
  uint8_t* slot = A.ws + d.slot_off;
  const SlotLayout L = slot_layout(d.w, d.h);
  const int r = decode_entropy(A.data + d.file_off + d.pay_off, (uint32_t)d.pay_bytes, d.w, d.h,
                               reinterpret_cast<uint32_t*>(slot + L.plane_a),
                               reinterpret_cast<uint32_t*>(slot + L.plane_b), slot_arena(slot, d.w, d.h), S, nullptr);
  if (r != 0) atomicCAS(&A.status[d.frame], 0, r);
}

// What the entropy kernel left in the slot, checked before the transforms index with it.
__device__ bool header_ok(const FrameHdr& H, int w, int h, uint32_t sub_cap) {
  if (H.n_xforms < 0 || H.n_xforms > 4) return false;
  int xs = w;
  bool indexed = false;
  for (int i = 0; i < H.n_xforms; ++i) {
    const Xform& X = H.x[i];
    if (X.xsize != xs || X.data_off < 0) return false;
    if (X.type == T_PREDICTOR || X.type == T_CROSS_COLOR) {
      if (X.bits < 2 || X.bits > 9) return false;
      if ((int64_t)X.data_off + (int64_t)sub_size(xs, X.bits) * sub_size(h, X.bits) > sub_cap) return false;
    } else if (X.type == T_INDEXING) {
      if (X.bits < 0 || X.bits > 3 || indexed || (int64_t)X.data_off + 256 > sub_cap) return false;
      indexed = true;
      xs = sub_size(xs, X.bits);
    } else if (X.type != T_SUB_GREEN) {
      return false;
    }
  }
  return H.xsize == xs && (H.in_b != 0) == indexed;
}

// The predictor on `cur` (xs * h) in place: a lane per row of a band, two pixels behind the lane above.
__device__ void predictor_inverse(uint32_t* cur, int xs, int h, const uint32_t* data, int bits) {
  const int lane = threadIdx.x;
  const int tiles = sub_size(xs, bits);
  for (int y0 = 0; y0 < h; y0 += WAVE) {
    const int y = y0 + lane;
    const bool have_row = y < h;
    uint32_t* row = cur + (int64_t)(have_row ? y : 0) * xs;
    uint32_t h0 = 0, h1 = 0, h2 = 0;  // the lane's pixels x - 1, x - 2, x - 3
    uint32_t first = 0;
    const int steps = xs + 2 * (WAVE - 1);
    for (int t = 0; t < steps; ++t) {
      const int x = t - 2 * lane;
      // the lane above is at x + 2: its last three pixels are this pixel's top-right, top and top-left
      uint32_t TR = __shfl_up(h0, 1), T = __shfl_up(h1, 1), TL = __shfl_up(h2, 1);
      uint32_t out = 0;
      if (have_row && x >= 0 && x < xs) {
        if (lane == 0 && y > 0) {  // the band before this one is in memory (fenced below)
          const uint32_t* up = row - xs;
          T = up[x];
          TL = x > 0 ? up[x - 1] : 0;
          TR = x + 1 < xs ? up[x + 1] : 0;
        }
        if (x + 1 == xs) TR = first;  // the pixel after the top one in memory: this row's first
        uint32_t pred;
        if (y == 0) pred = x == 0 ? 0xff000000u : h0;
        else if (x == 0) pred = T;
        else pred = predict((int)((data[(int64_t)(y >> bits) * tiles + (x >> bits)] >> 8) & 0xf), h0, T, TL, TR);
        out = add_pixels(row[x], pred);
        row[x] = out;
        if (x == 0) first = out;
      }
      h2 = h1;
      h1 = h0;
      h0 = out;
    }
    __threadfence_block();  // the band's last row is read by lane 0 of the next band
    __syncthreads();
  }
}

__global__ __launch_bounds__(WAVE) void transform_kernel(Args A) {
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_webp_desc d = A.descs[blockIdx.x];
  if (check_desc(A, d) != 0) return;
  if (uni(A.status[d.frame]) != 0) return;  // refused by the entropy kernel
  uint8_t* slot = A.ws + d.slot_off;
  const SlotLayout L = slot_layout(d.w, d.h);
  const Arena R = slot_arena(slot, d.w, d.h);
  uint32_t* plane_a = reinterpret_cast<uint32_t*>(slot + L.plane_a);
  uint32_t* plane_b = reinterpret_cast<uint32_t*>(slot + L.plane_b);
  const FrameHdr H = *R.hdr;
  if (!header_ok(H, d.w, d.h, R.sub_cap)) return fail(A, d.frame, VGE_WEBP_ERR_ARG);
  const int lane = threadIdx.x, h = d.h;
  uint32_t* cur = H.in_b ? plane_b : plane_a;
  for (int i = H.n_xforms - 1; i >= 0; --i) {
    const Xform X = H.x[i];
    const uint32_t* data = R.sub + X.data_off;
    const int xs = X.xsize, tiles = sub_size(xs, X.bits);
    const int64_t npix = (int64_t)xs * h;
    if (X.type == T_PREDICTOR) {
      predictor_inverse(cur, xs, h, data, X.bits);
    } else if (X.type == T_CROSS_COLOR) {
      for (int64_t q = lane; q < npix; q += WAVE) {
        const int y = (int)(q / xs), x = (int)(q % xs);
        cur[q] = cross_color_inverse(data[(int64_t)(y >> X.bits) * tiles + (x >> X.bits)], cur[q]);
      }
    } else if (X.type == T_SUB_GREEN) {
      for (int64_t q = lane; q < npix; q += WAVE) cur[q] = add_green(cur[q]);
    } else {
      const int in_xs = sub_size(xs, X.bits);
      for (int64_t q = lane; q < npix; q += WAVE) {
        const int y = (int)(q / xs), x = (int)(q % xs);
        plane_a[q] = unbundle(plane_b + (int64_t)y * in_xs, x, X.bits, data);
      }
      cur = plane_a;
    }
    __threadfence_block();  // the next transform reads what other lanes stored
    __syncthreads();
  }
}

}  // namespace

// For tools/bench_frames.py, which times the kernels one by one: bit 0 entropy, 1 transforms, 2 compose.
// Returns the previous mask; a negative mask only reads it.
static int g_stage_mask = 7;
extern "C" int vge_debug_webp_stage_mask(int mask) {
  const int prev = g_stage_mask;
  if (mask >= 0) g_stage_mask = mask & 7;
  return prev;
}

extern "C" int vge_webp_decode_device(const uint8_t* data, int64_t data_bytes, const vge_webp_desc* descs, int n_descs,
                                      int n_frames, int n_files, int width, int height, void* workspace,
                                      int64_t workspace_bytes, uint8_t* rgb, int32_t* status, void* stream) {
  if (n_descs < 0 || n_frames < 0 || data_bytes < 0 || workspace_bytes < 0 || n_files < 0 || width < 1 || height < 1 ||
      width > 16384 || height > 16384) {
    set_last_error("vge_webp_decode_device: bad argument (count, size or canvas)");
    return VGE_WEBP_ERR_ARG;
  }
  if (n_frames == 0) return VGE_WEBP_OK;
  if (!status || ((uintptr_t)status & 3)) {
    set_last_error("vge_webp_decode_device: bad argument (null or misaligned status)");
    return VGE_WEBP_ERR_ARG;
  }
  if (n_descs > 0 && (!data || !descs || !workspace || !rgb || ((uintptr_t)descs & 7) || ((uintptr_t)workspace & 15))) {
    set_last_error("vge_webp_decode_device: bad argument (null or misaligned buffer)");
    return VGE_WEBP_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, (size_t)n_frames * 4, s) != hipSuccess) {
    vge_gather::hip_failed("vge_webp_decode_device");
    return VGE_WEBP_ERR_HIP;
  }
  if (n_descs == 0) return VGE_WEBP_OK;
  Args A;
  A.data = data;
  A.data_bytes = data_bytes;
  A.descs = descs;
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
  if (stages & 1) hipLaunchKernelGGL(entropy_kernel, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  if (stages & 2) hipLaunchKernelGGL(transform_kernel, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  if ((stages & 4) && n_files > 0)
    hipLaunchKernelGGL(vge_compose::compose_kernel<Route>,
                       dim3(pix_groups, (unsigned)(n_files < 65535 ? n_files : 65535)), dim3(WIDE), 0, s, A);
  return vge_gather::hip_failed("vge_webp_decode_device") ? VGE_WEBP_ERR_HIP : VGE_WEBP_OK;
}
