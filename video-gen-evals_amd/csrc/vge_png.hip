// The device half of the PNG frame front end (include/vge_png.h): PNG files in device memory -> uint8 RGB frames, from
// the host's plan (csrc/vge_png.cpp: one descriptor per frame, one segment per IDAT chunk) and the file bytes alone.
//
//   gather    one workgroup per segment copies an IDAT payload to its place in the frame's gathered run, so that the
//             bit reader sees one contiguous zlib stream however the writer cut it (Pillow: every 64 KiB; libpng: 8 KiB).
//             The kernel is vge_gather.h's, shared with the GIF route.
//   inflate   one wave per frame: the zlib header, then the shared core (vge_inflate_core.h) through its LDS ring into
//             the frame's slot of filtered rows -- whole dwords, and at the end the last 1-3 bytes as one masked dword
//             (slots are padded to a dword).  It reads on past the count as zlib does with one spare output byte, and
//             records whether the final block ended exactly at the count with a whole trailer behind it.
//   adler     one workgroup per frame whose trailer is to be checked: A = 1 + sum d_i, B = n + sum (n - i) d_i, both
//             mod 65521, as per-thread 64-bit partial sums (no term exceeds 2^24 and a frame has fewer than 2^31 bytes).
//   unfilter  one wave per frame.  Lane l owns row r0 + l of a 64-row band and at step s handles pixel s - l: "up" is
//             what lane l - 1 produced one step ago (one __shfl_up per step), "up-left" what it produced two steps ago
//             (the lane's own previous "up"), "left" the lane's own last pixel.  A band costs width + 63 steps.  The
//             band's last row is written back over its filtered bytes in the slot, alpha included, and lane 0 of the
//             next band reads it from there (same workgroup, behind a barrier).
//
// Hard rules, the same as in vge_inflate.hip:
//   - every descriptor and segment is checked against the sizes the host passed (data_bytes, workspace_bytes, n_frames,
//     the layout) before anything is read or written through it;
//   - a frame reads only its own file bytes, writes only its own workspace run and slot and its own output rows;
//   - every loop consumes input or produces output;
//   - a frame that fails sets its own status (atomicCAS from 0: the first failure wins) and touches nothing else;
//   - no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vge_png.h"
#include "vge_error.h"
#include "vge_gather.h"
#include "vge_inflate_core.h"

namespace {

using namespace vge_inflate;
using vge::set_last_error;

constexpr int BAND = WAVE;       // rows per unfilter band: one per lane
constexpr int WIDE = vge_gather::WIDE;  // threads of the gather and Adler workgroups
constexpr uint32_t ADLER_MOD = 65521;

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

// What the inflate kernel leaves for the Adler kernel, one per descriptor at the start of the workspace.
struct Record {
  uint32_t check;     // 1: the trailer is whole and directly follows a final block that ended at the count
  uint32_t expected;  // its value
};

__host__ __device__ inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
__host__ __device__ inline int bytes_per_pixel(int ct) { return ct == 0 ? 1 : ct == 2 ? 3 : ct == 4 ? 2 : 4; }

// 0: run it; -1: an unused slot (or nobody to report to); else the code of a descriptor that does not fit the call.
__device__ int check_desc(const Args& A, const vge_png_desc& d) {
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

__device__ inline void fail(const Args& A, int frame, int code) {
  if (threadIdx.x == 0) atomicCAS(&A.status[frame], 0, code);
}

// What the shared gather kernel (vge_gather.h) needs of this route.
struct Route {
  using Args = ::Args;
  static constexpr int ERR_ARG = VGE_PNG_ERR_ARG;
  static __device__ int check_desc(const Args& A, const vge_png_desc& d) { return ::check_desc(A, d); }
  static __device__ void fail(const Args& A, int frame, int code) { ::fail(A, frame, code); }
};

__global__ __launch_bounds__(WAVE) void inflate_kernel(Args A) {
  __shared__ Shared S;
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_png_desc d = A.descs[blockIdx.x];
  const int chk = check_desc(A, d);
  if (chk < 0) return;
  if (chk > 0) return fail(A, d.frame, chk);
  if (uni((uint32_t)A.status[d.frame]) != 0) return;  // a segment of the frame was refused
  Record* rec = reinterpret_cast<Record*>(A.ws) + blockIdx.x;
  if (threadIdx.x == 0) *rec = Record{0, 0};
  const uint8_t* g = A.ws + d.gat_off;
  if (d.gat_bytes < 2) return fail(A, d.frame, VGE_PNG_ERR_IO);
  const uint32_t cmf = g[0], flg = g[1];
  if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20))
    return fail(A, d.frame, VGE_PNG_ERR_IO);

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
  if (end == STREAM_FAIL) return fail(A, d.frame, VGE_PNG_ERR_IO);
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
  const vge_png_desc d = A.descs[blockIdx.x];
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
    if (((fb << 16) | fa) != rec.expected) atomicCAS(&A.status[d.frame], 0, VGE_PNG_ERR_IO);
  }
}

__device__ inline int paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

__global__ __launch_bounds__(WAVE) void unfilter_kernel(Args A) {
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_png_desc d = A.descs[blockIdx.x];
  if (check_desc(A, d) != 0 || uni((uint32_t)A.status[d.frame]) != 0) return;
  const int lane = threadIdx.x, W = A.width, H = A.height, bpp = bytes_per_pixel(A.color_type);
  const bool grey = bpp < 3;
  const int64_t stride = 1 + (int64_t)W * bpp;
  uint8_t* slot = A.ws + d.slot_off;
  uint8_t* out_frame = A.rgb + (int64_t)d.frame * H * W * 3;
  for (int r0 = 0; r0 < H; r0 += BAND) {
    const int row = r0 + lane;
    const bool active = row < H;
    uint8_t* rowp = slot + (active ? row : 0) * stride;
    const int ft = active ? rowp[0] : 0;
    if (__any(ft > 4)) return fail(A, d.frame, VGE_PNG_ERR_IO);
    const uint8_t* carried = r0 > 0 ? slot + (int64_t)(r0 - 1) * stride + 1 : nullptr;  // the band above's last row
    const bool carry_out = lane == BAND - 1 && r0 + BAND < H;
    uint8_t* out_row = out_frame + (int64_t)(active ? row : 0) * W * 3;
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
        if (carry_out) rowp[1 + x * bpp + c] = (uint8_t)v;
      }
      left = px;
      last = px;
      out_row[3 * x] = (uint8_t)px;
      out_row[3 * x + 1] = (uint8_t)(grey ? px : px >> 8);
      out_row[3 * x + 2] = (uint8_t)(grey ? px : px >> 16);
    }
    __syncthreads();  // the carried row is in memory before lane 0 of the next band reads it
  }
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
    set_last_error(std::string("vge_png_decode_device: ") + hipGetErrorString(hipGetLastError()));
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
  if (stages & 2) hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  if (stages & 4) hipLaunchKernelGGL(adler_kernel, dim3((unsigned)n_descs), dim3(WIDE), 0, s, A);
  if (stages & 8) hipLaunchKernelGGL(unfilter_kernel, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error(std::string("vge_png_decode_device: ") + hipGetErrorString(e));
    return VGE_PNG_ERR_HIP;
  }
  return VGE_PNG_OK;
}
