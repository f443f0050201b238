// The kernels of the device decoders whose frames are zlib streams of PNG-filtered rows (vge_png.hip: a whole image per
// frame; vge_apng.hip: a rectangle per frame), after vge_gather.h's kernel has made each frame's stream contiguous.
//
//   inflate   one wave per frame: the zlib header, then the shared core (vge_inflate_core.h) through its LDS ring into
//             the frame's slot of filtered rows -- whole dwords, and at the end the last 1-3 bytes as one masked dword
//             (slots are padded to a dword).  It reads on past the count as zlib does with one spare output byte, and
//             records whether the final block ended exactly at the count with a whole trailer behind it.
//   adler     one workgroup per frame whose trailer is to be checked: A = 1 + sum d_i, B = n + sum (n - i) d_i, both
//             mod 65521, as per-thread 64-bit partial sums (no term exceeds 2^24 and a frame has fewer than 2^31 bytes).
//   unfilter  one wave per frame.  Lane l owns row r0 + l of a 64-row band and at step s handles pixel s - l: "up" is
//             what lane l - 1 produced one step ago (one __shfl_up per step), "up-left" what it produced two steps ago
//             (the lane's own previous "up"), "left" the lane's own last pixel.  A band costs width + 63 steps.  Where
//             a reconstructed pixel goes is the caller's sink; lane 0 of the next band reads the band's last row back
//             from the slot (same workgroup, behind a barrier), so the sink puts at least that row there.
//
// Hard rules, the same as in vge_inflate.hip:
//   - every descriptor is checked against the sizes the host passed (Route::check_desc) before anything is read or
//     written through it;
//   - a frame reads only its own gathered run, writes only its own record and slot and what its sink owns;
//   - every loop consumes input or produces output;
//   - a frame that fails sets its own status (atomicCAS from 0: the first failure wins) and touches nothing else;
//   - no workgroup waits for another.
//
// Beyond what vge_gather.h asks of it, Route supplies:
//   Route::Args          also with status, ws and n_descs; descriptors with raw_bytes and slot_off (16-aligned, padded
//                        to a dword, behind the records: check_desc sees to it)
//   Route::ERR_IO        the code of a stream that is not zlib's, does not inflate, fails its Adler sum or names a filter
//                        type above 4
//   Route::runs          whether descriptor k, which fits the call, is one the later kernels reach
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vge_gather.h"
#include "vge_inflate_core.h"

namespace vge_png_kernels {

using vge_gather::WAVE;
using vge_gather::WIDE;
static_assert(vge_inflate::WAVE == WAVE, "the inflate core runs on one wavefront");
constexpr int BAND = WAVE;  // rows per unfilter band: one per lane
constexpr uint32_t ADLER_MOD = 65521;

// What the inflate kernel leaves for the Adler kernel, one per descriptor at the start of the workspace.
struct Record {
  uint32_t check;     // 1: the trailer is whole and directly follows a final block that ended at the count
  uint32_t expected;  // its value
};

__host__ __device__ inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

template <class Route>
__global__ __launch_bounds__(WAVE) void inflate_kernel(typename Route::Args A) {
  using namespace vge_inflate;
  __shared__ Shared S;
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const auto d = A.descs[blockIdx.x];
  const int chk = Route::check_desc(A, d);
  if (chk < 0) return;
  if (chk > 0) return Route::fail(A, d.frame, chk);
  if (!Route::runs(A, (int)blockIdx.x)) return Route::fail(A, d.frame, Route::ERR_ARG);
  if (uni((uint32_t)A.status[d.frame]) != 0) return;  // a segment of the frame was refused
  Record* rec = reinterpret_cast<Record*>(A.ws) + blockIdx.x;
  if (threadIdx.x == 0) *rec = Record{0, 0};
  const uint8_t* g = A.ws + d.gat_off;
  if (d.gat_bytes < 2) return Route::fail(A, d.frame, Route::ERR_IO);
  const uint32_t cmf = g[0], flg = g[1];
  if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20))
    return Route::fail(A, d.frame, Route::ERR_IO);

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
  if (end == STREAM_FAIL) return Route::fail(A, d.frame, Route::ERR_IO);
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

template <class Route>
__global__ __launch_bounds__(WIDE) void adler_kernel(typename Route::Args A) {
  __shared__ uint64_t sa[WIDE], sb[WIDE];
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const auto d = A.descs[blockIdx.x];
  if (Route::check_desc(A, d) != 0 || A.status[d.frame] != 0) return;
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
    if (((fb << 16) | fa) != rec.expected) atomicCAS(&A.status[d.frame], 0, Route::ERR_IO);
  }
}

__device__ inline int paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// The unfilter of one frame, called by its wave with a descriptor that fits the call: H rows of a filter byte and W
// pixels of bpp bytes in the slot.  A band's filter bytes are checked, then the band runs, so the bands above a bad
// filter byte have been through the sink.  sink(row, x, px, bytes, carry) gets every reconstructed pixel once: px has
// channel c in bits [8c, 8c + 8), bytes are the pixel's filtered bytes in the slot, and carry marks the rows the next
// band reads back from there.
template <class Route, class Sink>
__device__ void unfilter_bands(const typename Route::Args& A, int frame, int W, int H, int bpp, uint8_t* slot,
                               const Sink& sink) {
  const int lane = threadIdx.x;
  const int64_t stride = 1 + (int64_t)W * bpp;
  for (int r0 = 0; r0 < H; r0 += BAND) {
    const int row = r0 + lane;
    const bool active = row < H;
    uint8_t* rowp = slot + (active ? row : 0) * stride;
    const int ft = active ? rowp[0] : 0;
    if (__any(ft > 4)) return Route::fail(A, frame, Route::ERR_IO);
    const uint8_t* carried = r0 > 0 ? slot + (int64_t)(r0 - 1) * stride + 1 : nullptr;  // the band above's last row
    const bool carry_out = lane == BAND - 1 && r0 + BAND < H;
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
        px |= ((uint32_t)(rowp[1 + x * bpp + c] + pred) & 255u) << (8 * c);
      }
      left = px;
      last = px;
      sink(row, x, px, rowp + 1 + x * bpp, carry_out);
    }
    __syncthreads();  // the band's last row is in memory before lane 0 of the next band reads it
  }
}

}  // namespace vge_png_kernels
