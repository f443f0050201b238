// Device half of the JPEG frame front end (include/vge_frames.h): dequantise, IDCT, chroma upsampling and colour
// conversion in ONE kernel, int16 coefficients in, interleaved uint8 RGB out; no intermediate plane touches HBM.
//
// A workgroup (256 threads) owns a 128 x 64 pixel tile of one frame.  Phase 1 runs the IDCT of every block the tile
// needs into uint8 planes in LDS: the tile's own Y / Cb / Cr blocks plus, for subsampled chroma, the ring of
// neighbouring chroma blocks that holds the one-sample halo of the fancy upsampling (recomputed per tile: a 4:2:0 tile
// runs 128 Y + 2 * 60 chroma blocks for 128 + 2 * 32 of its own; the neighbours' coefficients are L2 hits, tiles of one
// frame are dispatched together).  Eight lanes share a block: each loads one 16-byte coefficient row, the 8 x 8 is
// transposed through a pitch-9 LDS scratch (conflict-free both ways: bank = 8 block + 9 row + column), each lane runs
// the column pass on one column, a second transpose, the row pass on one row, and an 8-byte store into the plane.
// Phase 2 upsamples and converts out of LDS, four pixels (12 contiguous bytes, three dwords) per lane, consecutive lanes
// consecutive quads of a row.  Widths that are no multiple of 4 take a byte-store path (rows are then not dword aligned).
// The arithmetic is vge_jpeg_math.h, shared with the host reconstruct.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/vge_frames.h"
#include "vge_error.h"
#include "vge_jpeg_math.h"

using vge::set_last_error;

namespace {

constexpr int TW = 128, TH = 64;          // tile, pixels
constexpr int PLANE_BYTES = TW * TH;      // largest component region: 16 x 8 blocks (Y, or 4:4:4 chroma)
constexpr int GROUPS = 32;                // 8-lane groups per workgroup
constexpr int SCR = 72;                   // scratch words per group: 8 rows, pitch 9

struct Params {
  const int16_t* coef;
  const uint16_t* qtab;
  uint8_t* rgb;
  vge_jpeg_layout L;
  int tiles_x, tiles_y;
};

struct Region {  // the blocks of one component a tile decodes, and where its plane sits in LDS
  int bx0, by0, nx, ny, base, pitch;
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void jpeg_reconstruct_kernel(const Params P) {
  using namespace vge_jpeg;
  __shared__ __attribute__((aligned(16))) uint8_t planes[3 * PLANE_BYTES];
  __shared__ int32_t scratch[GROUPS * SCR];
  const vge_jpeg_layout& L = P.L;
  const int tid = threadIdx.x;
  const int tiles = P.tiles_x * P.tiles_y;
  const int f = blockIdx.x / tiles, t = blockIdx.x - f * tiles;
  const int ty = t / P.tiles_x, tx = t - ty * P.tiles_x;
  const int W = L.width, H = L.height;
  const int x0 = tx * TW, x1 = min(x0 + TW, W), y0 = ty * TH, y1 = min(y0 + TH, H);
  const int mode = L.h0 == 1 ? MODE_444 : (L.v0 == 1 ? MODE_H2V1 : MODE_H2V2);
  const int cw = (W + L.h0 - 1) / L.h0, ch = (H + L.v0 - 1) / L.v0;  // the cropped chroma plane

  auto region = [&](int c) {
    Region rg;
    const int hs = (c > 0 && mode != MODE_444) ? 1 : 0, vs = (c > 0 && mode == MODE_H2V2) ? 1 : 0;
    const int pw = c > 0 ? cw : W, ph = c > 0 ? ch : H;
    // samples the tile reads: its own plus a one-sample halo where the component is upsampled, inside the crop
    const int sx0 = max((x0 >> hs) - hs, 0), sx1 = min(((x1 - 1) >> hs) + hs, pw - 1);
    const int sy0 = max((y0 >> vs) - vs, 0), sy1 = min(((y1 - 1) >> vs) + vs, ph - 1);
    rg.bx0 = sx0 >> 3;
    rg.by0 = sy0 >> 3;
    rg.nx = c < L.n_comp ? (sx1 >> 3) - rg.bx0 + 1 : 0;
    rg.ny = c < L.n_comp ? (sy1 >> 3) - rg.by0 + 1 : 0;
    rg.base = c * PLANE_BYTES;
    rg.pitch = rg.nx * 8;
    return rg;
  };
  // three variables and selects below, not an array: a dynamically indexed register array would live in scratch
  const Region R0 = region(0), R1 = region(1), R2 = region(2);
  const int nb1 = R0.nx * R0.ny, nb2 = nb1 + R1.nx * R1.ny, nb3 = nb2 + R2.nx * R2.ny;

  // ---- phase 1: IDCT of every block of the three regions into the LDS planes
  const int grp = tid >> 3, r = tid & 7;
  int32_t* ws = scratch + grp * SCR;
  const size_t frame_blk = (size_t)f * L.blocks_per_frame;
  for (int g0 = 0; g0 < nb3; g0 += GROUPS) {
    const int g = g0 + grp;
    const bool active = g < nb3;
    const int c = g >= nb2 ? 2 : (g >= nb1 ? 1 : 0);
    const Region rg = c == 2 ? R2 : (c == 1 ? R1 : R0);
    const int lg = active ? g - (c == 2 ? nb2 : (c == 1 ? nb1 : 0)) : 0;
    const int c_off = c == 2 ? L.off[2] : (c == 1 ? L.off[1] : L.off[0]);
    const int c_bw = c == 2 ? L.bw[2] : (c == 1 ? L.bw[1] : L.bw[0]);
    const int lby = lg / max(rg.nx, 1), lbx = lg - lby * rg.nx;
    int32_t in[8], o[8];
    if (active) {
      const size_t blk = frame_blk + c_off + (size_t)(rg.by0 + lby) * c_bw + rg.bx0 + lbx;
      const uint4 cv = *reinterpret_cast<const uint4*>(P.coef + blk * 64 + r * 8);
      const uint4 qv = *reinterpret_cast<const uint4*>(P.qtab + ((size_t)f * 3 + c) * 64 + r * 8);
      const uint32_t cw4[4] = {cv.x, cv.y, cv.z, cv.w}, qw4[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // dequantise row r
        ws[r * 9 + 2 * k] = (int32_t)(int16_t)(cw4[k] & 0xffffu) * (int32_t)(qw4[k] & 0xffffu);
        ws[r * 9 + 2 * k + 1] = ((int32_t)cw4[k] >> 16) * (int32_t)(qw4[k] >> 16);
      }
    }
    wave_sync();
    if (active) {  // column r
#pragma unroll
      for (int v = 0; v < 8; ++v) in[v] = ws[v * 9 + r];
      idct_pass(in, o);
    }
    wave_sync();
    if (active) {
#pragma unroll
      for (int v = 0; v < 8; ++v) ws[v * 9 + r] = descale1(o[v]);
    }
    wave_sync();
    if (active) {  // row r
#pragma unroll
      for (int u = 0; u < 8; ++u) in[u] = ws[r * 9 + u];
      idct_pass(in, o);
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        lo |= (uint32_t)descale2(o[u]) << (8 * u);
        hi |= (uint32_t)descale2(o[u + 4]) << (8 * u);
      }
      *reinterpret_cast<uint2*>(planes + rg.base + (lby * 8 + r) * rg.pitch + lbx * 8) = make_uint2(lo, hi);
    }
    wave_sync();
  }
  __syncthreads();

  // ---- phase 2: upsample + colour convert out of LDS
  const uint8_t* py = planes + R0.base;
  const uint8_t* pb = planes + R1.base;
  const uint8_t* pr = planes + R2.base;
  const int p0 = R0.pitch, pc = R1.pitch;
  const int oy0 = R0.by0 * 8, ox0 = R0.bx0 * 8, oyc = R1.by0 * 8, oxc = R1.bx0 * 8;  // region origins, samples
  const bool gray = L.n_comp == 1;
  auto at_b = [=](int cx, int cy) { return (int)pb[(cy - oyc) * pc + (cx - oxc)]; };
  auto at_r = [=](int cx, int cy) { return (int)pr[(cy - oyc) * pc + (cx - oxc)]; };
  auto pixel = [&](int yv, int x, int y, int* rr, int* gg, int* bb) {
    if (gray) {
      *rr = *gg = *bb = yv;
    } else {
      ycc_to_rgb(yv, chroma_at(at_b, x, y, cw, ch, mode), chroma_at(at_r, x, y, cw, ch, mode), rr, gg, bb);
    }
  };
  const int tw = x1 - x0, th = y1 - y0;
  uint8_t* out = P.rgb + (size_t)f * H * W * 3;
  if ((W & 3) == 0) {
    const int nq = tw >> 2;
    for (int idx = tid; idx < nq * th; idx += 256) {
      const int row = idx / nq, x = x0 + 4 * (idx - row * nq), y = y0 + row;
      const uint32_t y4 = *reinterpret_cast<const uint32_t*>(py + (y - oy0) * p0 + (x - ox0));
      int c[12];
#pragma unroll
      for (int k = 0; k < 4; ++k) pixel((int)((y4 >> (8 * k)) & 255u), x + k, y, &c[3 * k], &c[3 * k + 1], &c[3 * k + 2]);
      uint32_t w[3];
#pragma unroll
      for (int k = 0; k < 3; ++k)
        w[k] = (uint32_t)c[4 * k] | ((uint32_t)c[4 * k + 1] << 8) | ((uint32_t)c[4 * k + 2] << 16) |
               ((uint32_t)c[4 * k + 3] << 24);
      uint32_t* dst = reinterpret_cast<uint32_t*>(out + ((size_t)y * W + x) * 3);
      dst[0] = w[0];
      dst[1] = w[1];
      dst[2] = w[2];
    }
  } else {
    for (int idx = tid; idx < tw * th; idx += 256) {
      const int row = idx / tw, x = x0 + idx - row * tw, y = y0 + row;
      int rr, gg, bb;
      pixel((int)py[(y - oy0) * p0 + (x - ox0)], x, y, &rr, &gg, &bb);
      uint8_t* dst = out + ((size_t)y * W + x) * 3;
      dst[0] = (uint8_t)rr;
      dst[1] = (uint8_t)gg;
      dst[2] = (uint8_t)bb;
    }
  }
}

}  // namespace

extern "C" int vge_jpeg_reconstruct(const int16_t* coef, const uint16_t* qtab, const vge_jpeg_layout* layout,
                                    int n_frames, uint8_t* rgb, void* stream) {
  vge_jpeg_layout want;
  if (n_frames < 0 || !layout ||
      vge_jpeg_make_layout(layout->width, layout->height, layout->n_comp, layout->h0, layout->v0, &want) != VGE_JPEG_OK ||
      memcmp(&want, layout, sizeof(want)) != 0 || (n_frames > 0 && (!coef || !qtab || !rgb)) ||
      ((uintptr_t)coef & 15) || ((uintptr_t)qtab & 15) || ((uintptr_t)rgb & 3)) {
    set_last_error("vge_jpeg_reconstruct: bad argument (layout not from vge_jpeg_make_layout, null or misaligned buffer)");
    return VGE_JPEG_ERR_ARG;
  }
  if (n_frames == 0) return VGE_JPEG_OK;
  Params P;
  P.coef = coef;
  P.qtab = qtab;
  P.rgb = rgb;
  P.L = want;
  P.tiles_x = (want.width + TW - 1) / TW;
  P.tiles_y = (want.height + TH - 1) / TH;
  const long long grid = (long long)n_frames * P.tiles_x * P.tiles_y;
  if (grid > 0x7fffffffLL) {
    set_last_error("vge_jpeg_reconstruct: too many tiles for one launch");
    return VGE_JPEG_ERR_ARG;
  }
  hipLaunchKernelGGL(jpeg_reconstruct_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error(std::string("vge_jpeg_reconstruct: ") + hipGetErrorString(e));
    return VGE_JPEG_ERR_HIP;
  }
  return VGE_JPEG_OK;
}
