// Device half of JPEG encoding (include/vge_frames.h): colour conversion, edge expansion, chroma downsampling, forward
// DCT and quantisation in ONE kernel, interleaved uint8 RGB in, int16 coefficients out; no intermediate plane touches
// HBM.  It is vge_jpeg.hip turned around, with the same tile.
//
// A workgroup (256 threads) owns a 128 x 64 pixel tile of one frame: a whole number of MCUs in all three samplings, so
// the real block a dummy block takes its DC from is always in the same tile.  Phase 1 converts the tile's pixels and
// writes the Y plane and the downsampled Cb / Cr planes to LDS as uint8.  A lane takes four pixels of one row (4:4:4,
// 4:2:2) or of two rows (4:2:0): 12 contiguous bytes per row, three dwords, consecutive lanes consecutive quads; widths
// that are no multiple of 4, and quads beyond the right edge, take a byte path (rows are then not dword aligned).
// Coordinates are clamped by libjpeg's edge rules: x to W - 1, luma rows to H - 1, chroma rows through down_rows_v2
// (the last DOWNSAMPLED row repeats, vge_jpeg_math.h).  Phase 2: eight lanes share a block: each runs the row pass on
// one row out of LDS, the 8 x 8 is transposed through a pitch-9 LDS scratch (conflict-free both ways: bank = 8 block +
// 9 row + column), each lane runs the column pass on one column, a second transpose, and each lane quantises and stores
// one 16-byte coefficient row.  A dummy block runs the same pass on its source block's samples and keeps only the DC.
// The arithmetic is vge_jpeg_math.h, shared with the host forward (vge_jpeg.cpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/vge_frames.h"
#include "vge_error.h"
#include "vge_jpeg_math.h"

using vge::set_last_error;

namespace {

constexpr int TW = 128, TH = 64;      // tile, pixels
constexpr int PLANE_BYTES = TW * TH;  // largest component region: 16 x 8 blocks (Y, or 4:4:4 chroma)
constexpr int GROUPS = 32;            // 8-lane groups per workgroup
constexpr int SCR = 72;               // scratch words per group: 8 rows, pitch 9

struct EncParams {
  const uint8_t* rgb;
  const uint16_t* qtab;
  int16_t* coef;
  vge_jpeg_layout L;
  int tiles_x, tiles_y;
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Pixels x .. x + 3 of one frame row (x a multiple of 4) -> Y, Cb, Cr; columns beyond W - 1 repeat column W - 1.
__device__ __forceinline__ void load_quad(const uint8_t* row, int x, int W, bool dwords, int* yy, int* cb, int* cr) {
  using namespace vge_jpeg;
  if (dwords && x + 3 < W) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(row + (size_t)x * 3);
    const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
    rgb_to_ycc(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, &yy[0], &cb[0], &cr[0]);
    rgb_to_ycc(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u, &yy[1], &cb[1], &cr[1]);
    rgb_to_ycc((w1 >> 16) & 255u, w1 >> 24, w2 & 255u, &yy[2], &cb[2], &cr[2]);
    rgb_to_ycc((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24, &yy[3], &cb[3], &cr[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint8_t* p = row + (size_t)min(x + k, W - 1) * 3;
      rgb_to_ycc(p[0], p[1], p[2], &yy[k], &cb[k], &cr[k]);
    }
  }
}

__device__ __forceinline__ uint32_t pack4(const int* v) {
  return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
}

__global__ __launch_bounds__(256) void jpeg_forward_kernel(const EncParams P) {
  using namespace vge_jpeg;
  __shared__ __attribute__((aligned(16))) uint8_t planes[3 * PLANE_BYTES];
  __shared__ int32_t scratch[GROUPS * SCR];
  const vge_jpeg_layout& L = P.L;
  const int tid = threadIdx.x;
  const int tiles = P.tiles_x * P.tiles_y;
  const int f = blockIdx.x / tiles, t = blockIdx.x - f * tiles;
  const int ty = t / P.tiles_x, tx = t - ty * P.tiles_x;
  const int W = L.width, H = L.height;
  const int hs = L.h0 == 2 ? 1 : 0, vs = L.v0 == 2 ? 1 : 0;  // chroma subsampling shifts
  // the tile's MCUs, and from them its blocks: luma nbx x nby, each chroma plane ncx x ncy
  const int tmx = TW >> (3 + hs), tmy = TH >> (3 + vs);
  const int ncx = min(tmx, L.mcus_x - tx * tmx), ncy = min(tmy, L.mcus_y - ty * tmy);
  const int nbx = ncx << hs, nby = ncy << vs;
  const int x0 = tx * TW, y0 = ty * TH;
  const int pc = TW >> hs;  // chroma plane pitch in LDS; the luma pitch is TW
  uint8_t* py = planes;
  uint8_t* pb = planes + PLANE_BYTES;
  uint8_t* pr = planes + 2 * PLANE_BYTES;

  // ---- phase 1: colour convert + downsample into the LDS planes, every sample of the tile's blocks
  {
    const uint8_t* frame = P.rgb + (size_t)f * H * W * 3;
    const bool dwords = (W & 3) == 0;
    const int nq = nbx * 2, nu = (nby * 8) >> vs;  // quads across, lane units down (one row, or two for 4:2:0)
    for (int idx = tid; idx < nq * nu; idx += 256) {
      const int u = idx / nq, lx = 4 * (idx - u * nq), x = x0 + lx;
      int ya[4], ba[4], ra[4];
      if (!vs) {
        const int y = min(y0 + u, H - 1);
        load_quad(frame + (size_t)y * W * 3, x, W, dwords, ya, ba, ra);
        *reinterpret_cast<uint32_t*>(py + u * TW + lx) = pack4(ya);
        if (!hs) {
          *reinterpret_cast<uint32_t*>(pb + u * pc + lx) = pack4(ba);
          *reinterpret_cast<uint32_t*>(pr + u * pc + lx) = pack4(ra);
        } else {
          const int i = lx >> 1;  // x0 is even: the bias parity of the plane's column is that of the tile's
          pb[u * pc + i] = (uint8_t)down_h2v1(ba[0], ba[1], i);
          pb[u * pc + i + 1] = (uint8_t)down_h2v1(ba[2], ba[3], i + 1);
          pr[u * pc + i] = (uint8_t)down_h2v1(ra[0], ra[1], i);
          pr[u * pc + i + 1] = (uint8_t)down_h2v1(ra[2], ra[3], i + 1);
        }
      } else {
        const int j = (y0 >> 1) + u;  // chroma row of the frame
        const int l0 = min(2 * j, H - 1), l1 = min(2 * j + 1, H - 1);
        int c0, c1;
        down_rows_v2(j, H, &c0, &c1);
        int yb[4], bb[4], rb[4];
        load_quad(frame + (size_t)l0 * W * 3, x, W, dwords, ya, ba, ra);
        load_quad(frame + (size_t)l1 * W * 3, x, W, dwords, yb, bb, rb);
        *reinterpret_cast<uint32_t*>(py + (2 * u) * TW + lx) = pack4(ya);
        *reinterpret_cast<uint32_t*>(py + (2 * u + 1) * TW + lx) = pack4(yb);
        if (c0 != l0 || c1 != l1) {  // below the last real chroma row: its two input rows, not the luma padding's
          int yt[4];
          load_quad(frame + (size_t)c0 * W * 3, x, W, dwords, yt, ba, ra);
          load_quad(frame + (size_t)c1 * W * 3, x, W, dwords, yt, bb, rb);
        }
        const int i = lx >> 1;
        pb[u * pc + i] = (uint8_t)down_h2v2(ba[0], ba[1], bb[0], bb[1], i);
        pb[u * pc + i + 1] = (uint8_t)down_h2v2(ba[2], ba[3], bb[2], bb[3], i + 1);
        pr[u * pc + i] = (uint8_t)down_h2v2(ra[0], ra[1], rb[0], rb[1], i);
        pr[u * pc + i + 1] = (uint8_t)down_h2v2(ra[2], ra[3], rb[2], rb[3], i + 1);
      }
    }
  }
  __syncthreads();

  // ---- phase 2: FDCT + quantisation of every block of the tile, dummy blocks included
  const int grp = tid >> 3, r = tid & 7;
  int32_t* ws = scratch + grp * SCR;
  const int nb1 = nbx * nby, nbc = ncx * ncy, nb3 = nb1 + 2 * nbc;
  const int cw = (W + hs) >> hs, ch = (H + vs) >> vs;  // the real chroma plane, samples
  const size_t frame_blk = (size_t)f * L.blocks_per_frame;
  for (int g0 = 0; g0 < nb3; g0 += GROUPS) {
    const int g = g0 + grp;
    const bool active = g < nb3;
    // selects, not arrays indexed by c: a dynamically indexed register array would live in scratch
    const int c = g >= nb1 + nbc ? 2 : (g >= nb1 ? 1 : 0);
    const int lg = active ? g - (c == 2 ? nb1 + nbc : (c == 1 ? nb1 : 0)) : 0;
    const int rnx = c ? ncx : nbx;
    const int c_off = c == 2 ? L.off[2] : (c == 1 ? L.off[1] : L.off[0]);
    const int c_bw = c == 2 ? L.bw[2] : (c == 1 ? L.bw[1] : L.bw[0]);
    const uint8_t* plane = c == 2 ? pr : (c == 1 ? pb : py);
    const int pitch = c ? pc : TW;
    const int lby = lg / rnx, lbx = lg - lby * rnx;
    // block coordinates in the component's plane; a dummy block reads its source block's samples
    const int bx = (c ? tx * tmx : (tx * tmx) << hs) + lbx, by = (c ? ty * tmy : (ty * tmy) << vs) + lby;
    const int rbw = ((c ? cw : W) + 7) >> 3, rbh = ((c ? ch : H) + 7) >> 3;
    int sx = bx, sy = by;
    const bool dummy = dummy_source(&sx, &sy, c ? 1 : L.h0, rbw, rbh);
    const int slbx = lbx - (bx - sx), slby = lby - (by - sy);  // the source is in the same MCU, so in this tile
    int32_t in[8], o[8];
    if (active) {  // row r
      const uint2 s = *reinterpret_cast<const uint2*>(plane + (slby * 8 + r) * pitch + slbx * 8);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        in[u] = (int32_t)((s.x >> (8 * u)) & 255u) - 128;
        in[u + 4] = (int32_t)((s.y >> (8 * u)) & 255u) - 128;
      }
      fdct_pass(in, o);
#pragma unroll
      for (int u = 0; u < 8; ++u) ws[r * 9 + u] = fdct_row_out(o[u], u);
    }
    wave_sync();
    if (active) {  // column r
#pragma unroll
      for (int v = 0; v < 8; ++v) in[v] = ws[v * 9 + r];
      fdct_pass(in, o);
    }
    wave_sync();
    if (active) {
#pragma unroll
      for (int v = 0; v < 8; ++v) ws[v * 9 + r] = fdct_col_out(o[v], v);
    }
    wave_sync();
    if (active) {  // coefficient row r: quantise, 16-byte store
      const uint4 qv = *reinterpret_cast<const uint4*>(P.qtab + c * 64 + r * 8);
      const uint32_t qw4[4] = {qv.x, qv.y, qv.z, qv.w};
      uint32_t w4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int32_t lo = quantise(ws[r * 9 + 2 * k], (int32_t)(qw4[k] & 0xffffu));
        int32_t hi = quantise(ws[r * 9 + 2 * k + 1], (int32_t)(qw4[k] >> 16));
        if (dummy) {
          hi = 0;
          if (r | k) lo = 0;
        }
        w4[k] = ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
      }
      const size_t blk = frame_blk + c_off + (size_t)by * c_bw + bx;
      *reinterpret_cast<uint4*>(P.coef + blk * 64 + r * 8) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
    }
    wave_sync();
  }
}

}  // namespace

extern "C" int vge_jpeg_forward(const uint8_t* rgb, const vge_jpeg_layout* layout, int n_frames, const uint16_t* qtab,
                                int16_t* coef, void* stream) {
  vge_jpeg_layout want;
  if (n_frames < 0 || !layout ||
      vge_jpeg_make_layout(layout->width, layout->height, layout->n_comp, layout->h0, layout->v0, &want) != VGE_JPEG_OK ||
      memcmp(&want, layout, sizeof(want)) != 0 || !qtab || (n_frames > 0 && (!rgb || !coef)) ||
      ((uintptr_t)coef & 15) || ((uintptr_t)qtab & 15) || ((want.width & 3) == 0 && ((uintptr_t)rgb & 3))) {
    // rgb is read as dwords only when the width is a multiple of 4 (every frame of the batch is then 4-byte aligned)
    set_last_error("vge_jpeg_forward: bad argument (layout not from vge_jpeg_make_layout, null or misaligned buffer)");
    return VGE_JPEG_ERR_ARG;
  }
  if (want.n_comp != 3) {
    set_last_error("vge_jpeg_forward: only 3-component (RGB) frames are encoded");
    return VGE_JPEG_ERR_COMPONENTS;
  }
  if (n_frames == 0) return VGE_JPEG_OK;
  EncParams P;
  P.rgb = rgb;
  P.qtab = qtab;
  P.coef = coef;
  P.L = want;
  P.tiles_x = (want.width + TW - 1) / TW;
  P.tiles_y = (want.height + TH - 1) / TH;
  const long long grid = (long long)n_frames * P.tiles_x * P.tiles_y;
  if (grid > 0x7fffffffLL) {
    set_last_error("vge_jpeg_forward: too many tiles for one launch");
    return VGE_JPEG_ERR_ARG;
  }
  hipLaunchKernelGGL(jpeg_forward_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error(std::string("vge_jpeg_forward: ") + hipGetErrorString(e));
    return VGE_JPEG_ERR_HIP;
  }
  return VGE_JPEG_OK;
}
