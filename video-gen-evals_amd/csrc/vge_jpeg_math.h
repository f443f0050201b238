// The JPEG reconstruction arithmetic (include/vge_frames.h), shared by the HIP kernel (vge_jpeg.hip) and the host
// reconstruct (vge_jpeg.cpp) so the two cannot drift apart.  It restates libjpeg's defaults, the ones cv2.imread and
// Pillow decode with: the "islow" integer IDCT (jidctint.c: CONST_BITS 13, PASS1_BITS 2), fancy h2v1 / h2v2 chroma
// upsampling (jdsample.c) and the 16-bit fixed-point YCbCr -> RGB (jdcolor.c).
//
// 32-bit safety.  One 8-point pass is an integer linear map out_j = sum_k m_jk in_k.  Its additions, subtractions and
// multiplications are done on uint32 (wrapping, a ring), so an intermediate may wrap freely: the result is right
// whenever the true value at the descale fits int32.  The largest |m_jk| is M = 11,363 (1.387 * 8192; measured from
// the constants by pushing unit vectors through the pass, tests/test_jpeg_host.py).  With s_c the L1 norm of column c
// of a dequantised block and S = sum_c s_c:
//   pass 1 (columns): |pre-descale| <= M s_c <= 11,363 * 32,767 < 2^29;  |out| <= M s_c / 2048 + 1.5
//   pass 2 (rows):    a row's inputs have L1 <= M S / 2048 + 12, so |pre-descale| + 2^17 <= M (M S / 2048 + 12) + 2^17
//                     = 2,066,3xx,xxx < 2^31 for S <= 32,767 (the bound allows S <= 34,058)
// hence VGE_JPEG_BLOCK_L1_MAX = 32,767; the entropy decoder refuses a frame with a block beyond it.  A block encoded
// from 8-bit samples has S <= 8 * 1024 (orthonormal DCT: L1 <= 8 * L2) + 64 * 127 (quantisation rounding) < 16,400.
#ifndef VGE_JPEG_MATH_H
#define VGE_JPEG_MATH_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VGE_JPEG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define VGE_JPEG_HD inline
#endif

namespace vge_jpeg {

// One 8-point islow pass on i[0..7] -> o[0..7] before the descale.  Wrapping arithmetic (see above).
VGE_JPEG_HD void idct_pass(const int32_t* i, int32_t* o) {
  typedef uint32_t u;
  const u i0 = (u)i[0], i1 = (u)i[1], i2 = (u)i[2], i3 = (u)i[3], i4 = (u)i[4], i5 = (u)i[5], i6 = (u)i[6], i7 = (u)i[7];
  // even part
  u z1 = (i2 + i6) * 4433u;
  const u t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
  const u t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
  const u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  // odd part
  u a = i7, b = i5, c = i3, d = i1;
  z1 = a + d;
  u z2 = b + c, z3 = a + c, z4 = b + d;
  const u z5 = (z3 + z4) * 9633u;
  a *= 2446u;
  b *= 16819u;
  c *= 25172u;
  d *= 12299u;
  z1 *= (u)-7373;
  z2 *= (u)-20995;
  z3 = z3 * (u)-16069 + z5;
  z4 = z4 * (u)-3196 + z5;
  a += z1 + z3;
  b += z2 + z4;
  c += z2 + z3;
  d += z1 + z4;
  o[0] = (int32_t)(t10 + d);
  o[1] = (int32_t)(t11 + c);
  o[2] = (int32_t)(t12 + b);
  o[3] = (int32_t)(t13 + a);
  o[4] = (int32_t)(t13 - a);
  o[5] = (int32_t)(t12 - b);
  o[6] = (int32_t)(t11 - c);
  o[7] = (int32_t)(t10 - d);
}

VGE_JPEG_HD int32_t descale1(int32_t x) { return (int32_t)((uint32_t)x + (1u << 10)) >> 11; }  // after the column pass
VGE_JPEG_HD int32_t clamp255(int32_t x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }
// after the row pass: descale, level shift, clamp -> sample
VGE_JPEG_HD int32_t descale2(int32_t x) { return clamp255(((int32_t)((uint32_t)x + (1u << 17)) >> 18) + 128); }

// Sampling modes of the chroma planes against luma.
enum { MODE_444 = 0, MODE_H2V1 = 1, MODE_H2V2 = 2 };

VGE_JPEG_HD int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Chroma sample of output pixel (x, y).  `at(cx, cy)` reads the component's decoded plane; cw x ch is the plane cropped
// to ceil(W h / hmax) x ceil(H v / vmax): neighbours beyond the crop repeat the edge sample, not the decoded padding.
// A plane of at most two columns is not interpolated at all: libjpeg picks its fancy upsamplers only when the
// component's downsampled width is > 2 (jdsample.c jinit_upsampler) and replicates samples otherwise, in both directions.
template <class At>
VGE_JPEG_HD int chroma_at(const At& at, int x, int y, int cw, int ch, int mode) {
  if (mode == MODE_444) return at(x, y);
  if (cw <= 2) return at(x >> 1, mode == MODE_H2V2 ? y >> 1 : y);
  const int k = x >> 1, kn = clampi((x & 1) ? k + 1 : k - 1, 0, cw - 1);
  if (mode == MODE_H2V1) return (3 * at(k, y) + at(kn, y) + ((x & 1) ? 2 : 1)) >> 2;
  const int r = y >> 1, rn = clampi((y & 1) ? r + 1 : r - 1, 0, ch - 1);
  const int c0 = 3 * at(k, r) + at(k, rn);     // the vertical step, unrounded
  const int c1 = 3 * at(kn, r) + at(kn, rn);
  return (3 * c0 + c1 + ((x & 1) ? 7 : 8)) >> 4;
}

// YCbCr -> RGB, F(x) = int(x * 65536 + 0.5): F(1.402) 91881, F(1.772) 116130, F(0.34414) 22554, F(0.71414) 46802.
VGE_JPEG_HD void ycc_to_rgb(int y, int cb, int cr, int* r, int* g, int* b) {
  cb -= 128;
  cr -= 128;
  *r = clamp255(y + ((91881 * cr + 32768) >> 16));
  *g = clamp255(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  *b = clamp255(y + ((116130 * cb + 32768) >> 16));
}

// ---------------------------------------------------------------------------------------------------------------------
// The forward (encoding) arithmetic, shared by vge_jpeg_enc.hip and the host forward in vge_jpeg_enc.cpp: libjpeg's
// defaults again, the ones cv2.imwrite and Pillow encode with.  RGB -> YCbCr in 16-bit fixed point (jccolor.c), h2v1 /
// h2v2 box downsampling without smoothing (jcsample.c), the "islow" forward DCT on samples - 128 (jfdctint.c: CONST_BITS
// 13, PASS1_BITS 2; the output is the DCT scaled by 8) and the rounding division of jcdctmgr.c.
//
// 32-bit safety.  Inputs are samples - 128, |d| <= 128.  Row pass: out 0 / 4 are sums of eight inputs << 2, |.| <= 4,096;
// the other outputs are at most M * 8 * 128 = 11,635,712 before the descale by 11 (M = 11,363 as above: the forward pass
// is the inverse's transpose), so every pass-1 output is below 2^13.  Column pass: |pre-descale| <= M * 8 * 2^13 <
// 2^30, plus the rounding constant 2^14.  Nothing wraps; plain int32 arithmetic.  The descaled column outputs are below
// 2^15, the quantised values below 2^15 / 8 + 1.

// F(x) = int(x * 65536 + 0.5): .299 19595, .587 38470, .114 7471, .16874 11059, .33126 21709, .5 32768, .41869 27439,
// .08131 5329.  Cb / Cr round with 32767, not 32768 (jccolor.c: CBCR_OFFSET + ONE_HALF - 1).
VGE_JPEG_HD void rgb_to_ycc(int r, int g, int b, int* y, int* cb, int* cr) {
  *y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  *cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  *cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// Box downsampling of output column i: the bias alternates along the output row and starts anew in every row.
VGE_JPEG_HD int down_h2v2(int a, int b, int c, int d, int i) { return (a + b + c + d + ((i & 1) ? 2 : 1)) >> 2; }
VGE_JPEG_HD int down_h2v1(int a, int b, int i) { return (a + b + (i & 1)) >> 1; }

// The two input rows of downsampled row j of a plane with vertical factor 2 (h2v2), frame height H, ch = ceil(H / 2)
// real rows.  libjpeg replicates the last input row only up to a multiple of the sampling factor, downsamples, and
// fills the remaining block rows with the last DOWNSAMPLED row: row j >= ch is row ch - 1, which for an even H averages
// rows H - 2 and H - 1 (replicating input rows instead would give row H - 1 alone).
VGE_JPEG_HD void down_rows_v2(int j, int H, int* r0, int* r1) {
  const int ch = (H + 1) >> 1, jc = j < ch ? j : ch - 1;
  *r0 = 2 * jc;  // < H
  *r1 = 2 * jc + 1 < H ? 2 * jc + 1 : H - 1;
}

// One 8-point islow forward pass on d[0..7] -> o[0..7] before the descale.  o[0] and o[4] are the plain sums t10 +- t11.
VGE_JPEG_HD void fdct_pass(const int32_t* d, int32_t* o) {
  const int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  o[0] = t10 + t11;
  o[4] = t10 - t11;
  int32_t z1 = (t12 + t13) * 4433;
  o[2] = z1 + t13 * 6270;
  o[6] = z1 - t12 * 15137;
  z1 = t4 + t7;
  int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int32_t z5 = (z3 + z4) * 9633;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  o[7] = t4 * 2446 + z1 + z3;
  o[5] = t5 * 16819 + z2 + z4;
  o[3] = t6 * 25172 + z2 + z3;
  o[1] = t7 * 12299 + z1 + z4;
}

VGE_JPEG_HD int32_t descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }
// output k of the row pass (first) and of the column pass (second)
VGE_JPEG_HD int32_t fdct_row_out(int32_t x, int k) { return (k & 3) == 0 ? x * 4 : descale(x, 11); }
VGE_JPEG_HD int32_t fdct_col_out(int32_t x, int k) { return (k & 3) == 0 ? descale(x, 2) : descale(x, 15); }

// jcdctmgr.c: divisor q << 3 (the FDCT output is scaled by 8), rounded half away from zero.  An exact integer division.
VGE_JPEG_HD int32_t quantise(int32_t v, int32_t q) {
  const uint32_t d = (uint32_t)q << 3, a = (uint32_t)(v < 0 ? -v : v);
  const int32_t m = (int32_t)((a + (d >> 1)) / d);
  return v < 0 ? -m : m;
}

// Blocks of a component's plane beyond its real ones -- ceil(ceil(W h / hmax) / 8) x ceil(ceil(H v / vmax) / 8) --
// exist only to fill the last MCU column / row (jccoefct.c): all-zero AC, and the DC of the previous block in the MCU's
// block order.  With the supported samplings only luma has them, at most one column and one row.  Returns whether block
// (*bx, *by) of a component with h blocks across an MCU is such a dummy and moves (*bx, *by) to the real block whose DC
// it takes: a dummy row takes the last block of the row above inside its MCU, a right-edge dummy the block to its left.
VGE_JPEG_HD bool dummy_source(int* bx, int* by, int h, int rbw, int rbh) {
  bool dummy = false;
  if (*by >= rbh) {
    dummy = true;
    *by -= 1;
    *bx = (*bx / h) * h + h - 1;
  }
  if (*bx >= rbw) {
    dummy = true;
    *bx -= 1;
  }
  return dummy;
}

}  // namespace vge_jpeg
#endif  // VGE_JPEG_MATH_H
