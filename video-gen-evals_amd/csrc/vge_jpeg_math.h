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

}  // namespace vge_jpeg
#endif  // VGE_JPEG_MATH_H
