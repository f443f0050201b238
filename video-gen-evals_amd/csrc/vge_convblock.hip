// One residual block of MovementConvEncoder (model.py:21-58 TemporalConvBlock; vge/model.py _Block) for training on
// gfx950: a forward that keeps what the backward needs, and the backward to every input and parameter
// (vge_convblock_forward / vge_convblock_backward, formulas in include/vge.h).  Exact f32 on v_mfma_f32_16x16x4_f32.
//
//   cb_pack_kernel      a [C_out, C_in, 5] weight -> the image the conv core's B reads use, as it is (a, u) or with
//                       the taps flipped and each tap's matrix transposed (dh, dx: the data gradient of a stride-1,
//                       symmetrically padded, dilated convolution is that same convolution).  Per call: the weights
//                       change every step.
//   cb_forward_kernel   one workgroup = one sample [T <= 64][C <= 256], held in LDS with 16 zero rows before and
//                       after, so a shifted tap row is a plain LDS row (the [B,T,5C] tap copy does not exist):
//                       a = conv(x; W1) -> h = gelu(a) m written over x in LDS -> u = conv(h; W2) + x -> g = gelu(u)
//                       -> mean / rstd of the sample -> y.  a, u, mean, rstd are stored for the backward.
//   cb_backward_kernel  one workgroup = one sample: q = dy gamma, g^ from u, the sample's mean(q) and mean(q g^), du
//                       (LDS and HBM), per-channel partials of dgamma / dbeta, dh = conv(du; W2 flipped), h and da
//                       (HBM; da over du in LDS), dx = du + conv(da; W1 flipped).
//   cb_wgrad_kernel     dW[o,i,j] = sum_{b,t} D[b,t,o] H[b,t+(j-2) dil,i] for (D, H) = (da, x) and (du, h): one
//                       workgroup = (chunk of samples, tap j, 64 output channels, which weight); K runs over the
//                       chunk's rows; the result is that chunk's partial.
//   cb_wreduce_kernel   adds the chunk partials in chunk order into torch's [C_out, C_in, 5] layout.
//   cb_gbreduce_kernel  adds the per-sample partials of dgamma / dbeta in sample order.
//
// Conv core.  Output tile [Tp = 16 ceil(T / 16)][C]; wave w owns the 16-column tiles w, w + 4, ... (at most 4) over
// every 16-row tile (at most 4): 16 accumulators.  An output element's 5 C products are summed in three levels: one
// MFMA chain per 16 products, those added per tap in f64, the five taps rounded to f32 and added.  MFMA k-step
// (tap j, c, q) takes from lane group g = lane >> 4 the input channel k = (C / 4) g + 4 c + q, so one ds_read_b128
// gives a lane its A values of 4 k-steps and one 16-byte global load its B values ([j][c][g][n][q] image).  Fragment
// maps: vge_common.h mfma16x16x4.
//
// Order of every sum is fixed by (B, T, C, dil): a thread owns fixed elements, wave sums are xor butterflies, wave
// partials are added in wave order, workgroup partials by a second launch in index order.  Products are MFMA f32
// chains.  A sample's statistics, dgamma / dbeta and the (at most 8) chunk partials of dw1 / dw2 are summed in f64 over
// f32 values and rounded to f32 once; inside a chunk a weight gradient adds one T-long MFMA chain per sample in f32.
// No floating-point atomics, no kernel waits on another workgroup.  Rows T .. Tp-1 of a tile are zero wherever a
// later sum or convolution reads them, and are never stored.
#include "vge_common.h"

#include <string>

#include "../../include/vge.h"
#include "vge_core.h"
#include "vge_error.h"
#include "vge_lds_attr.h"

namespace {

using vge::ConvBlockBwdArgs;
using vge::ConvBlockFwdArgs;
using vge::ConvBlockWgradArgs;

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int CB_HALO = 16;      // zero rows before and after the tile: 2 x the largest dilation
constexpr int CB_WG_OB = 64;     // output channels per weight-gradient workgroup
constexpr int CB_MAX_CHUNKS = 8; // sample chunks of the weight gradient (partials per weight)
constexpr float CB_EPS = 1e-5f;

__host__ __device__ constexpr int cb_tp(int T) { return (T + 15) & ~15; }

// Phi(z) and phi(z) of the standard normal: gelu(z) = z Phi(z), gelu'(z) = Phi(z) + z phi(z)
__device__ __forceinline__ float cb_Phi(float z) { return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)); }
__device__ __forceinline__ float cb_phi(float z) { return 0.39894228040143267794f * expf(-0.5f * z * z); }

// sum over the workgroup (256 threads), every thread receives it; red: 4 doubles of LDS
__device__ __forceinline__ double cb_block_sum(double v, double* red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

// ------------------------------------------------------------------------------------------------ weight image
// P[(((j nc + c) 4 + g) C + n) 4 + q] = flip ? W[k][n][4 - j] : W[n][k][j],  k = (C / 4) g + 4 c + q, nc = C / 16
__global__ void __launch_bounds__(256) cb_pack_kernel(const float* __restrict__ W, int C, int flip,
                                                      float* __restrict__ P) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 5 * C * C) return;
  const int nc = C >> 4;
  const int q = e & 3, n = (e >> 2) % C, rest = (e >> 2) / C;
  const int g = rest & 3, jc = rest >> 2, c = jc % nc, j = jc / nc;
  const int k = (C >> 2) * g + 4 * c + q;
  P[e] = flip ? W[((size_t)k * C + n) * 5 + (4 - j)] : W[((size_t)n * C + k) * 5 + j];
}

// ------------------------------------------------------------------------------------------------ conv core
// acc[n][rt] (C layout: row rt 16 + 4 (lane >> 4) + r, column (wave + 4 n) 16 + (lane & 15)) =
//   sum_j sum_k X[row + (j - 2) dil][k] Wimage(k, column, j);   X: row 0 of the tile (CB_HALO zero rows around it)
__device__ __forceinline__ void cb_conv(floatx4 (&acc)[4][4], const float* X, int LD, const float* __restrict__ P, int C,
                                        int dil, int nrt, int wave, int lane) {
  const int il = lane & 15, g = lane >> 4;
  const int nct = C >> 4;  // 16-column tiles of the output, and 16-channel c-steps of a tap
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[n][rt] = floatx4{0.f, 0.f, 0.f, 0.f};
  const floatx4 zero = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < 5; ++j) {
    // Short chains, because the rounding error of an f32 sum grows with its length: the 16 products of one c-step are
    // one MFMA chain (`part`, exact f32), a tap's C / 16 parts are added in f64 (`tap`), and each tap's sum is rounded
    // to f32 once and added to `acc`.
    doublex4 tap[4][4];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) tap[n][rt] = doublex4{0.0, 0.0, 0.0, 0.0};
    const float* xa = X + (il + (j - 2) * dil) * LD + (C >> 2) * g;
    const float* pb = P + ((size_t)(j * nct) * 4 + g) * C * 4 + (size_t)il * 4;
    for (int c = 0; c < nct; ++c) {
      floatx4 a[4], b[4];
#pragma unroll
      for (int n = 0; n < 4; ++n)
        if (wave + 4 * n < nct) b[n] = *reinterpret_cast<const floatx4*>(pb + ((size_t)c * 4 * C + (wave + 4 * n) * 16) * 4);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        if (rt < nrt) a[rt] = *reinterpret_cast<const floatx4*>(xa + rt * 16 * LD + 4 * c);
      floatx4 part[4][4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          if (wave + 4 * n < nct)
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
              if (rt < nrt) part[n][rt] = mfma16x16x4(a[rt][q], b[n][q], q == 0 ? zero : part[n][rt]);
#pragma unroll
      for (int n = 0; n < 4; ++n)
        if (wave + 4 * n < nct)
#pragma unroll
          for (int rt = 0; rt < 4; ++rt)
            if (rt < nrt) tap[n][rt] += __builtin_convertvector(part[n][rt], doublex4);
    }
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) acc[n][rt] += __builtin_convertvector(tap[n][rt], floatx4);
  }
}

// every (n, rt, r) element this lane owns in the C layout: fn(n, rt, r, row, col, row < T)
template <class Fn>
__device__ __forceinline__ void cb_each(int T, int C, int nrt, int wave, int lane, Fn fn) {
  const int il = lane & 15, g = lane >> 4, nct = C >> 4;
#pragma unroll
  for (int n = 0; n < 4; ++n)
    if (wave + 4 * n < nct)
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        if (rt < nrt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = rt * 16 + 4 * g + r;
            fn(n, rt, r, row, (wave + 4 * n) * 16 + il, row < T);
          }
}

// zero n_floats floats of LDS from p (n_floats a multiple of 4, p 16-byte aligned)
__device__ __forceinline__ void cb_zero(float* p, int n_floats) {
  for (int i = threadIdx.x * 4; i < n_floats; i += 256 * 4) *reinterpret_cast<floatx4*>(p + i) = floatx4{0.f, 0.f, 0.f, 0.f};
}

// ------------------------------------------------------------------------------------------------ forward
__global__ void __launch_bounds__(256) cb_forward_kernel(ConvBlockFwdArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = A.T, C = A.C, LD = C + 4, Tp = cb_tp(T), nrt = Tp >> 4;
  float* X = lds + CB_HALO * LD;
  double* red = reinterpret_cast<double*>(lds + (Tp + 2 * CB_HALO) * LD);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t base = (size_t)blockIdx.x * T * C;
  const float* __restrict__ xg = A.x + base;

  const int c4n = C >> 2;
  for (int i = tid; i < (Tp + 2 * CB_HALO) * c4n; i += 256) {
    const int r = i / c4n - CB_HALO, c4 = i - (r + CB_HALO) * c4n;
    floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
    if (r >= 0 && r < T) v = *reinterpret_cast<const floatx4*>(xg + (size_t)r * C + c4 * 4);
    *reinterpret_cast<floatx4*>(X + r * LD + c4 * 4) = v;
  }
  __syncthreads();

  floatx4 acc[4][4];
  cb_conv(acc, X, LD, A.P1, C, A.dil, nrt, wave, lane);
  __syncthreads();  // every wave has read x: h goes over it
  cb_each(T, C, nrt, wave, lane, [&](int n, int rt, int r, int row, int col, bool ok) {
    float h = 0.f;
    if (ok) {
      const float av = acc[n][rt][r];
      const size_t o = base + (size_t)row * C + col;
      if (A.a) A.a[o] = av;
      h = av * cb_Phi(av);
      if (A.m) h *= A.m[o];
    }
    X[row * LD + col] = h;
  });
  __syncthreads();

  cb_conv(acc, X, LD, A.P2, C, A.dil, nrt, wave, lane);
  double part = 0.0;  // sums leave f32 here: the thread's partial, the wave's and the workgroup's are f64
  cb_each(T, C, nrt, wave, lane, [&](int n, int rt, int r, int row, int col, bool ok) {
    float gv = 0.f;
    if (ok) {
      const size_t o = base + (size_t)row * C + col;
      const float uv = acc[n][rt][r] + xg[(size_t)row * C + col];
      if (A.u) A.u[o] = uv;
      gv = uv * cb_Phi(uv);
      part += (double)gv;
    }
    acc[n][rt][r] = gv;
  });
  const double cnt = (double)T * (double)C;
  const float mu = (float)(cb_block_sum(part, red) / cnt);
  part = 0.0;
  cb_each(T, C, nrt, wave, lane, [&](int n, int rt, int r, int, int, bool ok) {
    if (ok) {
      const double d = (double)(acc[n][rt][r] - mu);
      part = fma(d, d, part);
    }
  });
  const float rstd = (float)(1.0 / sqrt(cb_block_sum(part, red) / cnt + (double)CB_EPS));
  if (tid == 0 && A.mu) {
    A.mu[blockIdx.x] = mu;
    A.rstd[blockIdx.x] = rstd;
  }
  cb_each(T, C, nrt, wave, lane, [&](int n, int rt, int r, int row, int col, bool ok) {
    if (ok) A.y[base + (size_t)row * C + col] = (acc[n][rt][r] - mu) * rstd * A.gamma[col] + A.beta[col];
  });
}

// ------------------------------------------------------------------------------------------------ backward (data)
__global__ void __launch_bounds__(256) cb_backward_kernel(ConvBlockBwdArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = A.T, C = A.C, LD = C + 4, Tp = cb_tp(T), nrt = Tp >> 4;
  float* X = lds + CB_HALO * LD;
  double* red = reinterpret_cast<double*>(lds + (Tp + 2 * CB_HALO) * LD);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const size_t base = (size_t)b * T * C;

  cb_zero(lds, (Tp + 2 * CB_HALO) * LD);

  // q = dy gamma, g^ = (gelu(u) - mu) rstd, gelu'(u); per-channel sums of dy and dy g^ over this sample's rows
  const float mu = A.mu[b], rstd = A.rstd[b];
  floatx4 qv[4][4], gh[4][4], gp[4][4];
  double sb[4] = {0.0, 0.0, 0.0, 0.0}, sg[4] = {0.0, 0.0, 0.0, 0.0};  // f32 values and products, summed in f64
  double pq = 0.0, pqg = 0.0;
  cb_each(T, C, nrt, wave, lane, [&](int n, int rt, int r, int row, int col, bool ok) {
    float q = 0.f, gn = 0.f, d = 0.f;
    if (ok) {
      const size_t o = base + (size_t)row * C + col;
      const float uv = A.u[o], dyv = A.dy[o];
      const float Ph = cb_Phi(uv);
      gn = (uv * Ph - mu) * rstd;
      d = Ph + uv * cb_phi(uv);
      q = dyv * A.gamma[col];
      sb[n] += (double)dyv;
      sg[n] = fma((double)dyv, (double)gn, sg[n]);
      pq += (double)q;
      pqg = fma((double)q, (double)gn, pqg);
    }
    qv[n][rt][r] = q;
    gh[n][rt][r] = gn;
    gp[n][rt][r] = d;
  });
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    if (wave + 4 * n >= (C >> 4)) continue;
    double s0 = sb[n], s1 = sg[n];
    s0 += __shfl_xor(s0, 16, 64);
    s0 += __shfl_xor(s0, 32, 64);
    s1 += __shfl_xor(s1, 16, 64);
    s1 += __shfl_xor(s1, 32, 64);
    if (lane < 16) {
      const int col = (wave + 4 * n) * 16 + lane;
      A.gb_part[((size_t)b * 2 + 0) * C + col] = s1;  // dgamma
      A.gb_part[((size_t)b * 2 + 1) * C + col] = s0;  // dbeta
    }
  }
  const double cnt = (double)T * (double)C;
  const float mq = (float)(cb_block_sum(pq, red) / cnt);    // its first barrier also covers cb_zero
  const float mqg = (float)(cb_block_sum(pqg, red) / cnt);
  cb_each(T, C, nrt, wave, lane, [&](int n, int rt, int r, int row, int col, bool ok) {
    float du = 0.f;
    if (ok) {
      du = rstd * (qv[n][rt][r] - mq - gh[n][rt][r] * mqg) * gp[n][rt][r];
      A.du[base + (size_t)row * C + col] = du;
    }
    X[row * LD + col] = du;
  });
  __syncthreads();

  floatx4 acc[4][4];
  cb_conv(acc, X, LD, A.P2b, C, A.dil, nrt, wave, lane);
  __syncthreads();  // every wave has read du: da goes over it
  cb_each(T, C, nrt, wave, lane, [&](int n, int rt, int r, int row, int col, bool ok) {
    float da = 0.f;
    if (ok) {
      const size_t o = base + (size_t)row * C + col;
      const float av = A.a[o], mv = A.m ? A.m[o] : 1.0f;
      const float Ph = cb_Phi(av);
      A.h[o] = av * Ph * mv;
      da = acc[n][rt][r] * mv * (Ph + av * cb_phi(av));
      A.da[o] = da;
    }
    X[row * LD + col] = da;
  });
  __syncthreads();

  cb_conv(acc, X, LD, A.P1b, C, A.dil, nrt, wave, lane);
  cb_each(T, C, nrt, wave, lane, [&](int n, int rt, int r, int row, int col, bool ok) {
    if (ok) {
      const size_t o = base + (size_t)row * C + col;
      A.dx[o] = A.du[o] + acc[n][rt][r];  // du: this thread's own store above
    }
  });
}

// ------------------------------------------------------------------------------------------------ weight gradient
// grid (n_chunks, 5 * ceil(C / 64), 2).  A[m = o][k = t] = D[t][o], B[k = t][n = i] = H[t + (j - 2) dil][i]; wave w owns
// the input-channel tiles w, w + 4, ... over the (at most 4) output-channel tiles of the workgroup's 64.
__global__ void __launch_bounds__(256) cb_wgrad_kernel(ConvBlockWgradArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = A.T, C = A.C, Tp = cb_tp(T);
  const int LDH = C + 16, LDD = CB_WG_OB + 16;
  float* H = lds + CB_HALO * LDH;                     // row 0 of the tile
  float* D = lds + (Tp + 2 * CB_HALO) * LDH;          // [Tp][LDD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 15, g = lane >> 4;
  const int nob = (C + CB_WG_OB - 1) / CB_WG_OB;
  const int chunk = blockIdx.x, j = blockIdx.y / nob, ob = blockIdx.y - j * nob, z = blockIdx.z;
  const float* __restrict__ Dg = z ? A.du : A.da;
  const float* __restrict__ Hg = z ? A.h : A.x;
  const int o0 = ob * CB_WG_OB, now = min(CB_WG_OB, C - o0), nmt = now >> 4, nct = C >> 4;
  const int roff = (j - 2) * A.dil;
  const int b0 = chunk * A.per_chunk, b1 = min(A.B, b0 + A.per_chunk);

  cb_zero(lds, (Tp + 2 * CB_HALO) * LDH + Tp * LDD);  // the halo, and rows T .. Tp-1 of both tiles, stay zero

  floatx4 acc[4][4], one[4][4];  // the chunk's sum, and one sample's MFMA chain (T products), added sample by sample
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[n][mt] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int c4n = C >> 2, d4n = now >> 2;
  for (int b = b0; b < b1; ++b) {
    __syncthreads();  // the previous sample's reads (the first time: cb_zero's stores)
    const size_t base = (size_t)b * T * C;
    for (int i = tid; i < T * c4n; i += 256) {
      const int r = i / c4n, c4 = i - r * c4n;
      *reinterpret_cast<floatx4*>(H + r * LDH + c4 * 4) = *reinterpret_cast<const floatx4*>(Hg + base + (size_t)r * C + c4 * 4);
    }
    for (int i = tid; i < T * d4n; i += 256) {
      const int r = i / d4n, c4 = i - r * d4n;
      *reinterpret_cast<floatx4*>(D + r * LDD + c4 * 4) =
          *reinterpret_cast<const floatx4*>(Dg + base + (size_t)r * C + o0 + c4 * 4);
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) one[n][mt] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < ((T + 3) >> 2); ++s) {  // rows T .. 4 ceil(T / 4) - 1 of D are zero
      const int t = 4 * s + g;
      float a[4], bb[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        if (mt < nmt) a[mt] = D[t * LDD + mt * 16 + il];
#pragma unroll
      for (int n = 0; n < 4; ++n)
        if (wave + 4 * n < nct) bb[n] = H[(t + roff) * LDH + (wave + 4 * n) * 16 + il];
#pragma unroll
      for (int n = 0; n < 4; ++n)
        if (wave + 4 * n < nct)
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
            if (mt < nmt) one[n][mt] = mfma16x16x4(a[mt], bb[n], one[n][mt]);
    }
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[n][mt] += one[n][mt];
  }
  // partial [chunk][z][j][o][i]
  float* __restrict__ out = A.part + (((size_t)chunk * 2 + z) * 5 + j) * C * C;
#pragma unroll
  for (int n = 0; n < 4; ++n)
    if (wave + 4 * n < nct)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        if (mt < nmt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            out[(size_t)(o0 + mt * 16 + 4 * g + r) * C + (wave + 4 * n) * 16 + il] = acc[n][mt][r];
}

// dW[z][o][i][j] = sum over chunks, in chunk order, of part[chunk][z][j][o][i]
__global__ void __launch_bounds__(256) cb_wreduce_kernel(const float* __restrict__ part, int n_chunks, int C,
                                                         float* __restrict__ dw1, float* __restrict__ dw2) {
  const int e = blockIdx.x * 256 + threadIdx.x, CC = C * C;
  if (e >= 2 * 5 * CC) return;
  const int z = e / (5 * CC), rem = e - z * 5 * CC, j = rem / CC, oi = rem - j * CC;
  double s = 0.0;
  for (int ch = 0; ch < n_chunks; ++ch) s += (double)part[(size_t)ch * 2 * 5 * CC + e];
  (z ? dw2 : dw1)[(size_t)oi * 5 + j] = (float)s;
}

// dgamma[c] / dbeta[c] = sum over samples, in sample order, of gb_part[b][0 / 1][c]
__global__ void __launch_bounds__(256) cb_gbreduce_kernel(const double* __restrict__ gb_part, int B, int C,
                                                          float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * C) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += gb_part[(size_t)b * 2 * C + e];
  (e < C ? dgamma : dbeta)[e < C ? e : e - C] = (float)s;  // rounded to f32 once
}

int cb_sample_lds_bytes(int T, int C) { return (cb_tp(T) + 2 * CB_HALO) * (C + 4) * 4 + 64; }
int cb_wgrad_lds_bytes(int T, int C) { return ((cb_tp(T) + 2 * CB_HALO) * (C + 16) + cb_tp(T) * (CB_WG_OB + 16)) * 4; }

}  // namespace

namespace vge {

int convblock_chunks(int B, int* per_chunk) {
  const int per = (B + CB_MAX_CHUNKS - 1) / CB_MAX_CHUNKS;
  if (per_chunk) *per_chunk = per;
  return (B + per - 1) / per;
}

hipError_t launch_convblock_pack(const float* W, int C, int flip, float* P, hipStream_t s) {
  hipLaunchKernelGGL(cb_pack_kernel, dim3((5 * C * C + 255) / 256), dim3(256), 0, s, W, C, flip, P);
  return hipGetLastError();
}

hipError_t launch_convblock_forward(const ConvBlockFwdArgs& a, hipStream_t s) {
  static LdsAttrOnce attr;
  const hipError_t e = attr(reinterpret_cast<const void*>(cb_forward_kernel), cb_sample_lds_bytes(64, 256));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cb_forward_kernel, dim3(a.B), dim3(256), cb_sample_lds_bytes(a.T, a.C), s, a);
  return hipGetLastError();
}

hipError_t launch_convblock_backward(const ConvBlockBwdArgs& a, hipStream_t s) {
  static LdsAttrOnce attr;
  const hipError_t e = attr(reinterpret_cast<const void*>(cb_backward_kernel), cb_sample_lds_bytes(64, 256));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cb_backward_kernel, dim3(a.B), dim3(256), cb_sample_lds_bytes(a.T, a.C), s, a);
  return hipGetLastError();
}

hipError_t launch_convblock_wgrad(const ConvBlockWgradArgs& a, float* dw1, float* dw2, hipStream_t s) {
  static LdsAttrOnce attr;
  hipError_t e = attr(reinterpret_cast<const void*>(cb_wgrad_kernel), cb_wgrad_lds_bytes(64, 256));
  if (e != hipSuccess) return e;
  int per = 0;
  const int nch = convblock_chunks(a.B, &per);
  ConvBlockWgradArgs w = a;
  w.per_chunk = per;
  const int nob = (a.C + CB_WG_OB - 1) / CB_WG_OB;
  hipLaunchKernelGGL(cb_wgrad_kernel, dim3(nch, 5 * nob, 2), dim3(256), cb_wgrad_lds_bytes(a.T, a.C), s, w);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(cb_wreduce_kernel, dim3((10 * a.C * a.C + 255) / 256), dim3(256), 0, s, a.part, nch, a.C, dw1, dw2);
  return hipGetLastError();
}

hipError_t launch_convblock_gbreduce(const double* gb_part, int B, int C, float* dgamma, float* dbeta, hipStream_t s) {
  hipLaunchKernelGGL(cb_gbreduce_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, s, gb_part, B, C, dgamma, dbeta);
  return hipGetLastError();
}

}  // namespace vge

// ------------------------------------------------------------------------------------------------ C ABI
namespace {

int fail(int code, const std::string& msg) {
  vge::set_last_error(msg);
  return code;
}

hipStream_t S(vge_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

struct Span {
  const void* p;
  size_t bytes;
  const char* name;
};

bool overlap(const Span& a, const Span& b) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
  return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// workspace layout, in floats
struct CbWs {
  size_t P0, P1, du, da, h, gb, part, total;
};
CbWs cb_ws(int B, int T, int C) {
  CbWs w;
  const size_t pw = (size_t)5 * C * C, act = (size_t)B * T * C;
  w.P0 = 0;
  w.P1 = w.P0 + pw;
  w.du = w.P1 + pw;
  w.da = w.du + act;
  w.h = w.da + act;
  w.gb = w.h + act;
  w.part = w.gb + (size_t)B * 2 * C * 2;  // gb: doubles
  w.total = w.part + (size_t)vge::convblock_chunks(B, nullptr) * 2 * pw;
  return w;
}

// the shape rule of both entries; 0 when accepted
int cb_shape(const char* fn, int B, int T, int C, int dil) {
  if (C < 32 || C > 256 || C % 32 != 0)
    return fail(VGE_ERR_UNSUPPORTED, std::string(fn) + ": C must be a multiple of 32 in [32, 256]");
  if (T < 1 || T > 64) return fail(VGE_ERR_UNSUPPORTED, std::string(fn) + ": T must be in [1, 64]");
  if (B < 1 || (long long)B * T * C > 0x7fffffffLL)
    return fail(VGE_ERR_UNSUPPORTED, std::string(fn) + ": B must be at least 1 and B T C below 2^31");
  if (dil != 1 && dil != 2 && dil != 4 && dil != 8)
    return fail(VGE_ERR_UNSUPPORTED, std::string(fn) + ": dilation must be 1, 2, 4 or 8");
  return VGE_OK;
}

// null, alignment and aliasing of the listed buffers: the first n_in are inputs (they may alias each other), the
// rest outputs (they may alias nothing); entries with p == nullptr and optional == true are skipped
int cb_buffers(const char* fn, const Span* sp, const bool* optional, int n_in, int n) {
  for (int i = 0; i < n; ++i) {
    if (!sp[i].p) {
      if (optional[i]) continue;
      return fail(VGE_ERR_ARG, std::string(fn) + ": null " + sp[i].name);
    }
    if (reinterpret_cast<uintptr_t>(sp[i].p) & 15)
      return fail(VGE_ERR_ARG, std::string(fn) + ": " + sp[i].name + " must be 16-byte aligned");
  }
  for (int i = n_in; i < n; ++i)
    for (int k = 0; k < i; ++k)
      if (sp[i].p && sp[k].p && overlap(sp[i], sp[k]))
        return fail(VGE_ERR_ARG, std::string(fn) + ": " + sp[i].name + " must not alias " + sp[k].name);
  return VGE_OK;
}

#define HIPCHK(expr)                                                                                    \
  do {                                                                                                  \
    hipError_t _e = (expr);                                                                             \
    if (_e != hipSuccess) return fail(VGE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

}  // namespace

extern "C" {

size_t vge_convblock_forward_workspace_bytes(int C) {
  if (C < 32 || C > 256 || C % 32 != 0) return 0;
  return (size_t)2 * 5 * C * C * sizeof(float);  // the two weight images: CbWs::P0, P1
}

size_t vge_convblock_workspace_bytes(int B, int T, int C) {
  if (B < 1 || T < 1 || T > 64 || C < 32 || C > 256 || C % 32 != 0 || (long long)B * T * C > 0x7fffffffLL) return 0;
  return cb_ws(B, T, C).total * sizeof(float);
}

int vge_convblock_forward(const float* x, const float* w1, const float* w2, const float* mask, const float* gamma,
                          const float* beta, int B, int T, int C, int dilation, float* a, float* u, float* mean,
                          float* rstd, float* y, void* workspace, size_t workspace_bytes, vge_stream_t stream) {
  const char* fn = "vge_convblock_forward";
  if (int st = cb_shape(fn, B, T, C, dilation)) return st;
  const size_t act = (size_t)B * T * C * 4, wb = (size_t)5 * C * C * 4;
  const bool keep = a || u || mean || rstd;  // the saved set: all four or none
  const Span sp[] = {{x, act, "x"},          {w1, wb, "w1"},        {w2, wb, "w2"},
                     {mask, act, "mask"},    {gamma, (size_t)C * 4, "gamma"}, {beta, (size_t)C * 4, "beta"},
                     {a, act, "a"},          {u, act, "u"},         {mean, (size_t)B * 4, "mean"},
                     {rstd, (size_t)B * 4, "rstd"}, {y, act, "y"},  {workspace, workspace_bytes, "workspace"}};
  const bool opt[] = {false, false, false, true, false, false, !keep, !keep, !keep, !keep, false, false};
  if (int st = cb_buffers(fn, sp, opt, 6, 12)) return st;
  if (workspace_bytes < vge_convblock_forward_workspace_bytes(C))
    return fail(VGE_ERR_WORKSPACE, std::string(fn) + ": workspace smaller than vge_convblock_forward_workspace_bytes(C)");
  float* ws = static_cast<float*>(workspace);
  const CbWs L = cb_ws(B, T, C);
  HIPCHK(vge::launch_convblock_pack(w1, C, 0, ws + L.P0, S(stream)));
  HIPCHK(vge::launch_convblock_pack(w2, C, 0, ws + L.P1, S(stream)));
  vge::ConvBlockFwdArgs A{x, mask, ws + L.P0, ws + L.P1, gamma, beta, a, u, mean, rstd, y, B, T, C, dilation};
  HIPCHK(vge::launch_convblock_forward(A, S(stream)));
  return VGE_OK;
}

int vge_convblock_backward(const float* dy, const float* x, const float* w1, const float* w2, const float* mask,
                           const float* gamma, const float* a, const float* u, const float* mean, const float* rstd,
                           int B, int T, int C, int dilation, float* dx, float* dw1, float* dw2, float* dgamma,
                           float* dbeta, void* workspace, size_t workspace_bytes, vge_stream_t stream) {
  const char* fn = "vge_convblock_backward";
  if (int st = cb_shape(fn, B, T, C, dilation)) return st;
  const size_t act = (size_t)B * T * C * 4, wb = (size_t)5 * C * C * 4;
  const Span sp[] = {{dy, act, "dy"},        {x, act, "x"},          {w1, wb, "w1"},
                     {w2, wb, "w2"},         {mask, act, "mask"},    {gamma, (size_t)C * 4, "gamma"},
                     {a, act, "a"},          {u, act, "u"},          {mean, (size_t)B * 4, "mean"},
                     {rstd, (size_t)B * 4, "rstd"}, {dx, act, "dx"}, {dw1, wb, "dw1"},
                     {dw2, wb, "dw2"},       {dgamma, (size_t)C * 4, "dgamma"}, {dbeta, (size_t)C * 4, "dbeta"},
                     {workspace, workspace_bytes, "workspace"}};
  const bool opt[] = {false, false, false, false, true, false, false, false, false, false, false, false, false, false, false, false};
  if (int st = cb_buffers(fn, sp, opt, 10, 16)) return st;
  if (workspace_bytes < vge_convblock_workspace_bytes(B, T, C))
    return fail(VGE_ERR_WORKSPACE, std::string(fn) + ": workspace smaller than vge_convblock_workspace_bytes(B, T, C)");
  float* ws = static_cast<float*>(workspace);
  const CbWs L = cb_ws(B, T, C);
  HIPCHK(vge::launch_convblock_pack(w1, C, 1, ws + L.P0, S(stream)));
  HIPCHK(vge::launch_convblock_pack(w2, C, 1, ws + L.P1, S(stream)));
  vge::ConvBlockBwdArgs A{x,  mask, a, u, mean, rstd, gamma, dy, ws + L.P0, ws + L.P1, ws + L.du, ws + L.da, ws + L.h,
                          dx, reinterpret_cast<double*>(ws + L.gb), B, T, C, dilation};
  HIPCHK(vge::launch_convblock_backward(A, S(stream)));
  vge::ConvBlockWgradArgs Wg{x, ws + L.h, ws + L.da, ws + L.du, ws + L.part, B, T, C, dilation, 0};
  HIPCHK(vge::launch_convblock_wgrad(Wg, dw1, dw2, S(stream)));
  HIPCHK(vge::launch_convblock_gbreduce(reinterpret_cast<const double*>(ws + L.gb), B, C, dgamma, dbeta, S(stream)));
  return VGE_OK;
}

}  // extern "C"
