// One post-norm, ReLU nn.TransformerEncoderLayer of the temporal stack (vge/model.py HumanActionScorer.temporal) for
// training on gfx950: a forward that keeps what the backward needs, and the backward to the input and all twelve
// parameter tensors (vge_timelayer_forward / vge_timelayer_backward, formulas in include/vge.h).
//
//   tl_gemm_kernel     the exact-f32 GEMM of vge_f32gemm.h (shared with the linear and fusion nodes), in its three
//                      operand forms, with vector loads: every extent of a layer is a multiple of 4.
//   tl_attn_fwd_kernel one workgroup = one (sample, head): q, k, v [S <= 65][d <= 64] in LDS, the logits, the softmax,
//                      P m_attn, o = (P m_attn) v.
//   tl_attn_bwd_kernel one workgroup = one (sample, head): P again from q and k, then dv, dP, dS, dq, dk.
//   tl_ln_fwd_kernel   u = x (+ z m), LayerNorm over D, one wave per row; u, mean, rstd stored on request.
//   tl_ln_bwd_kernel   one workgroup = 16 rows, one wave per row at a time: du (and du m), and the workgroup's f64
//                      partials of dgamma / dbeta.
//   tl_colsum_kernel   bias gradients: f64 column sums of one 64-row chunk.
//   tl_reduce_kernel   (vge_f32gemm.h) adds f64 chunk partials in chunk order and rounds to f32 once.
//
// Summation.  A GEMM output's K products are summed in two levels: one MFMA chain per 16 products (exact f32
// products, f32 adds), the chains added in f64, the sum rounded to f32 once.  The weight gradients do the same over
// their rows and keep the chunk partials in f64, so a weight gradient is rounded to f32 once as well.  The attention's
// products (K = d <= 64 or S <= 65) are f32 x f32 formed exactly in f64 and summed in f64, rounded once; they run on
// the vector ALU, not on the matrix cores, so no tile is padded and no padding row exists in them.  The softmax
// subtracts the row maximum; its row sum and the LayerNorms' row sums are f64 sums of f32 values.
//
// Order of every sum is fixed by (B, S, D, H): a thread owns fixed elements, wave sums are xor butterflies, wave
// partials are added in wave order, chunk partials by a second launch in chunk order.  No floating-point atomics, no
// kernel waits on another workgroup.  Nothing but the parameter gradients is summed across rows of different samples:
// a GEMM row, a LayerNorm row and an attention workgroup read one sample only.  Rows past M of a GEMM tile are zero in
// LDS and never stored.
#include "vge_common.h"

#include <string>

#include "../../include/vge.h"
#include "vge_core.h"
#include "vge_error.h"
#include "vge_f32gemm.h"
#include "vge_node_args.h"
#include "vge_lds_attr.h"

namespace {

using vge::TimeAttnArgs;
using vge::TimeGemmArgs;

constexpr int TL_LN_ROWS = 16;     // rows per workgroup of the LayerNorm backward
constexpr int TL_CS_ROWS = 64;     // rows per workgroup of the column sums
constexpr int TL_MAX_S = 65;
constexpr float TL_EPS = 1e-5f;

// ------------------------------------------------------------------------------------------------ attention
__device__ __forceinline__ int tl_ldq(int d) { return d + 1; }  // odd row stride: a column of rows is conflict-free

// rows of q, k, v (or any [R][ld] matrix's d columns from col0) of sample b into LDS [S][d + 1]
__device__ __forceinline__ void tl_load_head(float* T, const float* __restrict__ G, int ld, size_t row0, int col0, int S,
                                             int d) {
  const int d4 = d >> 2, LQ = tl_ldq(d);
  for (int i = threadIdx.x; i < S * d4; i += 256) {
    const int r = i / d4, c4 = i - r * d4;
    const floatx4 v = *reinterpret_cast<const floatx4*>(G + (row0 + r) * ld + col0 + c4 * 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) T[r * LQ + c4 * 4 + q] = v[q];
  }
}

// P[i][j] = softmax_j(<q_i, k_j> / sqrt(d)) into Pb [S][S + 1]; PM = P m_attn.  Ends with a barrier.
__device__ __forceinline__ void tl_softmax(const float* q, const float* k, float* Pb, float* PM,
                                           const float* __restrict__ m, int S, int d) {
  const int LQ = tl_ldq(d), LP = S + 1;
  const double scale = 1.0 / sqrt((double)d);
  for (int e = threadIdx.x; e < S * S; e += 256) {
    const int i = e / S, j = e - i * S;
    double s = 0.0;
    for (int c = 0; c < d; ++c) s = fma((double)q[i * LQ + c], (double)k[j * LQ + c], s);
    Pb[i * LP + j] = (float)(s * scale);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < S; i += 4) {
    const int j1 = lane + 64;
    const float s0 = lane < S ? Pb[i * LP + lane] : -INFINITY, s1 = j1 < S ? Pb[i * LP + j1] : -INFINITY;
    const float mx = wave_max(fmaxf(s0, s1));
    const float e0 = lane < S ? expf(s0 - mx) : 0.f, e1 = j1 < S ? expf(s1 - mx) : 0.f;
    const double sum = wave_sum_d((double)e0 + (double)e1);
    if (lane < S) {
      const float p = (float)((double)e0 / sum);
      Pb[i * LP + lane] = p;
      PM[i * LP + lane] = m ? p * m[(size_t)i * S + lane] : p;
    }
    if (j1 < S) {
      const float p = (float)((double)e1 / sum);
      Pb[i * LP + j1] = p;
      PM[i * LP + j1] = m ? p * m[(size_t)i * S + j1] : p;
    }
  }
  __syncthreads();
}

__host__ __device__ constexpr int tl_attn_fwd_lds_floats(int S, int d) { return 3 * S * (d + 1) + 2 * S * (S + 1); }
__host__ __device__ constexpr int tl_attn_bwd_lds_floats(int S, int d) { return 4 * S * (d + 1) + 3 * S * (S + 1); }

// grid B H.  qkv [B S][3 D] -> o [B S][D]
__global__ void __launch_bounds__(256) tl_attn_fwd_kernel(TimeAttnArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int S = A.S, d = A.D / A.H, LQ = tl_ldq(d), LP = S + 1;
  const int b = blockIdx.x / A.H, h = blockIdx.x - b * A.H;
  float* q = lds;
  float* k = q + S * LQ;
  float* v = k + S * LQ;
  float* Pb = v + S * LQ;
  float* PM = Pb + S * LP;
  const size_t row0 = (size_t)b * S;
  tl_load_head(q, A.qkv, 3 * A.D, row0, h * d, S, d);
  tl_load_head(k, A.qkv, 3 * A.D, row0, A.D + h * d, S, d);
  tl_load_head(v, A.qkv, 3 * A.D, row0, 2 * A.D + h * d, S, d);
  __syncthreads();
  tl_softmax(q, k, Pb, PM, A.m ? A.m + (size_t)blockIdx.x * S * S : nullptr, S, d);
  for (int e = threadIdx.x; e < S * d; e += 256) {
    const int i = e / d, c = e - i * d;
    double s = 0.0;
    for (int j = 0; j < S; ++j) s = fma((double)PM[i * LP + j], (double)v[j * LQ + c], s);
    A.o[(row0 + i) * A.D + h * d + c] = (float)s;
  }
}

// grid B H.  qkv, d_o [B S][D] -> dqkv [B S][3 D]
__global__ void __launch_bounds__(256) tl_attn_bwd_kernel(TimeAttnArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int S = A.S, d = A.D / A.H, LQ = tl_ldq(d), LP = S + 1;
  const int b = blockIdx.x / A.H, h = blockIdx.x - b * A.H;
  float* q = lds;
  float* k = q + S * LQ;
  float* v = k + S * LQ;
  float* dO = v + S * LQ;
  float* Pb = dO + S * LQ;
  float* PM = Pb + S * LP;
  float* DS = PM + S * LP;
  const size_t row0 = (size_t)b * S;
  const float* __restrict__ m = A.m ? A.m + (size_t)blockIdx.x * S * S : nullptr;
  tl_load_head(q, A.qkv, 3 * A.D, row0, h * d, S, d);
  tl_load_head(k, A.qkv, 3 * A.D, row0, A.D + h * d, S, d);
  tl_load_head(v, A.qkv, 3 * A.D, row0, 2 * A.D + h * d, S, d);
  tl_load_head(dO, A.d_o, A.D, row0, h * d, S, d);
  __syncthreads();
  tl_softmax(q, k, Pb, PM, m, S, d);
  // dP = (dO v^T) m_attn
  for (int e = threadIdx.x; e < S * S; e += 256) {
    const int i = e / S, j = e - i * S;
    double s = 0.0;
    for (int c = 0; c < d; ++c) s = fma((double)dO[i * LQ + c], (double)v[j * LQ + c], s);
    const float dp = (float)s;
    DS[i * LP + j] = m ? dp * m[(size_t)i * S + j] : dp;
  }
  __syncthreads();
  // dS = P (dP - sum_j dP P)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < S; i += 4) {
    const int j1 = lane + 64;
    const float d0 = lane < S ? DS[i * LP + lane] : 0.f, d1 = j1 < S ? DS[i * LP + j1] : 0.f;
    const float p0 = lane < S ? Pb[i * LP + lane] : 0.f, p1 = j1 < S ? Pb[i * LP + j1] : 0.f;
    const float dot = (float)wave_sum_d(fma((double)d0, (double)p0, (double)d1 * (double)p1));
    if (lane < S) DS[i * LP + lane] = p0 * (d0 - dot);
    if (j1 < S) DS[i * LP + j1] = p1 * (d1 - dot);
  }
  __syncthreads();
  const double scale = 1.0 / sqrt((double)d);
  for (int e = threadIdx.x; e < S * d; e += 256) {
    const int i = e / d, c = e - i * d;
    double sq = 0.0, sk = 0.0, sv = 0.0;
    for (int j = 0; j < S; ++j) {
      sq = fma((double)DS[i * LP + j], (double)k[j * LQ + c], sq);   // dq[i] = sum_j dS[i][j] k[j]
      sk = fma((double)DS[j * LP + i], (double)q[j * LQ + c], sk);   // dk[i] = sum_j dS[j][i] q[j]
      sv = fma((double)PM[j * LP + i], (double)dO[j * LQ + c], sv);  // dv[i] = sum_j (P m)[j][i] dO[j]
    }
    float* out = A.dqkv + (row0 + i) * 3 * A.D + h * d + c;
    out[0] = (float)(sq * scale);
    out[A.D] = (float)(sk * scale);
    out[2 * A.D] = (float)sv;
  }
}

// ------------------------------------------------------------------------------------------------ LayerNorm
// one wave per row, lane owns columns lane + 64 c.  u = x (+ z m); y = (u - mean) rstd gamma + beta
__global__ void __launch_bounds__(256) tl_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                        const float* __restrict__ m, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int R, int D,
                                                        float* __restrict__ u_out, float* __restrict__ mean_out,
                                                        float* __restrict__ rstd_out, float* __restrict__ y) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const size_t base = (size_t)row * D;
  float u[4];
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = lane + 64 * c;
    u[c] = 0.f;
    if (col < D) {
      float v = x[base + col];
      if (z) {
        // two roundings, as x + z * m is in torch: no contraction into one fma
        const float zz = m ? __fmul_rn(z[base + col], m[base + col]) : z[base + col];
        v = __fadd_rn(v, zz);
      }
      u[c] = v;
      if (u_out) u_out[base + col] = v;
      s += (double)v;
    }
  }
  const float mu = (float)(wave_sum_d(s) / (double)D);
  s = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (lane + 64 * c < D) {
      const double dd = (double)(u[c] - mu);
      s = fma(dd, dd, s);
    }
  const float rstd = (float)(1.0 / sqrt(wave_sum_d(s) / (double)D + (double)TL_EPS));
  if (lane == 0 && mean_out) {
    mean_out[row] = mu;
    rstd_out[row] = rstd;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = lane + 64 * c;
    if (col < D) y[base + col] = (u[c] - mu) * rstd * gamma[col] + beta[col];
  }
}

// grid ceil(R / 16).  q = dy gamma, u^ = (u - mean) rstd, du = rstd (q - mean(q) - u^ mean(q u^)); dum = du m (when
// dum is given); part[0 / 1][chunk][D] = the chunk's sums of dy u^ (dgamma) and dy (dbeta)
__global__ void __launch_bounds__(256) tl_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ u,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const float* __restrict__ gamma, const float* __restrict__ m,
                                                        int R, int D, float* __restrict__ du, float* __restrict__ dum,
                                                        double* __restrict__ part) {
  __shared__ double red[4][2][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double sg[4] = {0.0, 0.0, 0.0, 0.0}, sb[4] = {0.0, 0.0, 0.0, 0.0};
  for (int rr = wave; rr < TL_LN_ROWS; rr += 4) {
    const int row = blockIdx.x * TL_LN_ROWS + rr;
    if (row >= R) break;
    const size_t base = (size_t)row * D;
    const float mu = mean[row], rs = rstd[row];
    float q[4], xh[4];
    double pq = 0.0, pqx = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = lane + 64 * c;
      q[c] = 0.f;
      xh[c] = 0.f;
      if (col < D) {
        const float dyv = dy[base + col];
        xh[c] = (u[base + col] - mu) * rs;
        q[c] = dyv * gamma[col];
        sb[c] += (double)dyv;
        sg[c] = fma((double)dyv, (double)xh[c], sg[c]);
        pq += (double)q[c];
        pqx = fma((double)q[c], (double)xh[c], pqx);
      }
    }
    const float mq = (float)(wave_sum_d(pq) / (double)D), mqx = (float)(wave_sum_d(pqx) / (double)D);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = lane + 64 * c;
      if (col < D) {
        const float v = rs * (q[c] - mq - xh[c] * mqx);
        du[base + col] = v;
        if (dum) dum[base + col] = v * m[base + col];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    red[wave][0][lane + 64 * c] = sg[c];
    red[wave][1][lane + 64 * c] = sb[c];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * D; e += 256) {
    const int z = e / D, col = e - z * D;
    part[((size_t)z * gridDim.x + blockIdx.x) * D + col] = ((red[0][z][col] + red[1][z][col]) + red[2][z][col]) + red[3][z][col];
  }
}

// grid (ceil(R / 64), ceil(N / 256)): part[chunk][n] = sum over the chunk's rows, in row order, of src[r][n]
__global__ void __launch_bounds__(256) tl_colsum_kernel(const float* __restrict__ src, int R, int N,
                                                        double* __restrict__ part) {
  const int n = blockIdx.y * 256 + threadIdx.x;
  if (n >= N) return;
  const int r0 = blockIdx.x * TL_CS_ROWS, r1 = min(R, r0 + TL_CS_ROWS);
  double s = 0.0;
  for (int r = r0; r < r1; ++r) s += (double)src[(size_t)r * N + n];
  part[(size_t)blockIdx.x * N + n] = s;
}

}  // namespace

namespace vge {

int timelayer_wgrad_chunks(int R, int* k_per_chunk) { return tl_wgrad_chunks(R, k_per_chunk); }
int timelayer_ln_chunks(int R) { return (R + TL_LN_ROWS - 1) / TL_LN_ROWS; }
int timelayer_colsum_chunks(int R) { return (R + TL_CS_ROWS - 1) / TL_CS_ROWS; }

hipError_t launch_timelayer_reduce(const double* part, int n_chunks, int n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(tl_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, s, part, n_chunks, n, out);
  return hipGetLastError();
}

hipError_t launch_timelayer_gemm(const TimeGemmArgs& a, int form, hipStream_t s) {
  return tl_launch_gemm(a, form, false, false, s);
}

hipError_t launch_timelayer_attn_forward(const TimeAttnArgs& a, hipStream_t s) {
  static LdsAttrOnce attr;
  const hipError_t e = attr(reinterpret_cast<const void*>(tl_attn_fwd_kernel), tl_attn_fwd_lds_floats(TL_MAX_S, 64) * 4);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tl_attn_fwd_kernel, dim3(a.B * a.H), dim3(256), tl_attn_fwd_lds_floats(a.S, a.D / a.H) * 4, s, a);
  return hipGetLastError();
}

hipError_t launch_timelayer_attn_backward(const TimeAttnArgs& a, hipStream_t s) {
  static LdsAttrOnce attr;
  const hipError_t e = attr(reinterpret_cast<const void*>(tl_attn_bwd_kernel), tl_attn_bwd_lds_floats(TL_MAX_S, 64) * 4);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tl_attn_bwd_kernel, dim3(a.B * a.H), dim3(256), tl_attn_bwd_lds_floats(a.S, a.D / a.H) * 4, s, a);
  return hipGetLastError();
}

hipError_t launch_timelayer_ln_forward(const float* x, const float* z, const float* m, const float* gamma,
                                       const float* beta, int R, int D, float* u, float* mean, float* rstd, float* y,
                                       hipStream_t s) {
  hipLaunchKernelGGL(tl_ln_fwd_kernel, dim3((R + 3) / 4), dim3(256), 0, s, x, z, m, gamma, beta, R, D, u, mean, rstd, y);
  return hipGetLastError();
}

hipError_t launch_timelayer_ln_backward(const float* dy, const float* u, const float* mean, const float* rstd,
                                        const float* gamma, const float* m, int R, int D, float* du, float* dum,
                                        double* part, float* dgamma, float* dbeta, hipStream_t s) {
  const int nch = timelayer_ln_chunks(R);
  hipLaunchKernelGGL(tl_ln_bwd_kernel, dim3(nch), dim3(256), 0, s, dy, u, mean, rstd, gamma, m, R, D, du, m ? dum : nullptr,
                     part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = launch_timelayer_reduce(part, nch, D, dgamma, s)) != hipSuccess) return e;
  return launch_timelayer_reduce(part + (size_t)nch * D, nch, D, dbeta, s);
}

hipError_t launch_timelayer_colsum(const float* src, int R, int N, double* part, float* out, hipStream_t s) {
  const int nch = timelayer_colsum_chunks(R);
  hipLaunchKernelGGL(tl_colsum_kernel, dim3(nch, (N + 255) / 256), dim3(256), 0, s, src, R, N, part);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_timelayer_reduce(part, nch, N, out, s);
}

}  // namespace vge

// ------------------------------------------------------------------------------------------------ C ABI
namespace {

bool tl_shape_ok(int B, int S, int D, int H, int F) {
  if (D < 32 || D > 256 || D % 32 != 0 || H < 1 || D % H != 0) return false;
  const int d = D / H;
  if (d % 16 != 0 || d > 64 || F != 4 * D || S < 1 || S > TL_MAX_S || B < 1) return false;
  return (long long)B * S * F <= 0x7fffffffLL && (long long)B * H * S * S <= 0x7fffffffLL;
}

int tl_shape(const char* fn, int B, int S, int D, int H, int F) {
  if (tl_shape_ok(B, S, D, H, F)) return VGE_OK;
  return fail(VGE_ERR_UNSUPPORTED, std::string(fn) + ": needs D a multiple of 32 in [32, 256], H dividing D with a head "
              "dimension D / H that is a multiple of 16 and at most 64, F = 4 D, 1 <= S <= 65, B >= 1 and every tensor "
              "below 2^31 elements; got B " + std::to_string(B) + ", S " + std::to_string(S) + ", D " +
              std::to_string(D) + ", H " + std::to_string(H) + ", F " + std::to_string(F));
}

// workspace layouts, in floats (every offset a multiple of 4: R D is a multiple of 32)
struct TlFwdWs {
  size_t qkv, o, z, x1, f, g, total;
};
TlFwdWs tl_fwd_ws(int B, int S, int D, int F) {
  const size_t RD = (size_t)B * S * D, RF = (size_t)B * S * F;
  TlFwdWs w;
  w.qkv = 0;
  w.o = w.qkv + 3 * RD;
  w.z = w.o + RD;
  w.x1 = w.z + RD;
  w.f = w.x1 + RD;
  w.g = w.f + RF;
  w.total = w.g + RD;
  return w;
}

struct TlBwdWs {
  size_t dA, dM, big, xo, dB, wpart, lnpart, cspart, total;  // the last three hold doubles
};
TlBwdWs tl_bwd_ws(int B, int S, int D, int F) {
  const int R = B * S;
  const size_t RD = (size_t)R * D, RF = (size_t)R * F;
  TlBwdWs w;
  w.dA = 0;
  w.dM = w.dA + RD;
  w.big = w.dM + RD;
  w.xo = w.big + RF;
  w.dB = w.xo + RD;
  w.wpart = w.dB + RD;
  w.lnpart = w.wpart + 2 * (size_t)vge::timelayer_wgrad_chunks(R, nullptr) * D * F;
  w.cspart = w.lnpart + 2 * (size_t)vge::timelayer_ln_chunks(R) * 2 * D;
  w.total = w.cspart + 2 * (size_t)vge::timelayer_colsum_chunks(R) * F;
  return w;
}

TimeGemmArgs tl_gemm(const float* A, int lda, const float* Bm, int ldb, int M, int N, int K, float* C) {
  TimeGemmArgs g{};
  g.A = A, g.lda = lda, g.B = Bm, g.ldb = ldb, g.M = M, g.N = N, g.K = K, g.C = C, g.ldc = N;
  return g;
}

// dW [M][N] = A^T Bm over R rows (chunk partials, then the reduce), and the bias gradient = column sums of A
int tl_wgrad(const float* A, int M, const float* Bm, int N, int R, double* wpart, double* cspart, float* dW, float* db,
             hipStream_t s) {
  TimeGemmArgs g = tl_gemm(A, M, Bm, N, M, N, R, nullptr);
  g.part = wpart;
  HIPCHK(vge::launch_timelayer_gemm(g, vge::TIME_GEMM_TN, s));
  HIPCHK(vge::launch_timelayer_reduce(wpart, vge::timelayer_wgrad_chunks(R, nullptr), M * N, dW, s));
  HIPCHK(vge::launch_timelayer_colsum(A, R, M, cspart, db, s));
  return VGE_OK;
}

}  // namespace

extern "C" {

size_t vge_timelayer_forward_workspace_bytes(int B, int S, int D, int H, int F) {
  if (!tl_shape_ok(B, S, D, H, F)) return 0;
  return tl_fwd_ws(B, S, D, F).total * sizeof(float);
}

size_t vge_timelayer_workspace_bytes(int B, int S, int D, int H, int F) {
  if (!tl_shape_ok(B, S, D, H, F)) return 0;
  const size_t fw = tl_fwd_ws(B, S, D, F).total, bw = tl_bwd_ws(B, S, D, F).total;
  return (fw > bw ? fw : bw) * sizeof(float);
}

int vge_timelayer_forward(const float* x, const float* in_proj_weight, const float* in_proj_bias,
                          const float* out_proj_weight, const float* out_proj_bias, const float* linear1_weight,
                          const float* linear1_bias, const float* linear2_weight, const float* linear2_bias,
                          const float* norm1_weight, const float* norm1_bias, const float* norm2_weight,
                          const float* norm2_bias, const float* m_attn, const float* m1, const float* m_ff,
                          const float* m2, int B, int S, int D, int H, int F, float* qkv, float* u1, float* f, float* u2,
                          float* stats, float* y, void* workspace, size_t workspace_bytes, vge_stream_t stream) {
  const char* fn = "vge_timelayer_forward";
  if (int st = tl_shape(fn, B, S, D, H, F)) return st;
  const int R = B * S;
  const size_t RD = (size_t)R * D * 4, RF = (size_t)R * F * 4, v = (size_t)D * 4;
  const bool keep = qkv || u1 || f || u2 || stats;  // the saved set: all five or none
  const Span sp[] = {{x, RD, "x", false},
                     {in_proj_weight, 3 * v * D, "in_proj_weight", false},
                     {in_proj_bias, 3 * v, "in_proj_bias", false},
                     {out_proj_weight, v * D, "out_proj_weight", false},
                     {out_proj_bias, v, "out_proj_bias", false},
                     {linear1_weight, v * F, "linear1_weight", false},
                     {linear1_bias, (size_t)F * 4, "linear1_bias", false},
                     {linear2_weight, v * F, "linear2_weight", false},
                     {linear2_bias, v, "linear2_bias", false},
                     {norm1_weight, v, "norm1_weight", false},
                     {norm1_bias, v, "norm1_bias", false},
                     {norm2_weight, v, "norm2_weight", false},
                     {norm2_bias, v, "norm2_bias", false},
                     {m_attn, (size_t)B * H * S * S * 4, "m_attn", true},
                     {m1, RD, "m1", true},
                     {m_ff, RF, "m_ff", true},
                     {m2, RD, "m2", true},
                     {qkv, 3 * RD, "qkv", !keep},
                     {u1, RD, "u1", !keep},
                     {f, RF, "f", !keep},
                     {u2, RD, "u2", !keep},
                     {stats, (size_t)4 * R * 4, "stats", !keep},
                     {y, RD, "y", false},
                     {workspace, workspace_bytes, "workspace", false}};
  if (int st = tl_buffers(fn, sp, 17, 24)) return st;
  if (workspace_bytes < vge_timelayer_forward_workspace_bytes(B, S, D, H, F))
    return fail(VGE_ERR_WORKSPACE, std::string(fn) + ": workspace smaller than vge_timelayer_forward_workspace_bytes");
  float* ws = static_cast<float*>(workspace);
  const TlFwdWs L = tl_fwd_ws(B, S, D, F);
  float* qkv_ = keep ? qkv : ws + L.qkv;
  float* f_ = keep ? f : ws + L.f;
  hipStream_t s = tl_stream(stream);

  TimeGemmArgs g = tl_gemm(x, D, in_proj_weight, D, R, 3 * D, D, qkv_);
  g.bias = in_proj_bias;
  HIPCHK(vge::launch_timelayer_gemm(g, vge::TIME_GEMM_NT, s));
  TimeAttnArgs at{qkv_, m_attn, nullptr, ws + L.o, nullptr, B, S, D, H};
  HIPCHK(vge::launch_timelayer_attn_forward(at, s));
  g = tl_gemm(ws + L.o, D, out_proj_weight, D, R, D, D, ws + L.z);
  g.bias = out_proj_bias;
  HIPCHK(vge::launch_timelayer_gemm(g, vge::TIME_GEMM_NT, s));
  HIPCHK(vge::launch_timelayer_ln_forward(x, ws + L.z, m1, norm1_weight, norm1_bias, R, D, u1, keep ? stats : nullptr,
                                          keep ? stats + R : nullptr, ws + L.x1, s));
  g = tl_gemm(ws + L.x1, D, linear1_weight, D, R, F, D, f_);
  g.bias = linear1_bias, g.relu = 1, g.mask = m_ff;
  HIPCHK(vge::launch_timelayer_gemm(g, vge::TIME_GEMM_NT, s));
  g = tl_gemm(f_, F, linear2_weight, F, R, D, F, ws + L.g);
  g.bias = linear2_bias;
  HIPCHK(vge::launch_timelayer_gemm(g, vge::TIME_GEMM_NT, s));
  HIPCHK(vge::launch_timelayer_ln_forward(ws + L.x1, ws + L.g, m2, norm2_weight, norm2_bias, R, D, u2,
                                          keep ? stats + 2 * (size_t)R : nullptr, keep ? stats + 3 * (size_t)R : nullptr,
                                          y, s));
  return VGE_OK;
}

int vge_timelayer_backward(const float* dy, const float* x, const float* in_proj_weight, const float* out_proj_weight,
                           const float* linear1_weight, const float* linear2_weight, const float* norm1_weight,
                           const float* norm1_bias, const float* norm2_weight, const float* m_attn, const float* m1,
                           const float* m_ff, const float* m2, const float* qkv, const float* u1, const float* f,
                           const float* u2, const float* stats, int B, int S, int D, int H, int F, float* dx,
                           float* d_in_proj_weight, float* d_in_proj_bias, float* d_out_proj_weight,
                           float* d_out_proj_bias, float* d_linear1_weight, float* d_linear1_bias,
                           float* d_linear2_weight, float* d_linear2_bias, float* d_norm1_weight, float* d_norm1_bias,
                           float* d_norm2_weight, float* d_norm2_bias, void* workspace, size_t workspace_bytes,
                           vge_stream_t stream) {
  const char* fn = "vge_timelayer_backward";
  if (int st = tl_shape(fn, B, S, D, H, F)) return st;
  const int R = B * S;
  const size_t RD = (size_t)R * D * 4, RF = (size_t)R * F * 4, v = (size_t)D * 4;
  const Span sp[] = {{dy, RD, "dy", false},
                     {x, RD, "x", false},
                     {in_proj_weight, 3 * v * D, "in_proj_weight", false},
                     {out_proj_weight, v * D, "out_proj_weight", false},
                     {linear1_weight, v * F, "linear1_weight", false},
                     {linear2_weight, v * F, "linear2_weight", false},
                     {norm1_weight, v, "norm1_weight", false},
                     {norm1_bias, v, "norm1_bias", false},
                     {norm2_weight, v, "norm2_weight", false},
                     {m_attn, (size_t)B * H * S * S * 4, "m_attn", true},
                     {m1, RD, "m1", true},
                     {m_ff, RF, "m_ff", true},
                     {m2, RD, "m2", true},
                     {qkv, 3 * RD, "qkv", false},
                     {u1, RD, "u1", false},
                     {f, RF, "f", false},
                     {u2, RD, "u2", false},
                     {stats, (size_t)4 * R * 4, "stats", false},
                     {dx, RD, "dx", false},
                     {d_in_proj_weight, 3 * v * D, "d_in_proj_weight", false},
                     {d_in_proj_bias, 3 * v, "d_in_proj_bias", false},
                     {d_out_proj_weight, v * D, "d_out_proj_weight", false},
                     {d_out_proj_bias, v, "d_out_proj_bias", false},
                     {d_linear1_weight, v * F, "d_linear1_weight", false},
                     {d_linear1_bias, (size_t)F * 4, "d_linear1_bias", false},
                     {d_linear2_weight, v * F, "d_linear2_weight", false},
                     {d_linear2_bias, v, "d_linear2_bias", false},
                     {d_norm1_weight, v, "d_norm1_weight", false},
                     {d_norm1_bias, v, "d_norm1_bias", false},
                     {d_norm2_weight, v, "d_norm2_weight", false},
                     {d_norm2_bias, v, "d_norm2_bias", false},
                     {workspace, workspace_bytes, "workspace", false}};
  if (int st = tl_buffers(fn, sp, 18, 32)) return st;
  if (workspace_bytes < vge_timelayer_workspace_bytes(B, S, D, H, F))
    return fail(VGE_ERR_WORKSPACE, std::string(fn) + ": workspace smaller than vge_timelayer_workspace_bytes");
  float* ws = static_cast<float*>(workspace);
  const TlBwdWs L = tl_bwd_ws(B, S, D, F);
  float *dA = ws + L.dA, *dM = ws + L.dM, *big = ws + L.big, *xo = ws + L.xo, *dB = ws + L.dB;
  double* wpart = reinterpret_cast<double*>(ws + L.wpart);
  double* lnpart = reinterpret_cast<double*>(ws + L.lnpart);
  double* cspart = reinterpret_cast<double*>(ws + L.cspart);
  const float *mean1 = stats, *rstd1 = stats + R, *mean2 = stats + 2 * (size_t)R, *rstd2 = stats + 3 * (size_t)R;
  hipStream_t s = tl_stream(stream);

  // the second LayerNorm: du2 (dA), dg = du2 m2 (dM)
  HIPCHK(vge::launch_timelayer_ln_backward(dy, u2, mean2, rstd2, norm2_weight, m2, R, D, dA, dM, lnpart, d_norm2_weight,
                                           d_norm2_bias, s));
  const float* dg = m2 ? dM : dA;
  // x1 again from u1 (xo)
  HIPCHK(vge::launch_timelayer_ln_forward(u1, nullptr, nullptr, norm1_weight, norm1_bias, R, D, nullptr, nullptr, nullptr,
                                          xo, s));
  // the feed-forward: dW2 = dg^T f, dc2; da1 = (dg W2) [f > 0] m_ff (big); dW1 = da1^T x1, dc1; dx1 = du2 + da1 W1 (dB)
  if (int st = tl_wgrad(dg, D, f, F, R, wpart, cspart, d_linear2_weight, d_linear2_bias, s)) return st;
  TimeGemmArgs g = tl_gemm(dg, D, linear2_weight, F, R, F, D, big);
  g.mask = m_ff, g.gate = f;
  HIPCHK(vge::launch_timelayer_gemm(g, vge::TIME_GEMM_NN, s));
  if (int st = tl_wgrad(big, F, xo, D, R, wpart, cspart, d_linear1_weight, d_linear1_bias, s)) return st;
  g = tl_gemm(big, F, linear1_weight, D, R, D, F, dB);
  g.res = dA;
  HIPCHK(vge::launch_timelayer_gemm(g, vge::TIME_GEMM_NN, s));
  // the first LayerNorm: du1 (dA), dz = du1 m1 (dM)
  HIPCHK(vge::launch_timelayer_ln_backward(dB, u1, mean1, rstd1, norm1_weight, m1, R, D, dA, dM, lnpart, d_norm1_weight,
                                           d_norm1_bias, s));
  const float* dz = m1 ? dM : dA;
  // o again from qkv (xo); dWo = dz^T o, db_o; do = dz Wo (dB)
  TimeAttnArgs at{qkv, m_attn, nullptr, xo, nullptr, B, S, D, H};
  HIPCHK(vge::launch_timelayer_attn_forward(at, s));
  if (int st = tl_wgrad(dz, D, xo, D, R, wpart, cspart, d_out_proj_weight, d_out_proj_bias, s)) return st;
  g = tl_gemm(dz, D, out_proj_weight, D, R, D, D, dB);
  HIPCHK(vge::launch_timelayer_gemm(g, vge::TIME_GEMM_NN, s));
  // the attention: dqkv (big); dWin = dqkv^T x, db_in; dx = du1 + dqkv Win
  at = TimeAttnArgs{qkv, m_attn, dB, nullptr, big, B, S, D, H};
  HIPCHK(vge::launch_timelayer_attn_backward(at, s));
  if (int st = tl_wgrad(big, 3 * D, x, D, R, wpart, cspart, d_in_proj_weight, d_in_proj_bias, s)) return st;
  g = tl_gemm(big, 3 * D, in_proj_weight, D, R, D, 3 * D, dx);
  g.res = dA;
  HIPCHK(vge::launch_timelayer_gemm(g, vge::TIME_GEMM_NN, s));
  return VGE_OK;
}

}  // extern "C"
