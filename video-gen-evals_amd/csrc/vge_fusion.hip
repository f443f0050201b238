// The modality fusion (vge/model.py _Fusion, with the affine-free LayerNorm in front of it) for training on gfx950: a
// forward that keeps what the backward needs, and the backward to the stacked per-modality sums and all eleven
// parameter tensors (vge_fusion_forward / vge_fusion_backward, formulas in include/vge.h).
//
// The node is the folded form of the module's graph.  Wk never meets a token: the logit of modality m is <kv_m, u>
// with u = Wk^T qv, one vector for every row, as the inference fuse kernel has it.  Wv commutes with the attention's
// weighted sum, so Wv and Wo run over the R pooled rows p, not over the R M tokens.
//
//   fu_query_fwd_kernel  one workgroup: ql = LN(latent) g_q + b_q, qv = Wq ql, u = Wk^T qv (row-independent).
//   fu_rows_fwd_kernel   one wave per row: per modality LN0 (no affine), kv_ln, the logit; the softmax over M, the
//                        dropout multiplier, p = sum_m ad_m kv_m.
//   (vge_linear.hip)     vp = p Wv^T, out = vp Wo^T; in the backward dWo, dvp, dWv, dp: the linear node's GEMMs.
//   fu_rows_bwd_kernel   one workgroup = 16 rows, one wave per row at a time: t and kv again from s and the saved
//                        statistics, the softmax backward, the two LayerNorm backwards, ds; and the workgroup's f64
//                        partials of du, dg_kv, db_kv, dbias and the logit scale's gradient.
//   (tl_reduce_kernel)   adds the partials in workgroup order (vge_f32gemm.h, through launch_timelayer_reduce).
//   fu_query_bwd_kernel  one workgroup: from the summed du  dWk = qv (x) du, dqv = Wk du, dWq = dqv (x) ql,
//                        dql = Wq^T dqv, the q_ln backward to dlatent, dg_q, db_q; dtemp from the scale's gradient.
//
// Sums.  Row sums (LayerNorm means and variances, the M + M dot products of a row, the softmax sum, the pooling) are
// f64 sums of f32 values or of exact f32 x f32 products, rounded once; the softmax subtracts the row maximum.  The
// GEMMs follow vge_f32gemm.h.  The matrix-vector products of the two query kernels are f64 sums in index order.
// Nothing but parameter gradients is summed across rows, and each of those is f64 partials per 16 rows in the
// workspace added by a second launch in chunk order.  No floating-point atomics, no kernel waits on another
// workgroup; the order of every sum is fixed by (R, M, D).
#include "vge_common.h"
#include "vge_core.h"
#include "vge_node_args.h"

namespace {

using vge::FusionQueryArgs;
using vge::FusionRowArgs;

constexpr int FU_MAX_M = 8;
constexpr int FU_ROWS = 16;        // rows per workgroup of the row backward
constexpr int FU_SCAL = 16;        // scalar sums per partial: dbias[8], dscale[8]
constexpr float FU_EPS = 1e-5f;

// c_m = 1 / sqrt(D) / (softplus(temp_m) + 1e-3); torch's softplus is the identity above 20
__device__ __forceinline__ double fu_softplus(double t) { return t > 20.0 ? t : log1p(exp(t)); }
__device__ __forceinline__ double fu_scale(float temp, int D) {
  return 1.0 / sqrt((double)D) / (fu_softplus((double)temp) + 1e-3);
}

// (v - mean) rstd of the wave's row, lane owning columns lane + 64 c; dead columns stay 0
__device__ __forceinline__ void fu_ln(const float (&v)[4], const bool (&live)[4], int D, float (&h)[4], float& mean,
                                      float& rstd) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (live[c]) s += (double)v[c];
  mean = (float)(wave_sum_d(s) / (double)D);
  s = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (live[c]) {
      const double dd = (double)(v[c] - mean);
      s = fma(dd, dd, s);
    }
  rstd = (float)(1.0 / sqrt(wave_sum_d(s) / (double)D + (double)FU_EPS));
#pragma unroll
  for (int c = 0; c < 4; ++c) h[c] = live[c] ? (v[c] - mean) * rstd : 0.f;
}

// dv = rstd (q - mean_D(q) - h mean_D(q h)) of the wave's row
__device__ __forceinline__ void fu_ln_bwd(const float (&q)[4], const float (&h)[4], const bool (&live)[4], int D,
                                          float rstd, float (&dv)[4]) {
  double pq = 0.0, pqh = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (live[c]) {
      pq += (double)q[c];
      pqh = fma((double)q[c], (double)h[c], pqh);
    }
  const float mq = (float)(wave_sum_d(pq) / (double)D), mqh = (float)(wave_sum_d(pqh) / (double)D);
#pragma unroll
  for (int c = 0; c < 4; ++c) dv[c] = live[c] ? rstd * (q[c] - mq - h[c] * mqh) : 0.f;
}

__device__ __forceinline__ double fu_dot(const float (&a)[4], const float (&b)[4]) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) s = fma((double)a[c], (double)b[c], s);  // dead columns hold 0
  return wave_sum_d(s);
}

// ------------------------------------------------------------------------------------------------ the query
// mean and rstd of latent, every thread for itself (D <= 256 values, the same order in every thread)
__device__ __forceinline__ void fu_latent_stats(const float* __restrict__ latent, int D, float& mean, float& rstd) {
  double s = 0.0;
  for (int k = 0; k < D; ++k) s += (double)latent[k];
  mean = (float)(s / (double)D);
  s = 0.0;
  for (int k = 0; k < D; ++k) {
    const double dd = (double)(latent[k] - mean);
    s = fma(dd, dd, s);
  }
  rstd = (float)(1.0 / sqrt(s / (double)D + (double)FU_EPS));
}

// grid 1.  qvec [3][D] = ql, qv, u
__global__ void __launch_bounds__(256) fu_query_fwd_kernel(FusionQueryArgs A) {
  __shared__ float ql[256], qv[256];
  const int j = threadIdx.x, D = A.D;
  float mean, rstd;
  fu_latent_stats(A.latent, D, mean, rstd);
  if (j < D) {
    ql[j] = (A.latent[j] - mean) * rstd * A.g_q[j] + A.b_q[j];
    A.qvec[j] = ql[j];
  }
  __syncthreads();
  if (j < D) {
    double s = 0.0;
    for (int k = 0; k < D; ++k) s = fma((double)A.Wq[(size_t)j * D + k], (double)ql[k], s);
    qv[j] = (float)s;
    A.qvec[D + j] = qv[j];
  }
  __syncthreads();
  if (j < D) {
    double s = 0.0;
    for (int n = 0; n < D; ++n) s = fma((double)A.Wk[(size_t)n * D + j], (double)qv[n], s);
    A.qvec[2 * D + j] = (float)s;
  }
}

// grid 1.  sums [3 D + 16] = du, dg_kv, db_kv, dbias[8], dscale[8]
__global__ void __launch_bounds__(256) fu_query_bwd_kernel(FusionQueryArgs A) {
  __shared__ float du[256], dqv[256], dql[256], hat[256];
  const int j = threadIdx.x, D = A.D;
  const float* __restrict__ ql = A.qvec;
  const float* __restrict__ qv = A.qvec + D;
  float mean, rstd;
  fu_latent_stats(A.latent, D, mean, rstd);
  if (j < D) {
    du[j] = A.sums[j];
    A.d_g_kv[j] = A.sums[D + j];
    A.d_b_kv[j] = A.sums[2 * D + j];
    hat[j] = (A.latent[j] - mean) * rstd;
  }
  if (j < A.M) {
    A.d_bias[j] = A.sums[3 * D + j];
    // c = isd / (softplus(t) + 1e-3):  dc / dt = -c sigmoid(t) / (softplus(t) + 1e-3)
    const double t = (double)A.temp[j], sp = fu_softplus(t) + 1e-3;
    const double sig = t > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-t));
    A.d_temp[j] = (float)((double)A.sums[3 * D + 8 + j] * (-fu_scale(A.temp[j], D) * sig / sp));
  }
  __syncthreads();
  if (j < D) {  // dqv = Wk du
    double s = 0.0;
    for (int k = 0; k < D; ++k) s = fma((double)A.Wk[(size_t)j * D + k], (double)du[k], s);
    dqv[j] = (float)s;
  }
  __syncthreads();
  if (j < D) {  // dql = Wq^T dqv
    double s = 0.0;
    for (int n = 0; n < D; ++n) s = fma((double)A.Wq[(size_t)n * D + j], (double)dqv[n], s);
    dql[j] = (float)s;
    A.d_g_q[j] = dql[j] * hat[j];
    A.d_b_q[j] = dql[j];
  }
  __syncthreads();
  for (int e = j; e < D * D; e += 256) {
    const int n = e / D, k = e - n * D;
    A.d_Wk[e] = qv[n] * du[k];
    A.d_Wq[e] = dqv[n] * ql[k];
  }
  if (j < D) {
    double pq = 0.0, pqh = 0.0;
    for (int k = 0; k < D; ++k) {
      const float q = dql[k] * A.g_q[k];
      pq += (double)q;
      pqh = fma((double)q, (double)hat[k], pqh);
    }
    const float mq = (float)(pq / (double)D), mqh = (float)(pqh / (double)D);
    A.d_latent[j] = rstd * (dql[j] * A.g_q[j] - mq - hat[j] * mqh);
  }
}

// ------------------------------------------------------------------------------------------------ the rows
// grid ceil(R / 4), one wave per row
__global__ void __launch_bounds__(256) fu_rows_fwd_kernel(FusionRowArgs A) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= A.R) return;
  const int D = A.D, M = A.M;
  const size_t RM = (size_t)A.R * M;
  bool live[4];
  float g[4], b[4], u[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = lane + 64 * c;
    live[c] = col < D;
    g[c] = live[c] ? A.g_kv[col] : 0.f;
    b[c] = live[c] ? A.b_kv[col] : 0.f;
    u[c] = live[c] ? A.qvec[2 * D + col] : 0.f;
  }
  float kv[FU_MAX_M][4], l[FU_MAX_M];
  float mx = -INFINITY;
#pragma unroll
  for (int m = 0; m < FU_MAX_M; ++m) {
    if (m < M) {
      const size_t tok = (size_t)row * M + m;
      float sv[4], t[4], h[4], mean0, rstd0, mean1, rstd1;
#pragma unroll
      for (int c = 0; c < 4; ++c) sv[c] = live[c] ? A.s[tok * D + lane + 64 * c] : 0.f;
      fu_ln(sv, live, D, t, mean0, rstd0);
      fu_ln(t, live, D, h, mean1, rstd1);
#pragma unroll
      for (int c = 0; c < 4; ++c) kv[m][c] = live[c] ? h[c] * g[c] + b[c] : 0.f;
      l[m] = (float)(fu_dot(kv[m], u) * fu_scale(A.temp[m], D) + (double)A.bias[m]);
      mx = fmaxf(mx, l[m]);
      if (A.stats && lane == 0) {
        A.stats[tok] = mean0;
        A.stats[RM + tok] = rstd0;
        A.stats[2 * RM + tok] = mean1;
        A.stats[3 * RM + tok] = rstd1;
      }
    }
  }
  double sum = 0.0;
#pragma unroll
  for (int m = 0; m < FU_MAX_M; ++m)
    if (m < M) {
      l[m] = expf(l[m] - mx);
      sum += (double)l[m];
    }
  double p[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int m = 0; m < FU_MAX_M; ++m)
    if (m < M) {
      const size_t tok = (size_t)row * M + m;
      const float a = (float)((double)l[m] / sum);
      const float ad = A.m ? a * A.m[tok] : a;
      if (A.a && lane == 0) A.a[tok] = a;
#pragma unroll
      for (int c = 0; c < 4; ++c) p[c] = fma((double)ad, (double)kv[m][c], p[c]);
    }
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (live[c]) A.p[(size_t)row * D + lane + 64 * c] = (float)p[c];
}

// grid ceil(R / 16).  part[chunk][3 D + 16]
__global__ void __launch_bounds__(256) fu_rows_bwd_kernel(FusionRowArgs A) {
  __shared__ double red[4][3][256];
  __shared__ double red_s[4][FU_SCAL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = A.D, M = A.M;
  const size_t RM = (size_t)A.R * M;
  bool live[4];
  float g[4], b[4], u[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = lane + 64 * c;
    live[c] = col < D;
    g[c] = live[c] ? A.g_kv[col] : 0.f;
    b[c] = live[c] ? A.b_kv[col] : 0.f;
    u[c] = live[c] ? A.qvec[2 * D + col] : 0.f;
  }
  double cm[FU_MAX_M];
#pragma unroll
  for (int m = 0; m < FU_MAX_M; ++m) cm[m] = m < M ? fu_scale(A.temp[m], D) : 0.0;
  double s_du[4] = {0.0, 0.0, 0.0, 0.0}, s_dg[4] = {0.0, 0.0, 0.0, 0.0}, s_db[4] = {0.0, 0.0, 0.0, 0.0};
  double s_sc[FU_SCAL];
#pragma unroll
  for (int i = 0; i < FU_SCAL; ++i) s_sc[i] = 0.0;

  for (int rr = wave; rr < FU_ROWS; rr += 4) {
    const int row = blockIdx.x * FU_ROWS + rr;
    if (row >= A.R) break;
    float dp[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) dp[c] = live[c] ? A.dp[(size_t)row * D + lane + 64 * c] : 0.f;
    float t[FU_MAX_M][4], h[FU_MAX_M][4], a[FU_MAX_M], mk[FU_MAX_M], da[FU_MAX_M], ku[FU_MAX_M];
    double dot = 0.0;
#pragma unroll
    for (int m = 0; m < FU_MAX_M; ++m)
      if (m < M) {
        const size_t tok = (size_t)row * M + m;
        const float mean0 = A.stats[tok], rstd0 = A.stats[RM + tok], mean1 = A.stats[2 * RM + tok],
                    rstd1 = A.stats[3 * RM + tok];
        float kv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          t[m][c] = live[c] ? (A.s[tok * D + lane + 64 * c] - mean0) * rstd0 : 0.f;
          h[m][c] = live[c] ? (t[m][c] - mean1) * rstd1 : 0.f;
          kv[c] = live[c] ? h[m][c] * g[c] + b[c] : 0.f;
        }
        a[m] = A.a[tok];
        mk[m] = A.m ? A.m[tok] : 1.f;
        da[m] = (float)fu_dot(dp, kv) * mk[m];  // d(loss) / d a_m
        ku[m] = (float)fu_dot(kv, u);
        dot = fma((double)a[m], (double)da[m], dot);
      }
    const float dotf = (float)dot;
#pragma unroll
    for (int m = 0; m < FU_MAX_M; ++m)
      if (m < M) {
        const size_t tok = (size_t)row * M + m;
        const float dl = a[m] * (da[m] - dotf);  // d(loss) / d logit_m
        s_sc[m] += (double)dl;
        s_sc[8 + m] = fma((double)dl, (double)ku[m], s_sc[8 + m]);
        const float w1 = a[m] * mk[m], w2 = (float)((double)dl * cm[m]);
        float dh[4], dt[4], dsv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float kvc = h[m][c] * g[c] + b[c];
          const float dkv = live[c] ? w1 * dp[c] + w2 * u[c] : 0.f;
          if (live[c]) {
            s_du[c] = fma((double)w2, (double)kvc, s_du[c]);
            s_dg[c] = fma((double)dkv, (double)h[m][c], s_dg[c]);
            s_db[c] += (double)dkv;
          }
          dh[c] = dkv * g[c];
        }
        fu_ln_bwd(dh, h[m], live, D, A.stats[3 * RM + tok], dt);
        fu_ln_bwd(dt, t[m], live, D, A.stats[RM + tok], dsv);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (live[c]) A.ds[tok * D + lane + 64 * c] = dsv[c];
      }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    red[wave][0][lane + 64 * c] = s_du[c];
    red[wave][1][lane + 64 * c] = s_dg[c];
    red[wave][2][lane + 64 * c] = s_db[c];
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < FU_SCAL; ++i) red_s[wave][i] = s_sc[i];
  }
  __syncthreads();
  const int W = 3 * D + FU_SCAL;
  double* __restrict__ out = A.part + (size_t)blockIdx.x * W;
  for (int e = threadIdx.x; e < W; e += 256) {
    if (e < 3 * D) {
      const int z = e / D, col = e - z * D;
      out[e] = ((red[0][z][col] + red[1][z][col]) + red[2][z][col]) + red[3][z][col];
    } else {
      const int i = e - 3 * D;
      out[e] = ((red_s[0][i] + red_s[1][i]) + red_s[2][i]) + red_s[3][i];
    }
  }
}

bool fu_shape_ok(long long R, long long M, long long D) {
  if (R < 1 || M < 1 || M > FU_MAX_M || D < 32 || D > 256 || D % 32 != 0) return false;
  return R * M * D <= 0x7fffffffLL;
}

int fu_shape(const char* fn, int R, int M, int D) {
  if (fu_shape_ok(R, M, D)) return VGE_OK;
  return fail(VGE_ERR_UNSUPPORTED, std::string(fn) + ": needs R >= 1, 1 <= M <= 8, D a multiple of 32 in [32, 256] and "
              "R M D < 2^31; got R " + std::to_string(R) + ", M " + std::to_string(M) + ", D " + std::to_string(D));
}

// workspace layouts, in floats (every offset a multiple of 4; the partials, doubles, start on an even offset)
struct FuFwdWs {
  size_t qvec, p, vp, total;
};
FuFwdWs fu_fwd_ws(int R, int D) {
  FuFwdWs w;
  w.qvec = 0;
  w.p = w.qvec + 3 * (size_t)D;
  w.vp = w.p + (size_t)R * D;
  w.total = w.vp + (size_t)R * D;
  return w;
}
struct FuBwdWs {
  size_t qvec, sums, dvp, dp, wpart, rpart, total;  // the last two hold doubles
};
FuBwdWs fu_bwd_ws(int R, int D) {
  FuBwdWs w;
  w.qvec = 0;
  w.sums = w.qvec + 3 * (size_t)D;
  w.dvp = w.sums + 3 * (size_t)D + FU_SCAL;
  w.dp = w.dvp + (size_t)R * D;
  w.wpart = w.dp + (size_t)R * D;
  w.rpart = w.wpart + 2 * (size_t)vge::linear_wgrad_chunks(R) * D * D;
  w.total = w.rpart + 2 * (size_t)vge::fusion_row_chunks(R) * (3 * (size_t)D + FU_SCAL);
  return w;
}

}  // namespace

namespace vge {

int fusion_row_chunks(int R) { return (R + FU_ROWS - 1) / FU_ROWS; }

hipError_t launch_fusion_query_forward(const FusionQueryArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(fu_query_fwd_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_fusion_query_backward(const FusionQueryArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(fu_query_bwd_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_fusion_rows_forward(const FusionRowArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(fu_rows_fwd_kernel, dim3((a.R + 3) / 4), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_fusion_rows_backward(const FusionRowArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(fu_rows_bwd_kernel, dim3(fusion_row_chunks(a.R)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace vge

extern "C" {

size_t vge_fusion_forward_workspace_bytes(int R, int M, int D) {
  if (!fu_shape_ok(R, M, D)) return 0;
  return fu_fwd_ws(R, D).total * sizeof(float);
}

size_t vge_fusion_workspace_bytes(int R, int M, int D) {
  if (!fu_shape_ok(R, M, D)) return 0;
  const size_t fw = fu_fwd_ws(R, D).total, bw = fu_bwd_ws(R, D).total;
  return (fw > bw ? fw : bw) * sizeof(float);
}

int vge_fusion_forward(const float* s, const float* latent, const float* q_ln_weight, const float* q_ln_bias,
                       const float* kv_ln_weight, const float* kv_ln_bias, const float* Wq, const float* Wk,
                       const float* Wv, const float* Wo, const float* logit_temp, const float* logit_bias,
                       const float* m_attn, int R, int M, int D, float* stats, float* a, float* p, float* vp, float* out,
                       void* workspace, size_t workspace_bytes, vge_stream_t stream) {
  const char* fn = "vge_fusion_forward";
  if (int st = fu_shape(fn, R, M, D)) return st;
  const size_t RD = (size_t)R * D * 4, RM = (size_t)R * M * 4, v = (size_t)D * 4, mv = (size_t)M * 4;
  const bool keep = stats || a || p || vp;  // the saved set: all four or none
  const Span sp[] = {{s, RD * M, "s", false},
                     {latent, v, "latent", false},
                     {q_ln_weight, v, "q_ln_weight", false},
                     {q_ln_bias, v, "q_ln_bias", false},
                     {kv_ln_weight, v, "kv_ln_weight", false},
                     {kv_ln_bias, v, "kv_ln_bias", false},
                     {Wq, v * D, "Wq", false},
                     {Wk, v * D, "Wk", false},
                     {Wv, v * D, "Wv", false},
                     {Wo, v * D, "Wo", false},
                     {logit_temp, mv, "logit_temp", false},
                     {logit_bias, mv, "logit_bias", false},
                     {m_attn, RM, "m_attn", true},
                     {stats, 4 * RM, "stats", !keep},
                     {a, RM, "a", !keep},
                     {p, RD, "p", !keep},
                     {vp, RD, "vp", !keep},
                     {out, RD, "out", false},
                     {workspace, workspace_bytes, "workspace", false}};
  if (int st = tl_buffers(fn, sp, 13, 19)) return st;
  if (workspace_bytes < vge_fusion_forward_workspace_bytes(R, M, D))
    return fail(VGE_ERR_WORKSPACE, std::string(fn) + ": workspace smaller than vge_fusion_forward_workspace_bytes");
  float* ws = static_cast<float*>(workspace);
  const FuFwdWs L = fu_fwd_ws(R, D);
  float* p_ = keep ? p : ws + L.p;
  float* vp_ = keep ? vp : ws + L.vp;
  hipStream_t st = tl_stream(stream);

  vge::FusionQueryArgs q{};
  q.latent = latent, q.g_q = q_ln_weight, q.b_q = q_ln_bias, q.Wq = Wq, q.Wk = Wk, q.qvec = ws + L.qvec, q.M = M, q.D = D;
  HIPCHK(vge::launch_fusion_query_forward(q, st));
  vge::FusionRowArgs r{};
  r.s = s, r.g_kv = kv_ln_weight, r.b_kv = kv_ln_bias, r.temp = logit_temp, r.bias = logit_bias, r.m = m_attn;
  r.qvec = ws + L.qvec, r.stats = stats, r.a = a, r.p = p_, r.R = R, r.M = M, r.D = D;
  HIPCHK(vge::launch_fusion_rows_forward(r, st));
  HIPCHK(vge::launch_linear_forward(p_, D, Wv, vp_, R, D, D, st));
  HIPCHK(vge::launch_linear_forward(vp_, D, Wo, out, R, D, D, st));
  return VGE_OK;
}

int vge_fusion_backward(const float* d_out, const float* s, const float* latent, const float* q_ln_weight,
                        const float* q_ln_bias, const float* kv_ln_weight, const float* kv_ln_bias, const float* Wq,
                        const float* Wk, const float* Wv, const float* Wo, const float* logit_temp,
                        const float* logit_bias, const float* m_attn, const float* stats, const float* a, const float* p,
                        const float* vp, int R, int M, int D, float* ds, float* d_latent, float* d_q_ln_weight,
                        float* d_q_ln_bias, float* d_kv_ln_weight, float* d_kv_ln_bias, float* d_Wq, float* d_Wk,
                        float* d_Wv, float* d_Wo, float* d_logit_temp, float* d_logit_bias, void* workspace,
                        size_t workspace_bytes, vge_stream_t stream) {
  const char* fn = "vge_fusion_backward";
  if (int st = fu_shape(fn, R, M, D)) return st;
  const size_t RD = (size_t)R * D * 4, RM = (size_t)R * M * 4, v = (size_t)D * 4, mv = (size_t)M * 4;
  const Span sp[] = {{d_out, RD, "d_out", false},
                     {s, RD * M, "s", false},
                     {latent, v, "latent", false},
                     {q_ln_weight, v, "q_ln_weight", false},
                     {q_ln_bias, v, "q_ln_bias", false},
                     {kv_ln_weight, v, "kv_ln_weight", false},
                     {kv_ln_bias, v, "kv_ln_bias", false},
                     {Wq, v * D, "Wq", false},
                     {Wk, v * D, "Wk", false},
                     {Wv, v * D, "Wv", false},
                     {Wo, v * D, "Wo", false},
                     {logit_temp, mv, "logit_temp", false},
                     {logit_bias, mv, "logit_bias", false},
                     {m_attn, RM, "m_attn", true},
                     {stats, 4 * RM, "stats", false},
                     {a, RM, "a", false},
                     {p, RD, "p", false},
                     {vp, RD, "vp", false},
                     {ds, RD * M, "ds", false},
                     {d_latent, v, "d_latent", false},
                     {d_q_ln_weight, v, "d_q_ln_weight", false},
                     {d_q_ln_bias, v, "d_q_ln_bias", false},
                     {d_kv_ln_weight, v, "d_kv_ln_weight", false},
                     {d_kv_ln_bias, v, "d_kv_ln_bias", false},
                     {d_Wq, v * D, "d_Wq", false},
                     {d_Wk, v * D, "d_Wk", false},
                     {d_Wv, v * D, "d_Wv", false},
                     {d_Wo, v * D, "d_Wo", false},
                     {d_logit_temp, mv, "d_logit_temp", false},
                     {d_logit_bias, mv, "d_logit_bias", false},
                     {workspace, workspace_bytes, "workspace", false}};
  if (int st = tl_buffers(fn, sp, 18, 31)) return st;
  if (workspace_bytes < vge_fusion_workspace_bytes(R, M, D))
    return fail(VGE_ERR_WORKSPACE, std::string(fn) + ": workspace smaller than vge_fusion_workspace_bytes");
  float* ws = static_cast<float*>(workspace);
  const FuBwdWs L = fu_bwd_ws(R, D);
  float *qvec = ws + L.qvec, *sums = ws + L.sums, *dvp = ws + L.dvp, *dp = ws + L.dp;
  double* wpart = reinterpret_cast<double*>(ws + L.wpart);
  double* rpart = reinterpret_cast<double*>(ws + L.rpart);
  hipStream_t st = tl_stream(stream);

  vge::FusionQueryArgs q{};
  q.latent = latent, q.g_q = q_ln_weight, q.b_q = q_ln_bias, q.Wq = Wq, q.Wk = Wk, q.qvec = qvec, q.M = M, q.D = D;
  HIPCHK(vge::launch_fusion_query_forward(q, st));
  // out = vp Wo^T, vp = p Wv^T
  HIPCHK(vge::launch_linear_wgrad(d_out, vp, D, wpart, d_Wo, R, D, D, st));
  HIPCHK(vge::launch_linear_dgrad(d_out, Wo, dvp, R, D, D, st));
  HIPCHK(vge::launch_linear_wgrad(dvp, p, D, wpart, d_Wv, R, D, D, st));
  HIPCHK(vge::launch_linear_dgrad(dvp, Wv, dp, R, D, D, st));
  vge::FusionRowArgs r{};
  r.s = s, r.g_kv = kv_ln_weight, r.b_kv = kv_ln_bias, r.temp = logit_temp, r.bias = logit_bias, r.m = m_attn;
  r.qvec = qvec, r.stats = const_cast<float*>(stats), r.a = const_cast<float*>(a), r.dp = dp, r.ds = ds, r.part = rpart;
  r.R = R, r.M = M, r.D = D;
  HIPCHK(vge::launch_fusion_rows_backward(r, st));
  HIPCHK(vge::launch_timelayer_reduce(rpart, vge::fusion_row_chunks(R), 3 * D + FU_SCAL, sums, st));
  q.sums = sums, q.temp = logit_temp;
  q.d_latent = d_latent, q.d_g_q = d_q_ln_weight, q.d_b_q = d_q_ln_bias, q.d_g_kv = d_kv_ln_weight;
  q.d_b_kv = d_kv_ln_bias, q.d_Wq = d_Wq, q.d_Wk = d_Wk, q.d_temp = d_logit_temp, q.d_bias = d_logit_bias;
  HIPCHK(vge::launch_fusion_query_backward(q, st));
  return VGE_OK;
}

}  // extern "C"
