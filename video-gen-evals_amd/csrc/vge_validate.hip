// Held-out validation loss of a checkpoint (gfx950): the forward-only selection criterion of the reference's
// training loop (train.py:286-333 evaluate_test_set, train.py:335-399 evaluate_test_set_centroid_distance).
//
//   time_gather_kernel     out[b,t,:] = feats[b, src[b,t], :] -- the three hard-negative window variants of
//                          utils.py:65-95 (partial shuffle / reverse / static) as one index table.  Pure copy,
//                          16-byte accesses; HBM-bound: one read and one write of the batch.
//   tcl_den_kernel         losses.py:31 denominators: den_j = sum_{k in P(j)} e_jk + k1 sum_{k in P(j)} exp(-s_jk)
//                          + k2 sum_{k in N(j)} e_jk, s = <z_j, z_k>, e = exp(s / temperature).
//   tcl_row_kernel         loss_i = (1 / |P(i)|) sum_{j in P(i)} -log(e_ij / den_j): the reference's [B,B] / [B]
//                          broadcast divides element (i,j) by the denominator of row j.  |P(i)| = 0 gives 0/0 = NaN,
//                          as the reference does (the caller skips such a batch, train.py:312-313).
//   mean_kernel            mean_i loss_i (losses.py:33).
//   hardneg_kernel         SupConWithHardNegatives(anchor, anchor, neg) (losses.py:37-56): cross entropy of the two
//                          logits (<a,a>, <a,n>) / temperature against class 0, mean over the batch.
//   centroid_dist_kernel   || normalize(emb_i) - centroid[label_i] ||_2 (train.py:366-378).
// and the gradients of the two losses for the training step (vge_tcl_loss_grad / vge_hardneg_loss_grad; the loss
// itself comes from the forward kernels above, launched as they are):
//   tcl_count_kernel       |P(j)| per row.
//   tcl_grad_kernel        grad_j = (1 / B) sum_k (W_jk + W_kj) z_k, the dot products recomputed a third time.
//   hardneg_grad_kernel    grad_neg_i = p_i a_i / (temp B), grad_anchor_i = p_i (n_i - 2 a_i) / (temp B).
//
// Every reduction runs in an order fixed by the problem size alone: each thread owns a fixed set of columns, wave
// sums are xor butterflies, wave partials are added in wave order; no floating-point atomics, and no kernel waits
// on another workgroup (what one pass needs from another is a separate launch).  Dot products are f32 products
// (exact in f64) accumulated in f64; exp / log and all sums are f64.
#include "vge_common.h"

#include <string>

#include "../../include/vge.h"
#include "vge_error.h"

namespace {

// ---------------------------------------------------------------------------------------------- time gather
// grid (B * T), 256 threads: one destination row of D4 = D / 4 float4 per workgroup.  T is 32 (checked on the
// host): the source index is masked to [0, 32), so a table that breaks the caller's contract still reads inside
// its own window.
__global__ void __launch_bounds__(256) time_gather_kernel(const float4* __restrict__ feats,
                                                          const int* __restrict__ src, int D4,
                                                          float4* __restrict__ out) {
  const size_t row = blockIdx.x;                       // b * 32 + t
  const int s = src[row] & (VGE_T - 1);
  const float4* in = feats + ((row & ~(size_t)(VGE_T - 1)) + s) * D4;
  float4* o = out + row * D4;
  for (int i = threadIdx.x; i < D4; i += 256) o[i] = in[i];
}

// ---------------------------------------------------------------------------------------------- TCL
constexpr int TCL_R = 8;      // rows of the Gram matrix per workgroup
constexpr int TCL_TH = 256;   // threads; thread t owns columns t, t + 256, ...
constexpr int TCL_DMAX = 256;

// rows [r0, r0 + TCL_R) of emb as doubles in LDS (rows past B as zeros)
__device__ __forceinline__ void tcl_load_rows(const float* __restrict__ emb, int B, int d, int r0,
                                              double (&zr)[TCL_R][TCL_DMAX]) {
  for (int e = threadIdx.x; e < TCL_R * d; e += TCL_TH) {
    const int r = e / d, c = e - r * d;
    zr[r][c] = (r0 + r < B) ? (double)emb[(size_t)(r0 + r) * d + c] : 0.0;
  }
}

// dot[r] = <z_{r0+r}, z_k> for the TCL_R rows in LDS (broadcast reads), z_k streamed from global in float4
__device__ __forceinline__ void tcl_dots(const float* __restrict__ zk, int d, const double (&zr)[TCL_R][TCL_DMAX],
                                         double (&dot)[TCL_R]) {
#pragma unroll
  for (int r = 0; r < TCL_R; ++r) dot[r] = 0.0;
  for (int c = 0; c < d; c += 4) {
    const float4 v = *reinterpret_cast<const float4*>(zk + c);
    const double x0 = v.x, x1 = v.y, x2 = v.z, x3 = v.w;
#pragma unroll
    for (int r = 0; r < TCL_R; ++r) {
      double a = dot[r];
      a = fma(zr[r][c], x0, a);
      a = fma(zr[r][c + 1], x1, a);
      a = fma(zr[r][c + 2], x2, a);
      a = fma(zr[r][c + 3], x3, a);
      dot[r] = a;
    }
  }
}

// sum of acc[r] over the workgroup's 256 threads: xor butterfly per wave, then the 4 waves in wave order.
// The result for row r is returned to thread r (r < TCL_R).
__device__ __forceinline__ double tcl_block_sum(double (&acc)[TCL_R], double (&red)[TCL_TH / 64][TCL_R]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < TCL_R; ++r) {
    const double s = wave_sum_d(acc[r]);
    if (lane == 0) red[w][r] = s;
  }
  __syncthreads();
  double out = 0.0;
  if (threadIdx.x < TCL_R) {
    const int r = threadIdx.x;
    out = ((red[0][r] + red[1][r]) + red[2][r]) + red[3][r];
  }
  return out;
}

// grid ceil(B / TCL_R).  den [B].
__global__ void __launch_bounds__(TCL_TH) tcl_den_kernel(const float* __restrict__ emb, const int* __restrict__ lab,
                                                        int B, int d, double temp, double k1, double k2,
                                                        double* __restrict__ den) {
  __shared__ double zr[TCL_R][TCL_DMAX];
  __shared__ double red[TCL_TH / 64][TCL_R];
  __shared__ int lr[TCL_R];
  const int r0 = blockIdx.x * TCL_R;
  tcl_load_rows(emb, B, d, r0, zr);
  if (threadIdx.x < TCL_R) lr[threadIdx.x] = (r0 + threadIdx.x < B) ? lab[r0 + threadIdx.x] : 0;
  __syncthreads();
  double acc[TCL_R];
#pragma unroll
  for (int r = 0; r < TCL_R; ++r) acc[r] = 0.0;
  for (int k = threadIdx.x; k < B; k += TCL_TH) {
    double dot[TCL_R];
    tcl_dots(emb + (size_t)k * d, d, zr, dot);
    const int lk = lab[k];
#pragma unroll
    for (int r = 0; r < TCL_R; ++r) {
      const double e = exp(dot[r] / temp);
      if (lr[r] != lk) acc[r] += k2 * e;                       // mask_negatives
      else if (r0 + r != k) acc[r] += e + k1 * exp(-dot[r]);   // mask_positives (same class, anchor out)
    }
  }
  const double s = tcl_block_sum(acc, red);
  if (threadIdx.x < TCL_R && r0 + threadIdx.x < B) den[r0 + threadIdx.x] = s;
}

// grid ceil(B / TCL_R).  rowloss [B] = sum_{j in P(i)} -log(e_ij / den_j) / |P(i)|.
__global__ void __launch_bounds__(TCL_TH) tcl_row_kernel(const float* __restrict__ emb, const int* __restrict__ lab,
                                                        int B, int d, double temp,
                                                        const double* __restrict__ den,
                                                        double* __restrict__ rowloss) {
  __shared__ double zr[TCL_R][TCL_DMAX];
  __shared__ double red[TCL_TH / 64][TCL_R];
  __shared__ int lr[TCL_R];
  const int r0 = blockIdx.x * TCL_R;
  tcl_load_rows(emb, B, d, r0, zr);
  if (threadIdx.x < TCL_R) lr[threadIdx.x] = (r0 + threadIdx.x < B) ? lab[r0 + threadIdx.x] : 0;
  __syncthreads();
  double acc[TCL_R], cnt[TCL_R];
#pragma unroll
  for (int r = 0; r < TCL_R; ++r) acc[r] = cnt[r] = 0.0;
  for (int j = threadIdx.x; j < B; j += TCL_TH) {
    const int lj = lab[j];
    bool any = false;
#pragma unroll
    for (int r = 0; r < TCL_R; ++r) any |= (lr[r] == lj) && (r0 + r != j) && (r0 + r < B);
    if (!any) continue;   // no positive pair in this column
    double dot[TCL_R];
    tcl_dots(emb + (size_t)j * d, d, zr, dot);
    const double dj = den[j];
#pragma unroll
    for (int r = 0; r < TCL_R; ++r)
      if (lr[r] == lj && r0 + r != j && r0 + r < B) {
        acc[r] += -log(exp(dot[r] / temp) / dj);
        cnt[r] += 1.0;
      }
  }
  const double s = tcl_block_sum(acc, red);
  __syncthreads();  // red is reused
  const double n = tcl_block_sum(cnt, red);
  if (threadIdx.x < TCL_R && r0 + threadIdx.x < B) rowloss[r0 + threadIdx.x] = s / n;   // |P(i)| = 0: 0/0 = NaN
}

// one workgroup: out[0] = (sum_i x[i]) / n, thread t summing x[t], x[t + 256], ... in order
__global__ void __launch_bounds__(256) mean_kernel(const double* __restrict__ x, int n, double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += x[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (((red[0] + red[1]) + red[2]) + red[3]) / (double)n;
}

// ---------------------------------------------------------------------------------------------- TCL gradient
// grid ceil(B / 256).  cnt[j] = |P(j)|: the rows with j's label, without j.
__global__ void __launch_bounds__(256) tcl_count_kernel(const int* __restrict__ lab, int B, double* __restrict__ cnt) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= B) return;
  const int lj = lab[j];
  int n = 0;
  for (int k = 0; k < B; ++k) n += (lab[k] == lj);
  cnt[j] = (double)(n - 1);
}

// grid ceil(B / TCL_R).  grad_j = (1 / B) sum_k (W_jk + W_kj) z_k for the workgroup's TCL_R rows j, with
//   k in P(j): W_jk = (e_jk / temp - k1 exp(-s_jk)) / den_j - 1 / (temp |P(j)|)
//   k in N(j): W_jk = k2 e_jk / (temp den_j),          W_jj = 0
// (the derivative of mean_j [log den_j - (1 / (temp |P(j)|)) sum_{k in P(j)} s_jk], which is the loss whenever every
// |P| >= 1).  The columns k go by in chunks of TCL_TH: thread t forms the TCL_R coefficients of column k0 + t from
// the recomputed dot products and leaves them in LDS; then thread (g, c) = (t / d, t % d), g < G = TCL_TH / d, adds
// coef[r][kk] * z[k0 + kk][c] for kk = g, g + G, ... in that order.  After the last chunk the G partials of a
// column are added in g order.  Nothing but (B, d) enters the order of any sum.
__global__ void __launch_bounds__(TCL_TH) tcl_grad_kernel(const float* __restrict__ emb, const int* __restrict__ lab,
                                                         int B, int d, double temp, double k1, double k2,
                                                         const double* __restrict__ den,
                                                         const double* __restrict__ cnt, float* __restrict__ grad) {
  __shared__ double zr[TCL_R][TCL_DMAX];
  __shared__ double coef[TCL_R][TCL_TH];   // after the last chunk: the partial sums, [TCL_R][g * d + c]
  __shared__ double dr[TCL_R], pr[TCL_R];  // 1 / den_j and 1 / (temp |P(j)|) of the workgroup's rows
  __shared__ int lr[TCL_R];
  const int r0 = blockIdx.x * TCL_R;
  tcl_load_rows(emb, B, d, r0, zr);
  if (threadIdx.x < TCL_R) {
    const int j = r0 + threadIdx.x;
    lr[threadIdx.x] = (j < B) ? lab[j] : 0;
    dr[threadIdx.x] = (j < B) ? 1.0 / den[j] : 0.0;
    pr[threadIdx.x] = (j < B) ? 1.0 / (temp * cnt[j]) : 0.0;
  }
  __syncthreads();
  const int G = TCL_TH / d, g = threadIdx.x / d, c = threadIdx.x - g * d;
  double acc[TCL_R];
#pragma unroll
  for (int r = 0; r < TCL_R; ++r) acc[r] = 0.0;
  for (int k0 = 0; k0 < B; k0 += TCL_TH) {
    const int k = k0 + threadIdx.x;
    if (k < B) {
      double dot[TCL_R];
      tcl_dots(emb + (size_t)k * d, d, zr, dot);
      const int lk = lab[k];
      const double dk = 1.0 / den[k], pk = 1.0 / (temp * cnt[k]);
#pragma unroll
      for (int r = 0; r < TCL_R; ++r) {
        const double e = exp(dot[r] / temp) / temp;
        double w;
        if (r0 + r >= B || r0 + r == k) w = 0.0;
        else if (lr[r] != lk) w = k2 * e * dr[r] + k2 * e * dk;
        else {
          const double num = e - k1 * exp(-dot[r]);
          w = (num * dr[r] - pr[r]) + (num * dk - pk);
        }
        coef[r][threadIdx.x] = w;
      }
    }
    __syncthreads();
    if (g < G) {
      const int nk = min(TCL_TH, B - k0);
      for (int kk = g; kk < nk; kk += G) {
        const double z = (double)emb[(size_t)(k0 + kk) * d + c];
#pragma unroll
        for (int r = 0; r < TCL_R; ++r) acc[r] = fma(coef[r][kk], z, acc[r]);
      }
    }
    __syncthreads();
  }
  if (g < G) {
#pragma unroll
    for (int r = 0; r < TCL_R; ++r) coef[r][threadIdx.x] = acc[r];
  }
  __syncthreads();
  if (g == 0) {
#pragma unroll
    for (int r = 0; r < TCL_R; ++r) {
      if (r0 + r >= B) break;
      double s = coef[r][c];
      for (int q = 1; q < G; ++q) s += coef[r][q * d + c];
      grad[(size_t)(r0 + r) * d + c] = (float)(s / (double)B);
    }
  }
}

// ---------------------------------------------------------------------------------------------- hard negatives
// one workgroup of 16 waves (the order of the sum is then a function of B alone, without a second launch).  Wave w
// takes the row groups w, w + 16, ...: HN_R consecutive rows per group, loaded together (one float4 per lane covers a
// row of 256), their 2 HN_R dot products reduced as independent butterflies; lane r then forms row r's term, so the
// f64 exp / log run once per group.  At the end the HN_WAVES x HN_R lane partials are added in order.
constexpr int HN_WAVES = 16, HN_R = 4;
__global__ void __launch_bounds__(HN_WAVES * 64) hardneg_kernel(const float* __restrict__ a,
                                                                const float* __restrict__ ng, int B, int d,
                                                                double temp, double* __restrict__ loss) {
  __shared__ double red[HN_WAVES][HN_R];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double s = 0.0;   // lanes 0 .. HN_R-1: the sum of the terms of rows i0 + lane
  for (int i0 = w * HN_R; i0 < B; i0 += HN_WAVES * HN_R) {
    double ap[HN_R], ah[HN_R];
#pragma unroll
    for (int r = 0; r < HN_R; ++r) ap[r] = ah[r] = 0.0;
    for (int c = lane * 4; c < d; c += 256) {
      float4 x[HN_R], y[HN_R];
#pragma unroll
      for (int r = 0; r < HN_R; ++r) {
        const bool ok = i0 + r < B;
        const size_t o = (size_t)(ok ? i0 + r : i0) * d + c;
        x[r] = *reinterpret_cast<const float4*>(a + o);
        y[r] = *reinterpret_cast<const float4*>(ng + o);
      }
#pragma unroll
      for (int r = 0; r < HN_R; ++r) {
        ap[r] = fma((double)x[r].x, (double)x[r].x, ap[r]);
        ap[r] = fma((double)x[r].y, (double)x[r].y, ap[r]);
        ap[r] = fma((double)x[r].z, (double)x[r].z, ap[r]);
        ap[r] = fma((double)x[r].w, (double)x[r].w, ap[r]);
        ah[r] = fma((double)x[r].x, (double)y[r].x, ah[r]);
        ah[r] = fma((double)x[r].y, (double)y[r].y, ah[r]);
        ah[r] = fma((double)x[r].z, (double)y[r].z, ah[r]);
        ah[r] = fma((double)x[r].w, (double)y[r].w, ah[r]);
      }
    }
    double p = 0.0, h = 0.0;
#pragma unroll
    for (int r = 0; r < HN_R; ++r) {
      const double sp = wave_sum_d(ap[r]), sh = wave_sum_d(ah[r]);
      if (lane == r) {
        p = sp;
        h = sh;
      }
    }
    p /= temp;
    h /= temp;
    const double m = fmax(p, h);
    const double term = (m + log(exp(p - m) + exp(h - m))) - p;   // CrossEntropyLoss against class 0
    if (lane < HN_R && i0 + lane < B) s += term;
  }
  if (lane < HN_R) red[w][lane] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < HN_WAVES; ++k)
      for (int r = 0; r < HN_R; ++r) t += red[k][r];
    loss[0] = t / (double)B;
  }
}

// gradient of hardneg_kernel's loss: one wave per row, 4 rows per workgroup.  With p_i = sigmoid((<a_i,n_i> -
// <a_i,a_i>) / temp):  grad_neg_i = p_i a_i / (temp B),  grad_anchor_i = p_i (n_i - 2 a_i) / (temp B)  (anchor is
// also the positive, so both of its uses carry gradient).  Rows are independent: no sum crosses a wave.
__global__ void __launch_bounds__(256) hardneg_grad_kernel(const float* __restrict__ a, const float* __restrict__ ng,
                                                           int B, int d, double temp, float* __restrict__ ga,
                                                           float* __restrict__ gn) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= B) return;
  const float* ai = a + (size_t)i * d;
  const float* ni = ng + (size_t)i * d;
  double ap = 0.0, ah = 0.0;
  for (int c = lane * 4; c < d; c += 256) {
    const float4 x = *reinterpret_cast<const float4*>(ai + c);
    const float4 y = *reinterpret_cast<const float4*>(ni + c);
    ap = fma((double)x.x, (double)x.x, ap);
    ap = fma((double)x.y, (double)x.y, ap);
    ap = fma((double)x.z, (double)x.z, ap);
    ap = fma((double)x.w, (double)x.w, ap);
    ah = fma((double)x.x, (double)y.x, ah);
    ah = fma((double)x.y, (double)y.y, ah);
    ah = fma((double)x.z, (double)y.z, ah);
    ah = fma((double)x.w, (double)y.w, ah);
  }
  const double m = (wave_sum_d(ah) - wave_sum_d(ap)) / temp;
  const double em = exp(-fabs(m));                              // sigmoid without overflow on either side
  const double p = (m >= 0.0 ? 1.0 : em) / (1.0 + em);
  const double s = p / (temp * (double)B);
  for (int c = lane * 4; c < d; c += 256) {
    const float4 x = *reinterpret_cast<const float4*>(ai + c);
    const float4 y = *reinterpret_cast<const float4*>(ni + c);
    float4 u, v;
    u.x = (float)(s * ((double)y.x - 2.0 * (double)x.x));
    u.y = (float)(s * ((double)y.y - 2.0 * (double)x.y));
    u.z = (float)(s * ((double)y.z - 2.0 * (double)x.z));
    u.w = (float)(s * ((double)y.w - 2.0 * (double)x.w));
    v.x = (float)(s * (double)x.x);
    v.y = (float)(s * (double)x.y);
    v.z = (float)(s * (double)x.z);
    v.w = (float)(s * (double)x.w);
    *reinterpret_cast<float4*>(ga + (size_t)i * d + c) = u;
    *reinterpret_cast<float4*>(gn + (size_t)i * d + c) = v;
  }
}

// ---------------------------------------------------------------------------------------------- centroid distance
// one wave per row, 4 rows per workgroup; float32 like the reference (F.normalize eps 1e-12, torch.norm)
__global__ void __launch_bounds__(256) centroid_dist_kernel(const float* __restrict__ emb,
                                                            const int* __restrict__ lab,
                                                            const float* __restrict__ cent, int n, int C, int d,
                                                            float* __restrict__ dist) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int c = lab[i];
  if (c < 0 || c >= C) {
    if (lane == 0) dist[i] = nanf("");
    return;
  }
  float ss = 0.f;
  for (int j = lane; j < d; j += 64) {
    const float x = emb[(size_t)i * d + j];
    ss += x * x;
  }
  const float nz = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
  float dd = 0.f;
  for (int j = lane; j < d; j += 64) {
    const float x = emb[(size_t)i * d + j] / nz - cent[(size_t)c * d + j];
    dd += x * x;
  }
  dd = wave_sum(dd);
  if (lane == 0) dist[i] = sqrtf(dd);
}

int fail(int code, const std::string& msg) {
  vge::set_last_error(msg);
  return code;
}

#define HIPCHK(expr)                                                                                    \
  do {                                                                                                  \
    hipError_t _e = (expr);                                                                             \
    if (_e != hipSuccess) return fail(VGE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

hipStream_t S(vge_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int vge_time_gather(const float* feats, const int32_t* src, int B, int T, int D, float* out, vge_stream_t stream) {
  if (!feats || !src || !out || B < 0) return fail(VGE_ERR_ARG, "vge_time_gather: null argument or negative B");
  if (T != VGE_T) return fail(VGE_ERR_ARG, "vge_time_gather: T must be 32");
  if (D < 4 || D % 4 != 0) return fail(VGE_ERR_ARG, "vge_time_gather: D must be a positive multiple of 4");
  if (out == feats) return fail(VGE_ERR_ARG, "vge_time_gather: out must not alias feats");
  if (!aligned16(feats) || !aligned16(out)) return fail(VGE_ERR_ARG, "vge_time_gather: feats / out must be 16-byte aligned");
  if ((long long)B * T > 0x7fffffffLL) return fail(VGE_ERR_ARG, "vge_time_gather: B too large");
  if (B == 0) return VGE_OK;
  hipLaunchKernelGGL(time_gather_kernel, dim3((unsigned)(B * T)), dim3(256), 0, S(stream),
                     reinterpret_cast<const float4*>(feats), src, D / 4, reinterpret_cast<float4*>(out));
  HIPCHK(hipGetLastError());
  return VGE_OK;
}

size_t vge_tcl_workspace_bytes(int B) { return B > 0 ? (size_t)B * 2 * sizeof(double) : 0; }

int vge_tcl_loss(const float* emb, const int32_t* labels, int B, int d, double temperature, double k1, double k2,
                 void* workspace, size_t workspace_bytes, double* loss, vge_stream_t stream) {
  if (!emb || !labels || !workspace || !loss) return fail(VGE_ERR_ARG, "vge_tcl_loss: null argument");
  if (B < 1 || B > 8192) return fail(VGE_ERR_ARG, "vge_tcl_loss: B must be in [1, 8192]");
  if (d < 32 || d > TCL_DMAX || d % 32 != 0) return fail(VGE_ERR_ARG, "vge_tcl_loss: d must be a multiple of 32 in [32, 256]");
  if (!(temperature > 0.0)) return fail(VGE_ERR_ARG, "vge_tcl_loss: temperature must be positive");
  if (workspace_bytes < vge_tcl_workspace_bytes(B)) return fail(VGE_ERR_ARG, "vge_tcl_loss: workspace smaller than vge_tcl_workspace_bytes(B)");
  if (!aligned16(emb) || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return fail(VGE_ERR_ARG, "vge_tcl_loss: emb must be 16-byte and workspace 8-byte aligned");
  double* den = static_cast<double*>(workspace);
  double* rowloss = den + B;
  const int nb = (B + TCL_R - 1) / TCL_R;
  const double temp = 1.0 / temperature;
  hipLaunchKernelGGL(tcl_den_kernel, dim3(nb), dim3(TCL_TH), 0, S(stream), emb, labels, B, d, temperature, k1, k2, den);
  hipLaunchKernelGGL(tcl_row_kernel, dim3(nb), dim3(TCL_TH), 0, S(stream), emb, labels, B, d, temperature, den, rowloss);
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, S(stream), rowloss, B, loss);
  HIPCHK(hipGetLastError());
  return VGE_OK;
}

int vge_hardneg_loss(const float* anchor, const float* neg, int B, int d, double temperature, double* loss,
                     vge_stream_t stream) {
  if (!anchor || !neg || !loss) return fail(VGE_ERR_ARG, "vge_hardneg_loss: null argument");
  if (B < 1 || d < 4 || d % 4 != 0) return fail(VGE_ERR_ARG, "vge_hardneg_loss: B must be positive and d a positive multiple of 4");
  if (!aligned16(anchor) || !aligned16(neg)) return fail(VGE_ERR_ARG, "vge_hardneg_loss: anchor / neg must be 16-byte aligned");
  if (!(temperature > 0.0)) return fail(VGE_ERR_ARG, "vge_hardneg_loss: temperature must be positive");
  hipLaunchKernelGGL(hardneg_kernel, dim3(1), dim3(HN_WAVES * 64), 0, S(stream), anchor, neg, B, d, temperature, loss);
  HIPCHK(hipGetLastError());
  return VGE_OK;
}

size_t vge_tcl_grad_workspace_bytes(int B) { return B > 0 ? (size_t)B * 3 * sizeof(double) : 0; }

int vge_tcl_loss_grad(const float* emb, const int32_t* labels, int B, int d, double temperature, double k1, double k2,
                      void* workspace, size_t workspace_bytes, double* loss, float* grad, vge_stream_t stream) {
  if (!grad) return fail(VGE_ERR_ARG, "vge_tcl_loss_grad: null grad");
  if (grad == emb) return fail(VGE_ERR_ARG, "vge_tcl_loss_grad: grad must not alias emb");
  if (B > 0 && workspace_bytes < vge_tcl_grad_workspace_bytes(B))
    return fail(VGE_ERR_ARG, "vge_tcl_loss_grad: workspace smaller than vge_tcl_grad_workspace_bytes(B)");
  // the loss is the forward's own three launches (den and rowloss in the first 2 B doubles of the workspace)
  const int st = vge_tcl_loss(emb, labels, B, d, temperature, k1, k2, workspace, workspace_bytes, loss, stream);
  if (st != VGE_OK) return st;
  const double* den = static_cast<const double*>(workspace);
  double* cnt = static_cast<double*>(workspace) + 2 * (size_t)B;
  hipLaunchKernelGGL(tcl_count_kernel, dim3((B + 255) / 256), dim3(256), 0, S(stream), labels, B, cnt);
  hipLaunchKernelGGL(tcl_grad_kernel, dim3((B + TCL_R - 1) / TCL_R), dim3(TCL_TH), 0, S(stream), emb, labels, B, d,
                     temperature, k1, k2, den, cnt, grad);
  HIPCHK(hipGetLastError());
  return VGE_OK;
}

int vge_hardneg_loss_grad(const float* anchor, const float* neg, int B, int d, double temperature, double* loss,
                          float* grad_anchor, float* grad_neg, vge_stream_t stream) {
  if (!grad_anchor || !grad_neg) return fail(VGE_ERR_ARG, "vge_hardneg_loss_grad: null grad_anchor / grad_neg");
  if (!aligned16(grad_anchor) || !aligned16(grad_neg))
    return fail(VGE_ERR_ARG, "vge_hardneg_loss_grad: grad_anchor / grad_neg must be 16-byte aligned");
  if (grad_anchor == grad_neg || grad_anchor == anchor || grad_anchor == neg || grad_neg == anchor || grad_neg == neg)
    return fail(VGE_ERR_ARG, "vge_hardneg_loss_grad: grad_anchor / grad_neg must not alias each other or an input");
  const int st = vge_hardneg_loss(anchor, neg, B, d, temperature, loss, stream);   // the forward's own launch
  if (st != VGE_OK) return st;
  hipLaunchKernelGGL(hardneg_grad_kernel, dim3((B + 3) / 4), dim3(256), 0, S(stream), anchor, neg, B, d, temperature,
                     grad_anchor, grad_neg);
  HIPCHK(hipGetLastError());
  return VGE_OK;
}

int vge_centroid_distance(const float* emb, const int32_t* labels, const float* centroids, int n, int C, int d,
                          float* dist, vge_stream_t stream) {
  if (!emb || !labels || !centroids || !dist) return fail(VGE_ERR_ARG, "vge_centroid_distance: null argument");
  if (n < 0 || C < 1 || d < 1) return fail(VGE_ERR_ARG, "vge_centroid_distance: n, C or d out of range");
  if (n == 0) return VGE_OK;
  hipLaunchKernelGGL(centroid_dist_kernel, dim3((n + 3) / 4), dim3(256), 0, S(stream), emb, labels, centroids, n, C, d,
                     dist);
  HIPCHK(hipGetLastError());
  return VGE_OK;
}

}  // extern "C"
