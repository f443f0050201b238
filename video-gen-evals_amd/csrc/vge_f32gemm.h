// The training nodes' exact-f32 GEMM and the chunk-partial reduce, shared by vge_timelayer.hip (the temporal layer) and
// vge_linear.hip (the bias-free linear node, which the fusion node's GEMMs use as well).
//
//   tl_gemm_kernel     exact-f32 GEMM on v_mfma_f32_16x16x4_f32, one 64 x 64 output tile per workgroup, in three
//                      operand forms:
//                        <0,0,0>  C[m,n] = sum_k A[m,k] W[n,k]      forward GEMMs (x W^T)
//                        <0,1,0>  C[m,n] = sum_k A[m,k] W[k,n]      data gradients (dY W)
//                        <1,1,1>  P[c][m,n] = sum_{r in chunk c} A[r,m] B[r,n]   weight gradients (dY^T X), one f64
//                                 partial per chunk of rows
//                      with the epilogue  v = f32(sum) (+ bias[n]) (relu) (* mask[m,n]) (gate[m,n] <= 0 ? 0 : v)
//                      (res[m,n] + v).
//                      Two more flags, A_SC and B_SC, make an operand's loads scalar with every element checked against
//                      its own bounds: for an operand whose base, row stride or contiguous extent is no multiple of 4
//                      floats (a column slice at column 1033, K = 3, 9, 69, 207).  With B_SC the output's N is
//                      arbitrary too and each stored column is checked.  Both default to false, and an instantiation
//                      without them is the temporal layer's kernel, instruction for instruction.
//   tl_reduce_kernel   adds f64 chunk partials in chunk order and rounds to f32 once.
//
// Summation: one MFMA chain per 16 products (exact f32 products, f32 adds), the chains added in f64, the sum rounded to
// f32 once.  K beyond the operand is zero in LDS -- whole chains of zeros add +0 -- and is never stored; so are rows
// past M and columns past N of a tile.
#pragma once
#include "vge_common.h"
#include "vge_core.h"

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int TL_TILE = 64;        // output tile of the GEMM, both ways
constexpr int TL_KSTEP = 32;       // K per LDS fill: two chains of 16
constexpr int TL_LDT = 80;         // LDS row stride of a [k][64] operand tile: the 4 lane groups hit 4 x 16 banks
constexpr int TL_WG_CHUNKS = 8;    // row chunks of a weight gradient

// MC (A_MC / B_MC): the operand's M (N) index is the contiguous one (row = k); otherwise k is contiguous (row = m or n).
// grid (ceil(M / 64), ceil(N / 64), chunks); chunks > 1 only with PARTIAL.  M is arbitrary.  Without SC, N and the
// contiguous extents are multiples of 4 and every row starts 16-byte aligned; K is arbitrary where k is not the
// contiguous index, a multiple of 4 where it is.
template <bool MC, bool SC>
__device__ __forceinline__ void tl_fill(float* T, const float* __restrict__ G, int ld, int mn0, int MN, int k0, int kend,
                                        int tid) {
  if (MC) {  // row k: 16 float4 along mn
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int k = (tid >> 4) + 16 * p, mn = (tid & 15) * 4;
      floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
      if (SC) {
        if (k0 + k < kend) {
          const float* __restrict__ row = G + (size_t)(k0 + k) * ld + mn0 + mn;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (mn0 + mn + q < MN) v[q] = row[q];
        }
      } else if (k0 + k < kend && mn0 + mn < MN) {
        v = *reinterpret_cast<const floatx4*>(G + (size_t)(k0 + k) * ld + mn0 + mn);
      }
      *reinterpret_cast<floatx4*>(T + k * TL_LDT + mn) = v;
    }
  } else {  // row mn: 8 float4 along k
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int mn = (tid >> 3) + 32 * p, k = (tid & 7) * 4;
      floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
      if (SC) {
        if (mn0 + mn < MN) {
          const float* __restrict__ row = G + (size_t)(mn0 + mn) * ld + k0 + k;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (k0 + k + q < kend) v[q] = row[q];
        }
      } else if (mn0 + mn < MN && k0 + k < kend) {
        v = *reinterpret_cast<const floatx4*>(G + (size_t)(mn0 + mn) * ld + k0 + k);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) T[(k + q) * TL_LDT + mn] = v[q];
    }
  }
}

template <bool A_MC, bool B_MC, bool PARTIAL, bool A_SC = false, bool B_SC = false>
__global__ void __launch_bounds__(256) tl_gemm_kernel(vge::TimeGemmArgs G) {
  __shared__ __attribute__((aligned(16))) float As[TL_KSTEP * TL_LDT];
  __shared__ __attribute__((aligned(16))) float Bs[TL_KSTEP * TL_LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * TL_TILE, n0 = blockIdx.y * TL_TILE;
  int k0 = 0, kend = G.K;
  if (PARTIAL) {
    k0 = blockIdx.z * G.k_per_chunk;
    kend = min(G.K, k0 + G.k_per_chunk);
  }
  doublex4 acc[4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) acc[rt] = doublex4{0.0, 0.0, 0.0, 0.0};
  const floatx4 zero = floatx4{0.f, 0.f, 0.f, 0.f};
  const bool col_live = n0 + wave * 16 < G.N;  // this wave's 16 columns exist (all of them, without B_SC)

  for (int kb = k0; kb < kend; kb += TL_KSTEP) {
    __syncthreads();  // the previous step's reads
    tl_fill<A_MC, A_SC>(As, G.A, G.lda, m0, G.M, kb, kend, tid);
    tl_fill<B_MC, B_SC>(Bs, G.B, G.ldb, n0, G.N, kb, kend, tid);
    __syncthreads();
    if (col_live) {
#pragma unroll
      for (int ch = 0; ch < TL_KSTEP / 16; ++ch) {
        floatx4 part[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = ch * 16 + q * 4 + g;
          const float b = Bs[k * TL_LDT + wave * 16 + il];
#pragma unroll
          for (int rt = 0; rt < 4; ++rt) part[rt] = mfma16x16x4(As[k * TL_LDT + rt * 16 + il], b, q == 0 ? zero : part[rt]);
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] += __builtin_convertvector(part[rt], doublex4);
      }
    }
  }
  if (!col_live) return;
  const int n = n0 + wave * 16 + il;
  if (B_SC && n >= G.N) return;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + rt * 16 + 4 * g + r;
      if (m >= G.M) continue;
      if (PARTIAL) {
        G.part[((size_t)blockIdx.z * G.M + m) * G.N + n] = acc[rt][r];
        continue;
      }
      const size_t o = (size_t)m * G.ldc + n;
      float v = (float)acc[rt][r];
      if (G.bias) v += G.bias[n];
      if (G.relu) v = v < 0.f ? 0.f : v;  // a NaN stays a NaN
      if (G.mask) v *= G.mask[o];
      if (G.gate) v = G.gate[o] <= 0.f ? 0.f : v;  // a NaN gate lets v through, as torch's relu backward does
      if (G.res) v = G.res[o] + v;
      G.C[o] = v;
    }
}

// out[e] = f32(sum over chunks, in chunk order, of part[chunk][e])
__global__ void __launch_bounds__(256) tl_reduce_kernel(const double* __restrict__ part, int n_chunks, int n,
                                                        float* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int ch = 0; ch < n_chunks; ++ch) s += part[(size_t)ch * n + e];
  out[e] = (float)s;
}

// rows per chunk of a weight gradient over R rows (whole chains of 16), and the number of chunks
inline int tl_wgrad_chunks(int R, int* k_per_chunk) {
  int per = (R + TL_WG_CHUNKS - 1) / TL_WG_CHUNKS;
  per = (per + 15) & ~15;
  if (k_per_chunk) *k_per_chunk = per;
  return (R + per - 1) / per;
}

// One launch of the GEMM in `form` (vge_core.h TIME_GEMM_*); a_sc / b_sc: the operand needs scalar, bounds-checked loads.
inline hipError_t tl_launch_gemm(const vge::TimeGemmArgs& a, int form, bool a_sc, bool b_sc, hipStream_t s) {
  vge::TimeGemmArgs g = a;
  dim3 grid((a.M + TL_TILE - 1) / TL_TILE, (a.N + TL_TILE - 1) / TL_TILE, 1);
  if (form == vge::TIME_GEMM_TN) grid.z = tl_wgrad_chunks(a.K, &g.k_per_chunk);
#define TL_GEMM_CASE(F, AMC, BMC, P, ASC, BSC)                                                             \
  if (form == F && a_sc == ASC && b_sc == BSC) {                                                          \
    hipLaunchKernelGGL((tl_gemm_kernel<AMC, BMC, P, ASC, BSC>), grid, dim3(256), 0, s, g);                \
    return hipGetLastError();                                                                             \
  }
  TL_GEMM_CASE(vge::TIME_GEMM_NT, false, false, false, false, false)
  TL_GEMM_CASE(vge::TIME_GEMM_NN, false, true, false, false, false)
  TL_GEMM_CASE(vge::TIME_GEMM_TN, true, true, true, false, false)
#ifdef VGE_F32GEMM_SCALAR_FORMS
  TL_GEMM_CASE(vge::TIME_GEMM_NT, false, false, false, true, false)
  TL_GEMM_CASE(vge::TIME_GEMM_NT, false, false, false, true, true)
  TL_GEMM_CASE(vge::TIME_GEMM_NN, false, true, false, false, true)
  TL_GEMM_CASE(vge::TIME_GEMM_TN, true, true, true, false, true)
#endif
#undef TL_GEMM_CASE
  return hipErrorInvalidValue;
}

}  // namespace
