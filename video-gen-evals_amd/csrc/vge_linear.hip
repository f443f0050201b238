// A bias-free linear map for training on gfx950: the movement encoders' stems (1 x 1 convolutions, K = 3 ... 1024) and
// projections (vge_linear_forward / vge_linear_backward, formulas in include/vge.h), and the launchers the fusion node
// (vge_fusion.hip) runs its D x D GEMMs through.
//
// Everything runs on tl_gemm_kernel of vge_f32gemm.h, the temporal layer's GEMM: exact f32 products on
// v_mfma_f32_16x16x4_f32, one chain per 16 products, chains added in f64, rounded to f32 once; dW as f64 partials per
// chunk of rows, added by tl_reduce_kernel in chunk order.  No floating-point atomics.
//
// x is read in place with its row stride: a stem's input is a column slice of the feature tensor.  Where x's base, ldx
// and K are all multiples of 4 floats the loads are the temporal layer's float4 loads; otherwise the scalar-load
// instantiations run, which check every element against its own bounds, so a K tail is zero in LDS and is never read
// past, and never stored.
#define VGE_F32GEMM_SCALAR_FORMS
#include "vge_f32gemm.h"
#include "vge_node_args.h"

namespace {

using vge::TimeGemmArgs;

// whether x [R][K] with row stride ldx can be read with 16-byte loads
bool lin_x_vector(const float* x, int ldx, int K) {
  return (reinterpret_cast<uintptr_t>(x) & 15) == 0 && ldx % 4 == 0 && K % 4 == 0;
}

bool lin_shape_ok(long long R, long long K, long long N, long long ldx) {
  if (R < 1 || K < 1 || K > 4096 || N < 32 || N > 256 || N % 32 != 0 || ldx < K) return false;
  const long long widest = ldx > N ? ldx : N;  // ldx >= K
  return R * widest <= 0x7fffffffLL;
}

int lin_shape(const char* fn, int R, int K, int N, int ldx) {
  if (lin_shape_ok(R, K, N, ldx)) return VGE_OK;
  const bool arg = R >= 1 && K >= 1 && ldx < K;
  return fail(arg ? VGE_ERR_ARG : VGE_ERR_UNSUPPORTED,
              std::string(fn) + ": needs R >= 1, 1 <= K <= 4096, N a multiple of 32 in [32, 256], ldx >= K and "
              "R max(K, N, ldx) < 2^31; got R " + std::to_string(R) + ", K " + std::to_string(K) + ", N " +
              std::to_string(N) + ", ldx " + std::to_string(ldx));
}

}  // namespace

namespace vge {

int linear_wgrad_chunks(int R) { return tl_wgrad_chunks(R, nullptr); }

hipError_t launch_linear_forward(const float* x, int ldx, const float* W, float* y, int R, int K, int N, hipStream_t s) {
  TimeGemmArgs g{};
  g.A = x, g.lda = ldx, g.B = W, g.ldb = K, g.M = R, g.N = N, g.K = K, g.C = y, g.ldc = N;
  return tl_launch_gemm(g, TIME_GEMM_NT, !lin_x_vector(x, ldx, K), K % 4 != 0, s);
}

hipError_t launch_linear_dgrad(const float* dy, const float* W, float* dx, int R, int K, int N, hipStream_t s) {
  TimeGemmArgs g{};
  g.A = dy, g.lda = N, g.B = W, g.ldb = K, g.M = R, g.N = K, g.K = N, g.C = dx, g.ldc = K;
  return tl_launch_gemm(g, TIME_GEMM_NN, false, K % 16 != 0, s);  // K is the output's N here: whole 16-column groups
}

hipError_t launch_linear_wgrad(const float* dy, const float* x, int ldx, double* part, float* dW, int R, int K, int N,
                               hipStream_t s) {
  TimeGemmArgs g{};
  g.A = dy, g.lda = N, g.B = x, g.ldb = ldx, g.M = N, g.N = K, g.K = R, g.part = part;
  const hipError_t e = tl_launch_gemm(g, TIME_GEMM_TN, false, !lin_x_vector(x, ldx, K) || K % 16 != 0, s);
  if (e != hipSuccess) return e;
  return launch_timelayer_reduce(part, linear_wgrad_chunks(R), N * K, dW, s);
}

}  // namespace vge

extern "C" {

size_t vge_linear_workspace_bytes(int R, int K, int N) {
  if (!lin_shape_ok(R, K, N, K)) return 0;
  return (size_t)vge::linear_wgrad_chunks(R) * N * K * sizeof(double);
}

int vge_linear_forward(const float* x, int ldx, const float* W, float* y, int R, int K, int N, vge_stream_t stream) {
  const char* fn = "vge_linear_forward";
  if (int st = lin_shape(fn, R, K, N, ldx)) return st;
  const size_t xb = ((size_t)(R - 1) * ldx + K) * 4;
  const Span sp[] = {{x, xb, "x", false, true}, {W, (size_t)N * K * 4, "W", false}, {y, (size_t)R * N * 4, "y", false}};
  if (int st = tl_buffers(fn, sp, 2, 3)) return st;
  HIPCHK(vge::launch_linear_forward(x, ldx, W, y, R, K, N, tl_stream(stream)));
  return VGE_OK;
}

int vge_linear_backward(const float* dy, const float* x, int ldx, const float* W, float* dx, float* dW, void* workspace,
                        size_t workspace_bytes, int R, int K, int N, vge_stream_t stream) {
  const char* fn = "vge_linear_backward";
  if (int st = lin_shape(fn, R, K, N, ldx)) return st;
  const size_t xb = ((size_t)(R - 1) * ldx + K) * 4;
  const Span sp[] = {{dy, (size_t)R * N * 4, "dy", false},
                     {x, xb, "x", false, true},
                     {W, (size_t)N * K * 4, "W", false},
                     {dx, (size_t)R * K * 4, "dx", true},
                     {dW, (size_t)N * K * 4, "dW", false},
                     {workspace, workspace_bytes, "workspace", false}};
  if (int st = tl_buffers(fn, sp, 3, 6)) return st;
  if (workspace_bytes < vge_linear_workspace_bytes(R, K, N))
    return fail(VGE_ERR_WORKSPACE, std::string(fn) + ": workspace smaller than vge_linear_workspace_bytes");
  hipStream_t s = tl_stream(stream);
  if (dx) HIPCHK(vge::launch_linear_dgrad(dy, W, dx, R, K, N, s));
  HIPCHK(vge::launch_linear_wgrad(dy, x, ldx, static_cast<double*>(workspace), dW, R, K, N, s));
  return VGE_OK;
}

}  // extern "C"
