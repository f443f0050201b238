// The scoring core's interface between the C ABI (vge_api.cpp) and its kernels: every kernel-argument struct, defined
// once for host and device, and every launcher of vge_featurize.hip, vge_encoder.hip, vge_encoder_x3.hip,
// vge_encoder_x3s.hip, vge_encoder_gen.hip, vge_transformer_x3.hip, vge_convblock.hip, vge_timelayer.hip,
// vge_linear.hip, vge_fusion.hip and vge_score.hip.  Host-safe: no device helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace vge {

// GEMM epilogues of gemm_kernel (vge_encoder.hip) and gemm_x3_kernel (vge_encoder_x3.hip): +PE/CLS token assembly,
// +bias, +bias+ReLU, +bias+residual+LayerNorm
enum Epi { EPI_TOKENS = 0, EPI_BIAS = 1, EPI_BIAS_RELU = 2, EPI_BIAS_RES_LN = 3 };

// ------------------------------------------------------------------ vge_featurize.hip
// tiles: TileDesc[n_tiles] (8 x int32 each) or null with `windows` given
hipError_t launch_featurize_tiles(const float* pose, const float* gori, const float* betas, const float* vit,
                                  const float* kp, const int* videos, const void* tiles, const int* windows,
                                  int n_tiles, const float* mean, const float* stdv, float* feats, int with_kp,
                                  hipStream_t s);
hipError_t launch_stats_colsum(const float* feats, const void* tiles, int n_tiles, int tiles_per_chunk, int n_chunks,
                               double* partial, double* sums, hipStream_t s);
hipError_t launch_stats_finalize(const double* sums, long long n_mesh, long long n_kp, float* mean, float* stdv,
                                 int with_kp, hipStream_t s);

// ------------------------------------------------------------------ vge_encoder.hip (exact f32 MFMA)
struct EncDesc {
  const float* stem;   // n_stem_panels * 16 chunks
  const float* conv;   // 4 blocks x 2 convs x 5 taps x 16 chunks
  const float* proj;   // 16 chunks
  const float* gn_w;   // [4][256]
  const float* gn_b;   // [4][256]
  int in_col;          // column offset of this encoder's input in feats
  int d_in;
  int n_stem_panels;
  int ld;              // feats row width (2596, or 2356 keypoint-less)
};

struct FuseParams {
  const float* kv_w;     // [256]
  const float* kv_b;     // [256]
  const float* u;        // [256] = Wk^T (Wq LN(latent))   (folded constant query)
  float inv_tau[8];      // 1 / (softplus(logit_temp) + 1e-3)
  float bias[8];         // logit_bias
  int n_mod;
  int has_motion[8];
};

struct GemmArgs {
  const float* A;  int lda;     // rows padded to a multiple of 32 (pad rows are finite)
  const float* W;               // packed chunks [N/256][K/256][16][4096]
  float* out;      int ldo;
  int M, K, N;
  const float* bias;            // [N]
  const float* res;  int ldr;   // residual (EPI_BIAS_RES_LN)
  const float* ln_w; const float* ln_b;
  const float* pe;              // EPI_TOKENS: pos_enc.pe [5000,256]
  const float* cls;             // EPI_TOKENS: cls [256]
};

hipError_t encoder_kernel_setup();
hipError_t launch_conv_encoders(const float* feats, int n_windows, const EncDesc* encs, int n_enc, float* enc_out,
                                hipStream_t s);
hipError_t launch_fuse(const float* enc_out, int n_rows, const FuseParams& fp, float* pooled, hipStream_t s);
hipError_t launch_gemm(int epi, const GemmArgs& a, hipStream_t s);
hipError_t launch_attn(const float* qkv, int n_windows, float* out, hipStream_t s);
hipError_t launch_embed_tc(const float* x, int n_windows, float* seq, float* frame, float* tc, hipStream_t s);

// ------------------------------------------------------------------ vge_encoder_x3.hip / vge_encoder_x3s.hip (3xfp16)
// One MovementConvEncoder's weights (model.py:21-58) as the x3 conv kernels read them.
struct EncDescX3 {
  const _Float16* stem;  // stem chunks; panel p (256 K) starts at chunk 16p, padded to STREAM_GROUP chunks
  const _Float16* conv;  // 8 convs x 5 taps x 16 chunks
  const _Float16* proj;  // 16 chunks
  const float* gn_w;     // [4][256]
  const float* gn_b;     // [4][256]
  const float* cs;       // [10][256] weight column scales: stem, conv 0..7, proj
  // staggered split kernel only (vge_encoder_x3s.hip), else null: the GroupNorm-folded corrections of blocks 1..3's
  // conv1, [3 blocks][256 cols][16] = per-tap sums over input channels of W1 gamma (taps 0..4), then of W1 beta (at 8..12),
  // then the proj's [256][2] (sums of P gamma, P beta)
  const float* fold;
  int in_col, d_in, n_stem_panels, ld;  // ld: feats row width (2596, or 2356 keypoint-less)
  float gn_gmax[4], gn_bmax[4];  // max |gamma|, max |beta| of each GroupNorm (split-exponent bounds)
};

struct GemmArgsX3 {
  const float* A;  int lda;
  const _Float16* W;            // chunks [N/256][K/16][16 KB]
  float* out;      int ldo;
  int M, K, N;
  const float* bias;
  const float* res;  int ldr;
  const float* ln_w; const float* ln_b;
  const float* pe;
  const float* cls;
  const float* cs;              // [N] weight column scales
};

struct FfnArgsX3 {
  const float* X1;  // [M (padded to 64)][256] input, also the residual
  float* out;       // [M][256]
  int M;
  const _Float16* W1; const float* cs1; const float* b1;  // linear1 [1024][256]: 4 column blocks x 16 chunks
  const _Float16* W2; const float* cs2; const float* b2;  // linear2 [256][1024]: 64 chunks (4 K panels)
  const float* ln_w; const float* ln_b;
};

// Persistent schedule of the quad / pair conv kernels.  Work units: Q quads (4 windows) then the pairs (2 windows)
// covering the rest of each encoder's windows; encoder e takes q_e quads (windows [0, 4 q_e)) and the pairs after
// them.  Grid = G blocks (one per CU); unit u runs on block u % G in round u / G, so with Q a multiple of G every CU
// does the same number of quads and at most one pair.  Within a round the block index is remapped so the 8 XCDs
// (blocks dealt round robin) take contiguous runs of G / 8 units, i.e. the same encoders' weights in their L2.
// q_e: whole XCD runs where that tiles Q (conv_quad_sched: then every XCD streams ONE encoder per round, and the
// encoders with multi-panel stems -- `heavy`, a bit mask -- take the pairs), else nearly equal.  qpre / ppre: prefix
// sums of the quads / pairs per encoder.
constexpr int CONV_MAX_ENC = 16;
struct ConvSched {
  int n_windows, n_enc, G, Q, n_units;
  int qpre[CONV_MAX_ENC + 1], ppre[CONV_MAX_ENC + 1];
};
int conv_cu_count();  // CUs of the current device (256 where the query fails), read once
ConvSched conv_quad_sched(int n_windows, int n_enc, unsigned heavy = 0);
// the unit table of conv_encoder_f16w_kernel (units of up to wmax windows), and its plan without the table
bool conv_f16w_schedule(int n_windows, int n_enc, int wmax, std::vector<int>& table, int& G, int& R);
bool conv_f16w_plan(int n_windows, int n_enc, int wmax, int& G, int& R, int& U);

hipError_t encoder_x3_kernel_setup();
hipError_t launch_pack_x3(const float* W, int N, int K_real, int ldk, int conv, int nch, int* sh, float* cs, int* bad,
                          _Float16* out, hipStream_t s);
hipError_t launch_conv_encoders_x3(const float* feats, int n_windows, const EncDescX3* encs, int n_enc, unsigned heavy,
                                   float* enc_out, bool split, bool stem_split, hipStream_t s);
hipError_t launch_conv_f16w_table(int n_windows, int n_enc, int G, int R, int U, int* d_table, hipStream_t s);
hipError_t launch_conv_encoders_f16w(const float* feats, int n_windows, const EncDescX3* encs, float* enc_out,
                                     const int* d_units, int G, int R, hipStream_t s);
hipError_t launch_gemm_x3(int epi, const GemmArgsX3& a, hipStream_t s);
hipError_t launch_ffn_x3(const FfnArgsX3& a, hipStream_t s);

hipError_t encoder_x3s_kernel_setup();
hipError_t launch_conv_encoders_x3s(const float* feats, int n_windows, const EncDescX3* encs, int n_enc, unsigned heavy,
                                    float* enc_out, int* status, bool split, hipStream_t s);

// ------------------------------------------------------------------ vge_transformer_x3.hip (fused transformer)
constexpr int TX_MAX_LAYERS = 8;

struct TxLayerX3 {
  const _Float16* in_w;  const float* in_cs; const float* in_b;     // in_proj [768][256]: 3 col blocks x 16
  const _Float16* out_w; const float* out_cs; const float* out_b;   // out_proj [256][256]: 16 chunks
  const float* n1_w; const float* n1_b;
  const _Float16* l1_w; const float* l1_cs; const float* l1_b;      // linear1 [1024][256]: 4 col blocks x 16
  const _Float16* l2_w; const float* l2_cs; const float* l2_b;      // linear2 [256][1024]: 4 K panels x 16
  const float* n2_w; const float* n2_b;
  int e_x1, e_x2, e_h, pad;  // static split exponents: LN1 / LN2 outputs, FFN hidden (host: range bounds)
};

struct TxArgsX3 {  // by value: the layer table is kernel-argument memory (scalar loads, no vmcnt waits)
  const float* pooled;  // [B*32][256] fused per-frame vectors (fuse_kernel)
  int n_windows, n_layers;
  const _Float16* ov_w; const float* ov_cs;  // Wov = Wo Wv of the fusion (16 chunks)
  const float* cls; const float* pe;         // [256], [33][256]
  float* seq; float* frame; float* tc;       // [B][256], [B][33][256] | null, [B] | null
  TxLayerX3 layers[TX_MAX_LAYERS];           // entries past n_layers: zero
};

hipError_t transformer_x3_kernel_setup();
// mode: 0 single fp16, 1 activations split (fp16 weights), 2 3xfp16
hipError_t launch_transformer_x3(const TxArgsX3& a, int mode, hipStream_t s);

// ------------------------------------------------------------------ vge_encoder_gen.hip (generic-shape exact f32)
struct GenFuse {
  const float* kv_w; const float* kv_b; const float* u;  // [d] each (u = Wk^T Wq q_ln(latent))
  float inv_tau[8], bias[8];
  int n_mod, d;
  int has_motion[8];
};

hipError_t launch_gen_conv(const float* x, int ldx, int xcol, int cin, const float* W, int cout, int taps, int dil, int epi,
                           const float* res, float* out, int n_windows, hipStream_t s);
hipError_t launch_gen_groupnorm(float* x, int n_windows, int d, const float* g, const float* b, hipStream_t s);
hipError_t launch_gen_fuse(const float* enc_out, int n_rows, const GenFuse& f, float* pooled_pre, hipStream_t s);
hipError_t launch_gen_gemm(const float* A, int lda, const float* W, int M, int N, int K, const float* bias, int epi,
                           const float* res, const float* pe, const float* cls, float* out, int ldo, hipStream_t s);
hipError_t launch_gen_attn(const float* qkv, int n_windows, int d, int heads, float* out, hipStream_t s);
hipError_t launch_gen_add_ln(const float* a, const float* b, int rows, int d, const float* g, const float* be, float* out,
                             hipStream_t s);
hipError_t launch_gen_embed_tc(const float* x, int n_windows, int d, float* seq, float* frame, float* tc, hipStream_t s);

// ------------------------------------------------------------------ vge_convblock.hip (training: one conv block)
// x, m (null: all ones), a, u, y and the gradients: [B][T][C]; P1 / P2: weight images of launch_convblock_pack
struct ConvBlockFwdArgs {
  const float* x; const float* m; const float* P1; const float* P2; const float* gamma; const float* beta;
  float* a; float* u; float* mu; float* rstd;  // the saved set: all four or all null
  float* y;
  int B, T, C, dil;
};

struct ConvBlockBwdArgs {
  const float* x; const float* m; const float* a; const float* u; const float* mu; const float* rstd;
  const float* gamma; const float* dy;
  const float* P1b; const float* P2b;  // flipped images of W1, W2
  float* du; float* da; float* h;      // [B][T][C] scratch the weight gradient reads
  float* dx;
  double* gb_part;                     // [B][2][C] per-sample sums of dy g^ (dgamma) and dy (dbeta)
  int B, T, C, dil;
};

struct ConvBlockWgradArgs {
  const float* x; const float* h; const float* da; const float* du;
  float* part;                         // [chunks][2][5][C][C]
  int B, T, C, dil, per_chunk;         // per_chunk: set by the launcher
};

int convblock_chunks(int B, int* per_chunk);  // sample chunks of the weight gradient, and samples per chunk
hipError_t launch_convblock_pack(const float* W, int C, int flip, float* P, hipStream_t s);
hipError_t launch_convblock_forward(const ConvBlockFwdArgs& a, hipStream_t s);
hipError_t launch_convblock_backward(const ConvBlockBwdArgs& a, hipStream_t s);
hipError_t launch_convblock_wgrad(const ConvBlockWgradArgs& a, float* dw1, float* dw2, hipStream_t s);
hipError_t launch_convblock_gbreduce(const double* gb_part, int B, int C, float* dgamma, float* dbeta, hipStream_t s);

// ------------------------------------------------------------------ vge_timelayer.hip (training: one temporal layer)
// Exact-f32 GEMM C [M][N] (row stride ldc) from A and B in one of three operand forms; epilogue in this order, each
// step only where its pointer / flag is set: + bias[n], relu, * mask[m][n], gate[m][n] <= 0 ? 0 : v, res[m][n] + v
// (mask, gate and res have C's layout).  TIME_GEMM_TN writes f64 partials part[chunk][M][N] over chunks of K instead.
enum { TIME_GEMM_NT = 0,   // C[m][n] = sum_k A[m][k] B[n][k]
       TIME_GEMM_NN = 1,   // C[m][n] = sum_k A[m][k] B[k][n]
       TIME_GEMM_TN = 2 }; // part[c][m][n] = sum_{k in chunk c} A[k][m] B[k][n]
struct TimeGemmArgs {
  const float* A; int lda; const float* B; int ldb;
  int M, N, K;
  const float* bias; const float* mask; const float* gate; const float* res; int relu;
  float* C; int ldc;
  double* part; int k_per_chunk;       // TIME_GEMM_TN; k_per_chunk: set by the launcher
};

// qkv [B S][3 D], m (null: all ones) [B][H][S][S], d_o / o [B S][D], dqkv [B S][3 D]
struct TimeAttnArgs {
  const float* qkv; const float* m; const float* d_o;
  float* o; float* dqkv;
  int B, S, D, H;
};

int timelayer_wgrad_chunks(int R, int* k_per_chunk);  // row chunks of a weight gradient over R rows, rows per chunk
int timelayer_ln_chunks(int R);                       // workgroups (partials) of the LayerNorm backward
int timelayer_colsum_chunks(int R);                   // row chunks of a bias gradient
hipError_t launch_timelayer_gemm(const TimeGemmArgs& a, int form, hipStream_t s);
hipError_t launch_timelayer_attn_forward(const TimeAttnArgs& a, hipStream_t s);
hipError_t launch_timelayer_attn_backward(const TimeAttnArgs& a, hipStream_t s);
// u = x (+ z m; z, m nullable), y = LayerNorm(u); u, mean / rstd stored where given
hipError_t launch_timelayer_ln_forward(const float* x, const float* z, const float* m, const float* gamma,
                                       const float* beta, int R, int D, float* u, float* mean, float* rstd, float* y,
                                       hipStream_t s);
// du, dum = du m (m nullable: dum untouched), dgamma, dbeta; part: 2 timelayer_ln_chunks(R) D doubles
hipError_t launch_timelayer_ln_backward(const float* dy, const float* u, const float* mean, const float* rstd,
                                        const float* gamma, const float* m, int R, int D, float* du, float* dum,
                                        double* part, float* dgamma, float* dbeta, hipStream_t s);
hipError_t launch_timelayer_reduce(const double* part, int n_chunks, int n, float* out, hipStream_t s);
// out[n] = sum_r src[r][n]; part: timelayer_colsum_chunks(R) N doubles
hipError_t launch_timelayer_colsum(const float* src, int R, int N, double* part, float* out, hipStream_t s);

// ------------------------------------------------------------------ vge_linear.hip (training: a bias-free linear map)
// y [R][N] = x W^T, dx [R][K] = dy W, dW [N][K] = dy^T x on the GEMM of vge_f32gemm.h; x [R][K] with row stride ldx,
// W [N][K].  x needs 4-byte alignment only: an operand that is not 16-byte aligned row by row, or a K that is no
// multiple of 4, takes the scalar-load instantiations.  part: linear_wgrad_chunks(R) N K doubles.
int linear_wgrad_chunks(int R);
hipError_t launch_linear_forward(const float* x, int ldx, const float* W, float* y, int R, int K, int N, hipStream_t s);
hipError_t launch_linear_dgrad(const float* dy, const float* W, float* dx, int R, int K, int N, hipStream_t s);
hipError_t launch_linear_wgrad(const float* dy, const float* x, int ldx, double* part, float* dW, int R, int K, int N,
                               hipStream_t s);

// ------------------------------------------------------------------ vge_fusion.hip (training: the modality fusion)
// s, ds [R][M][D]; stats [4][R M] = mean0, rstd0 (the affine-free LayerNorm), mean1, rstd1 (kv_ln); a, m (null: all
// ones) [R][M]; p, dp [R][D]; qvec [3][D] = LN(latent) g_q + b_q, qv = Wq of it, u = Wk^T qv
struct FusionRowArgs {
  const float* s; const float* g_kv; const float* b_kv; const float* temp; const float* bias; const float* m;
  const float* qvec;
  float* stats; float* a;              // forward: written where given (both or neither); backward: read
  float* p;                            // forward: written
  const float* dp; float* ds;          // backward
  double* part;                        // backward: [chunks][3 D + 16] sums of du, dg_kv, db_kv, dbias[8], dscale[8]
  int R, M, D;
};
struct FusionQueryArgs {
  const float* latent; const float* g_q; const float* b_q; const float* Wq; const float* Wk;
  float* qvec;                         // forward: written; backward: read
  const float* sums;                   // backward: [3 D + 16] the reduced row sums
  const float* temp;
  float* d_latent; float* d_g_q; float* d_b_q; float* d_g_kv; float* d_b_kv; float* d_Wq; float* d_Wk;
  float* d_temp; float* d_bias;
  int M, D;
};
int fusion_row_chunks(int R);          // workgroups (partials) of the row backward
hipError_t launch_fusion_query_forward(const FusionQueryArgs& a, hipStream_t s);
hipError_t launch_fusion_query_backward(const FusionQueryArgs& a, hipStream_t s);
hipError_t launch_fusion_rows_forward(const FusionRowArgs& a, hipStream_t s);
hipError_t launch_fusion_rows_backward(const FusionRowArgs& a, hipStream_t s);

// ------------------------------------------------------------------ vge_score.hip
// d <= 256
hipError_t launch_centroid_accum(const float* seq, const int* cls, int n, int C, int d, float* sums, float* counts,
                                 hipStream_t s);
hipError_t launch_centroid_final(const float* sums, const float* counts, int C, int d, float* cent, hipStream_t s);
hipError_t launch_tc_windows(const float* fe, int B, int T1, int d, float* tc, hipStream_t s);
hipError_t launch_score_videos(const float* seq, const float* tcw, const int* first, const int* vcls, const float* cent,
                               int V, int d, float* ac, double* tc, hipStream_t s);

}  // namespace vge
