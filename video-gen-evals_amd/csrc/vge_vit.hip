// Per-frame mesh extractor (TokenHMR: ViT-H/16 backbone + SMPL token-decoder head) on gfx950.
//
// Reference: modifications/mesh_generator.py:119-171 runs TokenHMR on 256x256 person crops in batches of 8
// and keeps pred_smpl_params {body_pose, global_orient, betas, token_out} (modifications/token_head.py:180-246);
// extract_mesh.py:35-43 saves them as the npz arrays pose / global_orient / betas / vit that the scoring
// path reads.  The backbone is HMR2's ViT-H/16 (256x192 input = columns 32..223 of the crop, patch 16,
// padding 2, 16 x 12 tokens, embed 1280, 32 pre-norm blocks, 16 heads, MLP 5120, LayerNorm eps 1e-6).
//
// Kernels (all bf16 operands, f32 accumulation, residual stream kept in f32):
//   gemm_bf16_kernel<EPI>  C = A W^T (+ epilogue) for every Linear / the patch-embed conv (as im2col GEMM):
//                          256 x 256 tiles, 8 waves (2 M x 4 N, 128 x 64 per wave) on
//                          v_mfma_f32_32x32x16_bf16 (16x16x32 for the bf16-output epilogues), both operands
//                          staged HBM -> LDS by global_load_lds (16 B per lane) through a 5-stage x 32-k ring
//                          (160 KB, counted vmcnt), LDS image XOR-swizzled on the source address so the fragment
//                          ds_read_b128 are conflict-free; XCD-grouped tile order.  (Stage, tile walk, interleave and
//                          epilogue conversions shared with the conv kernels: vge_bf16_tile.h.)
//   gemm2_bf16_kernel<EPI> the same product on 128 x 256 tiles, two workgroups per CU (an A/B option, slower).
//   ln_bf16_kernel         LayerNorm f32 -> bf16 (one wave per row).
//   patchify_kernel        uint8 RGB crop -> normalised, zero-padded im2col rows of the 16x16 patches.
//   vit_attn_kernel        softmax(Q K^T / sqrt(hd)) V per (frame, head) on MFMA: S^T = K Q^T so a query's
//                          192 scores are lane-local (+ the partner half via permlane32), P^T feeds the
//                          PV MFMA straight from the accumulators.
//   xattn1_kernel          the decoder's one-query cross-attention over the 192 context tokens.
//   softmax_rows_kernel, readout_kernel (6D -> rotation matrix, mean-pose residuals), small helpers.
#include "vge_bf16_tile.h"
#include "vge_gemm.h"
#include "vge_hmr_k.h"
#include "vge_lds_attr.h"
#include <atomic>
#include <cstdlib>
#include <type_traits>

#ifndef VGE_GABL
#define VGE_GABL 0  // timing-only GEMM ablations (tools/ablate_gemm.sh): 1 no global_load_lds after the prologue,
                    // 2 no LDS fragment reads after the first, 4 no per-stage wait + barrier; 0 = the product
#endif

namespace {

// ------------------------------------------------------------------------------------------- GEMM
// 256 x 256 output tile per 512-thread workgroup; K in 32-deep stages through a 5-slot LDS ring (A 16 KB + B 16 KB
// per slot = 160 KB).  Step kt MFMAs stage kt from registers while the wave reads stage kt + 1's fragments from
// LDS (register double buffer, so no ds_read latency restarts at the per-stage barrier) and global_load_lds
// fills stage kt + 4; the per-stage wait is a counted vmcnt (stages kt + 2, kt + 3 stay in flight), never a drain.
constexpr int GB_M = 256, GB_N = 256, GB_K = 32, GB_ST = 5, GB_GM = 8;
constexpr int GB_TILE = GB_M * GB_K * 2;      // 16 KB per operand per stage
constexpr int GB_LDS = GB_ST * 2 * GB_TILE;   // 160 KB

using namespace vge;  // the epilogue ids GEMM_* (vge_gemm.h)

struct GemmBf16Args {
  const bf16* A;     // [M][lda]   rows of the activation
  const bf16* W;     // [N][ldw]   nn.Linear weight (row n = output column n)
  void* out;         // [M][ldo]   bf16 or f32
  const float* bias; // [N] or null
  const float* res;  // GEMM_RES_F32: [M][ldr] residual (may alias out)
  const float* pos;  // GEMM_PE_F32: pos_embed [tokens + 1][N]
  long lda, ldw, ldo, ldr;
  int M, N, K, tokens;
  const bf16* resb;  // GEMM_RESB_*: bf16 residual [M][ldr]
};

// NW = 8: waves 2 (M) x 4 (N), 128 x 64 per wave (2 waves per SIMD); NW = 4: waves 2 x 2, 128 x 128 per wave
// (one wave per SIMD, 256 accumulator registers): 25 % fewer LDS fragment bytes per MFMA.
// SH = 1 (NW = 8 only): the same wave tile on v_mfma_f32_16x16x32_bf16 (8 x 4 tiles of 16 x 16, one MFMA per 32-k
// stage and tile) -- same LDS fragment bytes and MFMA cycles per stage; the chip holds a higher clock on this shape
// (MI355X_MICROARCH.md, DVFS give-back item 7).
// PM: M is not a multiple of 256 (the last row tile's A loads clamp to row M - 1 and its stores stop at M); the ViT's
// GEMMs (M = frames x 192) take the PM = false code unchanged
template <int EPI, int NW, int SH = 0, bool PM = false>
__global__ void __launch_bounds__(64 * NW, 1) gemm_bf16_kernel(GemmBf16Args g) {
  static_assert(SH == 0 || NW == 8, "16x16x32 variant: 8 waves");
  constexpr int TN = NW == 8 ? 2 : 4;  // 32-column tiles per wave
  constexpr int LPS = 2 * (16 / NW);   // global_load_lds per thread per stage
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / (NW / 2), wn = wave % (NW / 2);
  // tile order: XCD-contiguous ids (xcd_remap), grouped panel walk (panel_tile)
  const int ntn = g.N / GB_N, mtn = (g.M + GB_M - 1) / GB_M;
  int mt, nt;
  panel_tile<GB_GM>(xcd_remap(blockIdx.x, gridDim.x), ntn, mtn, mt, nt);
  const int m0 = mt * GB_M, n0 = nt * GB_N;
  const int nk = g.K / GB_K;                 // >= 2 (K % 64 == 0)
  const int h = lane >> 5;
  const int swz = (lane >> 2) & 3;           // ((row >> 2) & 3) of every fragment row this lane reads
  const int rowoff = (lane & 31) * 64;

  floatx16 acc[SH ? 1 : 4][SH ? 1 : TN];
  floatx4 acq[SH ? 8 : 1][SH ? 4 : 1];  // SH = 1: 16 x 16 tiles [row tile][column tile]
  if constexpr (SH == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int u = 0; u < TN; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
  } else {
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) acq[t][u] = (floatx4){0.f, 0.f, 0.f, 0.f};
  }

  auto issue = [&](int st) {
    char* slot = lds + (st % GB_ST) * 2 * GB_TILE;
    stage_rows<GB_M, NW, PM>(g.A, g.lda, m0, st * GB_K, slot, wave, lane, g.M - 1);
    stage_rows<GB_N, NW, false>(g.W, g.ldw, n0, st * GB_K, slot + GB_TILE, wave, lane, g.N - 1);
  };
  struct Frag {
    bf16x8 a[2][4], b[2][TN];  // SH = 0: [16-k step][32-row / 32-column tile]; SH = 1: a = 8 16-row tiles, b = 4
  };
  auto read = [&](int st, Frag& f) {  // this wave's fragments of stage st (both 16-k steps)
    const char* cur = lds + (st % GB_ST) * 2 * GB_TILE;
    if constexpr (SH == 0) {
      const char* As = cur + wm * 128 * 64 + rowoff;
      const char* Bs = cur + GB_TILE + wn * (32 * TN) * 64 + rowoff;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int co = ((2 * s + h) ^ swz) * 16;
#pragma unroll
        for (int t = 0; t < 4; ++t) f.a[s][t] = *reinterpret_cast<const bf16x8*>(As + t * 32 * 64 + co);
#pragma unroll
        for (int u = 0; u < TN; ++u) f.b[s][u] = *reinterpret_cast<const bf16x8*>(Bs + u * 32 * 64 + co);
      }
    } else {
      // 16x16x32 fragments: lane -> row (lane & 15) of a 16-row tile, k chunk lane >> 4 of the stage's 32
      const int co = ((lane >> 4) ^ ((lane >> 2) & 3)) * 16, ro = (lane & 15) * 64;
      const char* As = cur + wm * 128 * 64 + ro + co;
      const char* Bs = cur + GB_TILE + wn * 64 * 64 + ro + co;
#pragma unroll
      for (int t = 0; t < 8; ++t) f.a[t >> 2][t & 3] = *reinterpret_cast<const bf16x8*>(As + t * 16 * 64);
#pragma unroll
      for (int u = 0; u < 4; ++u) f.b[u >> 1][u & 1] = *reinterpret_cast<const bf16x8*>(Bs + u * 16 * 64);
    }
  };
  auto mma = [&](const Frag& f, int s) {  // SH = 1: s = row tiles 4s..4s+3
    if constexpr (SH == 0) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < TN; ++u)
          acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[s][t], f.b[s][u], acc[t][u], 0, 0, 0);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acq[4 * s + t][u] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[s][t], f.b[u >> 1][u & 1], acq[4 * s + t][u], 0, 0, 0);
    }
  };
  constexpr int MPS = SH ? 2 : 1;  // MFMAs per step relative to the 32x32x16 schedule
  // Step kt: stage kt's fragments are already in registers (read during step kt - 1).  Wait for stage kt + 1 and
  // barrier (it also retires every wave's reads of stage kt - 1's slot); then one straight-line block: stage
  // kt + 4's global_load_lds into that slot interleaved with the first 16-k MFMAs, stage kt + 1's fragment reads
  // interleaved with the second (sched_group_barrier), so loads and LDS reads issue between MFMAs instead of in a
  // burst in front of them.  Branch-free: past the last stage the loads re-fetch stage nk - 1 into its own slot
  // (identical bytes) and the reads re-read it, so the wait is always vmcnt(2 LPS) (3 stages = 96 KB in flight).
  auto step = [&](int kt, Frag& cur, Frag& nxt) {
#if !(VGE_GABL & 4)
    vmcnt_b<2 * LPS>();  // outstanding: the loads of steps kt - 3 .. kt - 1 -> retire step kt - 3's (stage kt + 1)
    lds_barrier_b();
#endif
#if !(VGE_GABL & 1)
    issue(min(kt + 4, nk - 1));
#endif
#if !(VGE_GABL & 2)
    read(min(kt + 1, nk - 1), nxt);
#else
    nxt = cur;
#endif
    mma(cur, 0);
    mma(cur, 1);
    mfma_interleave<LPS, MPS * 8 / LPS, 4, MPS * 2, (8 + 2 * TN) / 4>();
  };
  for (int st = 0; st < GB_ST - 1; ++st) issue(min(st, nk - 1));
  vmcnt_b<3 * LPS>();  // retire stage 0
  lds_barrier_b();
  Frag f0, f1;
  read(0, f0);
  for (int kt = 0; kt < nk; kt += 2) {  // nk is even (K % 64 == 0)
    step(kt, f0, f1);
    step(kt + 1, f1, f0);
  }

  // Epilogue through LDS (free once every wave's tail loads and reads have retired): each wave writes half of its
  // 128 x (32 TN) accumulator tile (C layout, wave-private region, in-order LDS so no barrier) and reads it back
  // row-major, 16 B per lane, so bias / residual / position loads and the output stores are whole-row vector
  // accesses (256-B f32 rows, 128-B bf16 rows) instead of 2-4-byte column scatters.
  constexpr int WC = 32 * TN;            // wave tile columns
  constexpr int RPI = 64 / (WC / 4);     // rows per read instruction (16 B per lane)
#if (VGE_GABL & 8) && defined(__HIP_DEVICE_COMPILE__)  // no epilogue (the accumulators kept live)
  if constexpr (SH == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int u = 0; u < TN; ++u) asm volatile("" ::"v"(acc[t][u]));
  } else {
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) asm volatile("" ::"v"(acq[t][u]));
  }
  return;
#endif
  vmcnt_b<0>();
  lds_barrier_b();
  float* my = reinterpret_cast<float*>(lds) + wave * (64 * WC);
  const int lr = lane / (WC / 4), c4 = (lane % (WC / 4)) * 4;
  const int gcol = n0 + wn * WC + c4;
  floatx4 bb = {0.f, 0.f, 0.f, 0.f};
  if (g.bias) bb = *reinterpret_cast<const floatx4*>(g.bias + gcol);
  if constexpr (EPI == GEMM_PE_F32) bb += *reinterpret_cast<const floatx4*>(g.pos + gcol);  // pos_embed[:, :1]
  // f32 epilogues read one row vector per output (residual or position embedding): every load of a half is issued
  // before that half's LDS round trip, and the next half's while this one is written, so the epilogue pays about one
  // memory latency instead of one per 4-iteration batch
  constexpr int NIT = 64 / RPI;                          // row-major iterations per half
  constexpr bool RB = EPI == GEMM_RESB_BF16 || EPI == GEMM_RESB_RELU_BF16;
  constexpr bool LD = EPI == GEMM_RES_F32 || EPI == GEMM_PE_F32 || RB;
  constexpr int NPF = LD ? (NIT > 16 ? 16 : NIT) : 1;    // loads kept in flight (NW = 4: 16 of 32 per half)
  auto grow_of = [&](int half, int it) { return m0 + wm * 128 + half * 64 + it * RPI + lr; };
  auto rowload = [&](int half, int it) -> floatx4 {
    const int grow = PM ? min(grow_of(half, it), g.M - 1) : grow_of(half, it);  // (PM: rows past M are not stored)
    if constexpr (EPI == GEMM_RES_F32) return *reinterpret_cast<const floatx4*>(g.res + ((long)grow * g.ldr + gcol));
    if constexpr (RB) {
      return to_floatx4(*reinterpret_cast<const bf16x4*>(g.resb + ((long)grow * g.ldr + gcol)));
    }
    if constexpr (EPI == GEMM_PE_F32)  // tokens per frame = 192 (checked by the host)
      return *reinterpret_cast<const floatx4*>(g.pos + ((1 + grow - (grow / 192) * 192) * g.N + gcol));
    return floatx4{0.f, 0.f, 0.f, 0.f};
  };
  floatx4 rr[NPF];
  if constexpr (LD) {
#pragma unroll
    for (int it = 0; it < NPF; ++it) rr[it] = rowload(0, it);
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if constexpr (SH == 0) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int u = 0; u < TN; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            my[(tt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * WC + u * 32 + (lane & 31)] = acc[2 * half + tt][u][r];
    } else {
#pragma unroll
      for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            my[(tt * 16 + 4 * (lane >> 4) + r) * WC + u * 16 + (lane & 15)] = acq[4 * half + tt][u][r];
    }
    // NW = 4 only: there hipcc sank ds_writes of rows 4 k + 3 below the row-major ds_reads of those rows (other lanes
    // read them), which corrupted the rows of the f32 epilogues that load a row vector.  The 8-wave forms keep the
    // program order today (test_gemm_wave_modes_match_default and the conv variant tests pin their outputs); the
    // ordering point changes their listings, so it goes in with the next measured change of this epilogue
    if constexpr (NW == 4) wave_lds_order();
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int rl = it * RPI + lr;
      const int grow = grow_of(half, it);
      floatx4 v = *reinterpret_cast<const floatx4*>(my + rl * WC + c4) + bb;
      const long o = (long)grow * g.ldo + gcol;  // 64-bit: a 1x1 conv's output may pass 2^31 elements
      if constexpr (RB || EPI == GEMM_RELU_BF16) {  // the 1x1 conv epilogues: bias (+ bf16 residual) (+ ReLU) -> bf16
        if constexpr (RB) {
          v += (it < NPF) ? rr[it % NPF] : rowload(half, it);
          if (it < NPF && half == 0) rr[it % NPF] = rowload(1, it);
        }
        if constexpr (EPI == GEMM_RELU_BF16 || EPI == GEMM_RESB_RELU_BF16)
          v = relu4(v);
        bf16x4 ob;  // (not to_bf16x4: with it the partial-M kernels' stores come out in another order)
        ob[0] = (bf16)v.x; ob[1] = (bf16)v.y; ob[2] = (bf16)v.z; ob[3] = (bf16)v.w;
        if (!PM || grow < g.M) *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(g.out) + o) = ob;
      } else if constexpr (EPI == GEMM_BF16 || EPI == GEMM_GELU_BF16) {
        if constexpr (EPI == GEMM_GELU_BF16) {  // exact-erf GELU: the one-exp2 form (|error| < 4.8e-7) flips enough
          floatx2 y[2] = {{v.x, v.y}, {v.z, v.w}};  // bf16 roundings to move TokenHMR's global_orient past the e2e
          gelu2_many(y);                              // chain's 1.5e-2 bound vs the bf16-point oracle (1.68e-2, r04 box)
          v = {y[0].x, y[0].y, y[1].x, y[1].y};
        }
        bf16x4 ob;  // (not to_bf16x4: with it the partial-M kernels' stores come out in another order)
        ob[0] = (bf16)v.x; ob[1] = (bf16)v.y; ob[2] = (bf16)v.z; ob[3] = (bf16)v.w;
        if (!PM || grow < g.M) *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(g.out) + o) = ob;
      } else {
        v += (it < NPF) ? rr[it % NPF] : rowload(half, it);
        if (!PM || grow < g.M) *reinterpret_cast<floatx4*>(reinterpret_cast<float*>(g.out) + o) = v;
        if (it < NPF && half == 0) rr[it % NPF] = rowload(1, it);  // the next half's, in the freed register
      }
    }
    if constexpr (NW == 4) wave_lds_order();
  }
}

// ------------------------------------------------------------- GEMM, persistent (gemmp)
// The 16x16x32 8-wave tile of gemm_bf16_kernel (SH = 1), persistent: one workgroup per CU walks its tiles (virtual
// block b + i G through xcd_remap, G a multiple of 8, so an XCD's workgroups take consecutive tiles of that XCD's
// range at a time, as the one-tile kernel's do) through ONE continuous 5-slot ring: the next tile's first four stages
// are issued during this tile's last four steps, and the epilogue -- bias, GELU / ReLU, bf16, 8-B stores straight from
// the accumulators after a quad transpose (lane i of a quad takes row i, four consecutive columns), no LDS -- runs
// while they land.  The one-tile kernel pays its epilogue (an LDS round trip and the stores) and the next workgroup's
// prologue (four stages of loads before its first MFMA) back to back on every tile: 13-36 % of the ViT GEMMs' time
// (VGE_GABL 8, profiles/ab_r05p_gemm_ablation.json).
// vmcnt accounting (loads and stores retire in issue order): a step waits for its next stage with the two later stages
// in flight (2 LPS); the tile's bias is loaded by inline asm at the top of its second-to-last step (hipcc's waitcnt
// pass answers a compiler-visible load issued among LDS-DMA loads with vmcnt(0)), so the last step also lets those
// NCL loads be outstanding and the epilogue retires them at 2 LPS; the epilogue's NST stores follow the next tile's
// stage 3, so that tile's steps 0..2 let them be outstanding too.  Stores go through a per-tile buffer descriptor
// (rows past M fall outside it and are dropped): one store instruction per (row tile, column tile) on every path,
// which the counts rely on.  Residual-free bf16 epilogues only (GEMM_BF16, GEMM_GELU_BF16, GEMM_RELU_BF16), a bias, K / 32
// >= 6 (so the bias and store windows of a tile never meet).
constexpr int GP_LPS = 4;   // global_load_lds per thread per stage (2 A + 2 W)
constexpr int GP_NST = 32;  // epilogue stores per thread: 8 row tiles x 4 column tiles of 16 x 16
constexpr int GP_NCL = 4;   // bias loads per thread: one floatx4 per column tile

template <int EPI, bool PM>
__global__ void __launch_bounds__(512, 1) gemmp_bf16_kernel(GemmBf16Args g) {
  static_assert(EPI == GEMM_BF16 || EPI == GEMM_GELU_BF16 || EPI == GEMM_RELU_BF16, "residual-free bf16 epilogues");
  constexpr int LPS = GP_LPS;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / 4, wn = wave % 4;
  const int ntn = g.N / GB_N, mtn = (g.M + GB_M - 1) / GB_M, ntiles = mtn * ntn;
  const int G = gridDim.x, b = blockIdx.x;
  const int T = (ntiles - b + G - 1) / G;  // >= 1 (host: G <= ntiles)
  const int nk = g.K / GB_K;               // even, >= 6 (host)
  const int total = T * nk;
  auto tile_mn = [&](int i, int& m0, int& n0) {
    int mt, nt;
    panel_tile<GB_GM>(xcd_remap(b + i * G, ntiles), ntn, mtn, mt, nt);
    m0 = mt * GB_M;
    n0 = nt * GB_N;
  };

  // ---- issue side: the next stage to load (global stage index is_g = tile is_i, k stage is_k); past the last stage
  // it re-loads that stage into its own slot (identical bytes), so every step issues LPS loads
  int is_g = 0, is_i = 0, is_k = 0, is_m0, is_n0;
  tile_mn(0, is_m0, is_n0);
  auto issue_next = [&]() {
    char* slot = lds + (is_g % GB_ST) * 2 * GB_TILE;
    stage_rows<GB_M, 8, PM>(g.A, g.lda, is_m0, is_k * GB_K, slot, wave, lane, g.M - 1);
    stage_rows<GB_N, 8, false>(g.W, g.ldw, is_n0, is_k * GB_K, slot + GB_TILE, wave, lane, g.N - 1);
    if (is_g + 1 < total) {
      ++is_g;
      if (++is_k == nk) {
        is_k = 0;
        tile_mn(++is_i, is_m0, is_n0);
      }
    }
  };

  // ---- compute side (gemm_bf16_kernel's SH = 1 fragments and MFMAs)
  floatx4 acq[8][4];
  auto zero = [&]() {
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) acq[t][u] = (floatx4){0.f, 0.f, 0.f, 0.f};
  };
  zero();
  struct Frag {
    bf16x8 a[2][4], b[2][2];
  };
  const int co = ((lane >> 4) ^ ((lane >> 2) & 3)) * 16, ro = (lane & 15) * 64;
  auto read = [&](int st, Frag& f) {
    const char* cur = lds + (st % GB_ST) * 2 * GB_TILE;
    const char* As = cur + wm * 128 * 64 + ro + co;
    const char* Bs = cur + GB_TILE + wn * 64 * 64 + ro + co;
#pragma unroll
    for (int t = 0; t < 8; ++t) f.a[t >> 2][t & 3] = *reinterpret_cast<const bf16x8*>(As + t * 16 * 64);
#pragma unroll
    for (int u = 0; u < 4; ++u) f.b[u >> 1][u & 1] = *reinterpret_cast<const bf16x8*>(Bs + u * 16 * 64);
  };
  auto mma = [&](const Frag& f, int s) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u)
        acq[4 * s + t][u] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[s][t], f.b[u >> 1][u & 1], acq[4 * s + t][u], 0, 0, 0);
  };

  // ---- epilogue state: the tile's bias, one column per lane and column tile (the bias and the activation are applied
  // in the MFMA layout, where a lane holds one column of four rows, before the transpose); asm loads, retired by count
  float bb[4];
  const int cq = 4 * ((lane & 15) >> 2);  // this lane's first column of a 16-column tile after the transpose
  auto load_consts = [&](int i) {
    int m0, n0;
    tile_mn(i, m0, n0);
    int lc = lane & 15;
    asm volatile("" : "+v"(lc));  // opaque per call: keeps LICM from hoisting the pointer (live across the loop, spilled)
    const float* bp = g.bias + n0 + wn * 64 + lc;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      asm volatile("global_load_dword %0, %1, off" : "=v"(bb[u]) : "v"(bp + 16 * u) : "memory");
  };
  // wait: 1 = the previous epilogue's stores may be outstanding, 2 = this tile's bias loads may, 0 = neither; only
  // the wait instruction is branched on (one copy of the step body: copies per mode raise the register pressure)
  auto step = [&](int wait, bool consts, int gs, Frag& cur, Frag& nxt, int ci) {
    if (wait == 1)
      vmcnt_b<2 * LPS + GP_NST>();  // stage gs + 1 landed (its two successors, + what the mode names, in flight)
    else if (wait == 2)
      vmcnt_b<2 * LPS + GP_NCL>();
    else
      vmcnt_b<2 * LPS>();
    lds_barrier_b();   // ... for every wave; every wave is done reading stage gs - 1's slot
    if (consts) load_consts(ci);
    __builtin_amdgcn_sched_barrier(0);
    issue_next();      // stage gs + 4 into stage gs - 1's slot
    read(min(gs + 1, total - 1), nxt);
    mma(cur, 0);
    mma(cur, 1);
    mfma_interleave<LPS, 2 * 8 / LPS, 4, 4, 3>();
  };
  const bool o1 = lane & 1, o2 = lane & 2;
  auto epilogue = [&](int i) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(bb[0]), "+v"(bb[1]), "+v"(bb[2]), "+v"(bb[3]) : "i"(2 * LPS) : "memory");
    int m0, n0;
    tile_mn(i, m0, n0);
    const int rows = min(GB_M, g.M - m0);
    const __amdgpu_buffer_rsrc_t ob = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<char*>(g.out) + (size_t)m0 * g.ldo * 2, (short)0, (int)((size_t)rows * g.ldo * 2), 0x00020000);
    int r0 = wm * 128 + 4 * (lane >> 4) + (lane & 3);
    asm volatile("" : "+v"(r0));  // opaque per tile: the 32 store offsets are not hoisted out of the tile loop (spills)
    const int c0 = n0 + wn * 64 + cq;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        floatx4 v = acq[t][u] + bb[u];
        if constexpr (EPI == GEMM_RELU_BF16) v = relu4(v);
        if constexpr (EPI == GEMM_GELU_BF16) {
          floatx2 y[2] = {{v.x, v.y}, {v.z, v.w}};
          gelu2_many(y);
          v = floatx4{y[0].x, y[0].y, y[1].x, y[1].y};
        }
        const bf16x4 o = to_bf16x4(quad_t4(v, o1, o2));
        const int off = ((r0 + 16 * t) * (int)g.ldo + c0 + 16 * u) * 2;  // < rows x ldo x 2 < 2^31 (host)
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(uintx2_t, o), ob, off, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);
  };

  for (int st = 0; st < GB_ST - 1; ++st) issue_next();  // stages 0..3
  vmcnt_b<3 * LPS>();                                     // stage 0 landed
  lds_barrier_b();
  Frag f0, f1;
  read(0, f0);
  // step kk of tile i: steps 0..2 of the tiles after the first let the previous epilogue's stores be outstanding, step
  // nk - 2 loads the tile's bias ahead of its ring loads, step nk - 1 lets those loads be outstanding; f0 holds the
  // fragments of even steps (nk is even)
  int gs = 0;
  for (int i = 0; i < T; ++i) {
    for (int kk = 0; kk < nk; kk += 2) {
      step((i > 0 && kk < 3) ? 1 : 0, kk == nk - 2, gs++, f0, f1, i);
      step((i > 0 && kk + 1 < 3) ? 1 : kk + 1 == nk - 1 ? 2 : 0, false, gs++, f1, f0, i);
    }
    epilogue(i);
    zero();
  }
  vmcnt_b<0>();
}

// ------------------------------------------------------------- GEMM, two workgroups per CU (gemm2)
// The 256 x 256 kernel above holds a CU alone (160 KB of LDS), so its epilogue -- the bias / GELU / residual pass, which
// moves the output tile's bytes at the chip's HBM rate because every CU reaches it at the same time -- leaves the
// matrix pipe idle: without it the ViT-H GEMMs run 13-36 % faster (`VGE_GABL` 8, profiles/ab_r05p_gemm_ablation.json).
// gemm2 halves the tile (128 x 256, 4 waves of 64 x 128, same fragment bytes per MFMA) and the LDS (a 3-slot x 32-k
// ring, 72 KB), so two workgroups share a CU and one's epilogue runs beside the other's MFMAs.  The epilogue needs no
// LDS: the MFMA operands are swapped (weights as A, activations as B), so a lane's accumulators are 4 consecutive
// output columns of one row (v_mfma_f32_32x32x16_bf16 D layout: lane l -> row l & 31, registers 4g..4g+3 -> columns
// 8g + 4 (l >> 5) .. + 3) and bias / residual / position loads and the output stores are 16-B (f32) or 8-B (bf16)
// vector accesses straight from the registers.  The products and their k order are the 256 x 256 kernel's.
constexpr int G2_M = 128, G2_N = 256, G2_K = 32, G2_ST = 3, G2_GM = 16;
constexpr int G2_TA = G2_M * G2_K * 2;       // 8 KB of A per stage
constexpr int G2_SLOT = G2_TA + G2_N * G2_K * 2;  // + 16 KB of W = 24 KB
constexpr int G2_LDS = G2_ST * G2_SLOT;     // 72 KB

template <bool B>
struct BoolC {
  static constexpr bool value = B;
};

template <int EPI, bool PM>
__global__ void __launch_bounds__(256, 2) gemm2_bf16_kernel(GemmBf16Args g) {
  constexpr int LPS = G2_M / 64 + G2_N / 64;  // global_load_lds per thread per stage (2 A + 4 W)
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = g.N / G2_N, mtn = (g.M + G2_M - 1) / G2_M;
  int mt, nt;
  panel_tile<G2_GM>(xcd_remap(blockIdx.x, gridDim.x), ntn, mtn, mt, nt);
  const int m0 = mt * G2_M, n0 = nt * G2_N;
  const int nk = g.K / G2_K;  // >= 2, even
  const int h = lane >> 5;
  const int swz = (lane >> 2) & 3;
  const int rowoff = (lane & 31) * 64;

  floatx16 acc[2][4];  // [32-row tile t][32-column tile u]
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;

  auto issue = [&](int st) {
    char* slot = lds + (st % G2_ST) * G2_SLOT;
    stage_rows<G2_M, 4, PM>(g.A, g.lda, m0, st * G2_K, slot, wave, lane, g.M - 1);
    stage_rows<G2_N, 4, false>(g.W, g.ldw, n0, st * G2_K, slot + G2_TA, wave, lane, g.N - 1);
  };
  struct Frag {
    bf16x8 a[2][2], b[2][4];  // [16-k step][tile]
  };
  auto read = [&](int st, Frag& f) {
    const char* cur = lds + (st % G2_ST) * G2_SLOT;
    const char* As = cur + wm * 64 * 64 + rowoff;
    const char* Bs = cur + G2_TA + wn * 128 * 64 + rowoff;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int co = ((2 * s + h) ^ swz) * 16;
#pragma unroll
      for (int t = 0; t < 2; ++t) f.a[s][t] = *reinterpret_cast<const bf16x8*>(As + t * 32 * 64 + co);
#pragma unroll
      for (int u = 0; u < 4; ++u) f.b[s][u] = *reinterpret_cast<const bf16x8*>(Bs + u * 32 * 64 + co);
    }
  };
  auto mma = [&](const Frag& f, int s) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u)
        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.b[s][u], f.a[s][t], acc[t][u], 0, 0, 0);
  };
  // Step kt: stage kt's fragments are in registers (read during step kt - 1).  Wait for stage kt + 1 (issued at step
  // kt - 2; stage kt + 2 stays in flight) and barrier: every wave's reads of stage kt's slot have retired (the
  // barrier's lgkmcnt(0)), so stage kt + 3 goes into that slot.  Past the last stage the loads re-fetch stage nk - 1
  // (identical bytes; at step nk - 1 into its own slot, whose fragments are already in registers) and the reads
  // re-read it, so every wait is the same count.
  auto step = [&](int kt, Frag& cur, Frag& nxt) {
    vmcnt_b<LPS>();
    lds_barrier_b();
    issue(min(kt + 3, nk - 1));
    read(min(kt + 1, nk - 1), nxt);
    mma(cur, 0);
    mma(cur, 1);
    mfma_interleave<LPS, 1, 6, 1, 2>();
  };
  issue(0);
  issue(1);
  issue(min(2, nk - 1));
  vmcnt_b<2 * LPS>();  // retire stage 0
  lds_barrier_b();
  Frag f0, f1;
  read(0, f0);
  for (int kt = 0; kt < nk; kt += 2) {
    step(kt, f0, f1);
    step(kt + 1, f1, f0);
  }
  vmcnt_b<0>();  // the tail's re-fetches land before the workgroup's LDS can be handed on

  // ---- epilogue from the registers: lane -> row m0 + 64 wm + 32 t + (lane & 31), columns nb .. nb + 3 of group g;
  // UB column tiles per batch (every load of a batch in flight together; the position-embedding epilogue, with two
  // row vectors per output, takes one tile at a time to stay inside 256 registers)
  constexpr bool RB = EPI == GEMM_RESB_BF16 || EPI == GEMM_RESB_RELU_BF16;
  constexpr int UB = EPI == GEMM_PE_F32 ? 1 : 4;
  const int cb = n0 + wn * 128 + 4 * h;
  // (one branch on the bias pointer around the whole epilogue: a per-load test makes hipcc branch and drain vmcnt
  // around every load)
  auto epilogue = [&](auto hb) {
  constexpr bool HB = decltype(hb)::value;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = m0 + wm * 64 + t * 32 + (lane & 31);
    const int lrow = PM ? min(row, g.M - 1) : row;  // (PM: rows past M are loaded clamped, never stored)
    const bool st_ok = !PM || row < g.M;
#pragma unroll
    for (int u0 = 0; u0 < 4; u0 += UB) {
      floatx4 v[UB][4];  // [u - u0][g]
#pragma unroll
      for (int u = 0; u < UB; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          v[u][q] = floatx4{acc[t][u0 + u][4 * q], acc[t][u0 + u][4 * q + 1], acc[t][u0 + u][4 * q + 2],
                            acc[t][u0 + u][4 * q + 3]};
      // (acc + (bias + pos_embed[0])) + pos_embed[1 + token]: the 256 x 256 kernel's operation order
#pragma unroll
      for (int u = 0; u < UB; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = cb + (u0 + u) * 32 + 8 * q;
          floatx4 bb = {0.f, 0.f, 0.f, 0.f};
          if constexpr (HB) bb = *reinterpret_cast<const floatx4*>(g.bias + c);
          if constexpr (EPI == GEMM_PE_F32) bb += *reinterpret_cast<const floatx4*>(g.pos + c);
          v[u][q] += bb;
        }
      if constexpr (EPI == GEMM_PE_F32) {  // tokens per frame = 192 (checked by the host)
        const float* pr = g.pos + (long)(1 + lrow - (lrow / 192) * 192) * g.N + cb;
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q) v[u][q] += *reinterpret_cast<const floatx4*>(pr + (u0 + u) * 32 + 8 * q);
      }
      if constexpr (EPI == GEMM_RES_F32) {
        const float* rr = g.res + (long)lrow * g.ldr + cb;
        floatx4 rv[UB][4];
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q) rv[u][q] = *reinterpret_cast<const floatx4*>(rr + (u0 + u) * 32 + 8 * q);
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q) v[u][q] += rv[u][q];
      }
      if constexpr (RB) {
        const bf16* rr = g.resb + (long)lrow * g.ldr + cb;
        bf16x4 rv[UB][4];
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q) rv[u][q] = *reinterpret_cast<const bf16x4*>(rr + (u0 + u) * 32 + 8 * q);
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            v[u][q] += to_floatx4(rv[u][q]);
      }
      if constexpr (EPI == GEMM_RELU_BF16 || EPI == GEMM_RESB_RELU_BF16) {
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q) v[u][q] = relu4(v[u][q]);
      }
      if constexpr (EPI == GEMM_GELU_BF16) {
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          floatx2 y[8];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            y[2 * q] = floatx2{v[u][q].x, v[u][q].y};
            y[2 * q + 1] = floatx2{v[u][q].z, v[u][q].w};
          }
          gelu2_many(y);
#pragma unroll
          for (int q = 0; q < 4; ++q) v[u][q] = floatx4{y[2 * q].x, y[2 * q].y, y[2 * q + 1].x, y[2 * q + 1].y};
        }
      }
      if (st_ok) {
        if constexpr (EPI == GEMM_RES_F32 || EPI == GEMM_PE_F32 || EPI == GEMM_F32) {
          float* o = reinterpret_cast<float*>(g.out) + (long)row * g.ldo + cb;
#pragma unroll
          for (int u = 0; u < UB; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<floatx4*>(o + (u0 + u) * 32 + 8 * q) = v[u][q];
        } else {
          bf16* o = reinterpret_cast<bf16*>(g.out) + (long)row * g.ldo + cb;
#pragma unroll
          for (int u = 0; u < UB; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<bf16x4*>(o + (u0 + u) * 32 + 8 * q) = to_bf16x4(v[u][q]);
        }
      }
    }
  }
  };
  if (g.bias)
    epilogue(BoolC<true>{});
  else
    epilogue(BoolC<false>{});
}

// ------------------------------------------------------------------------------------- LayerNorm
// y = (x - mean) / sqrt(var + eps) * w + b over D = 256 NV columns, one wave per row (4 rows per block)
template <int NV>
__global__ void __launch_bounds__(256) ln_bf16_kernel(const float* __restrict__ x, long ldx, bf16* __restrict__ y,
                                                      long ldy, const float* __restrict__ w,
                                                      const float* __restrict__ b, int rows, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  constexpr int D = 256 * NV;
  const float* xr = x + (size_t)row * ldx;
  floatx4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    v[i] = *reinterpret_cast<const floatx4*>(xr + 4 * (lane + 64 * i));
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  const float mean = wave_sum(s) * (1.0f / D);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const floatx4 d = v[i] - mean;
    q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / D) + eps);
  bf16* yr = y + (size_t)row * ldy;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = 4 * (lane + 64 * i);
    const floatx4 ww = *reinterpret_cast<const floatx4*>(w + c);
    const floatx4 bb = *reinterpret_cast<const floatx4*>(b + c);
    const floatx4 o = (v[i] - mean) * rstd * ww + bb;
    *reinterpret_cast<bf16x4*>(yr + c) = to_bf16x4(o);
  }
}

// f32 -> bf16 copy of a [rows][D] block (D % 4 == 0)
__global__ void cast_bf16_kernel(const float* __restrict__ x, long ldx, bf16* __restrict__ y, long ldy, int rows,
                                 int D) {
  const int q = D / 4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)rows * q) return;
  const int r = (int)(i / q), c = (int)(i % q) * 4;
  const floatx4 v = *reinterpret_cast<const floatx4*>(x + (size_t)r * ldx + c);
  *reinterpret_cast<bf16x4*>(y + (size_t)r * ldy + c) = to_bf16x4(v);
}

// rows [0, rows) of a [rows][D] f32 block = vec[D] (the decoder's input token: to_token_embedding of the
// zero token = its bias, plus pos_embedding)
__global__ void bcast_rows_kernel(const float* __restrict__ vec, float* __restrict__ y, int rows, int D) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (long)rows * D) y[i] = vec[i % D];
}

// ------------------------------------------------------------------------------------- patchify
// Patch-embed input rows: A[f * gh * gw + py * gw + px][c * P * P + ky * P + kx] =
//   (img[f][py P - pad + ky][x0 + px P - pad + kx][c] - mean[c]) / std[c], zero outside the img_h x img_w crop
// (the conv's zero padding applies to the normalised image).  One thread per 8 consecutive kx.
struct PatchArgs {
  const uint8_t* frames;  // [F][in_h][in_w][3] RGB
  bf16* out;              // [F * gh * gw][3 P P]
  int F, in_h, in_w, x0, img_h, img_w, P, pad, gh, gw;
  float mean[3], stdv[3];
};

__global__ void patchify_kernel(PatchArgs a) {
  const int K = 3 * a.P * a.P, kc8 = K / 8, kxc = a.P / 8;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)a.F * a.gh * a.gw * kc8;
  if (i >= total) return;
  const int kc = (int)(i % kc8);
  const long row = i / kc8;
  const int f = (int)(row / (a.gh * a.gw)), p = (int)(row % (a.gh * a.gw));
  const int py = p / a.gw, px = p % a.gw;
  const int c = kc / (a.P * kxc), ky = (kc / kxc) % a.P, kx0 = (kc % kxc) * 8;
  const int y = py * a.P - a.pad + ky;
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int x = px * a.P - a.pad + kx0 + j;
    float v = 0.f;
    if (y >= 0 && y < a.img_h && x >= 0 && x < a.img_w) {
      const float u = (float)a.frames[(((size_t)f * a.in_h + y) * a.in_w + a.x0 + x) * 3 + c];
      v = (u - a.mean[c]) / a.stdv[c];
    }
    o[j] = (bf16)v;
  }
  *reinterpret_cast<bf16x8*>(a.out + (size_t)row * K + kc * 8) = o;
}

// ------------------------------------------------------------------------------------- attention
// softmax(Q K^T * scale) V for one (frame, head): qkv rows [tok0, tok0 + 192), q / k / v at column offsets
// 0 / D / 2D + head * HD (timm's qkv.reshape(B, N, 3, heads, hd)).  6 waves, wave w = queries 32w..32w+31.
constexpr int AT_T = 192;
template <int HD>
struct AttnCfg {
  static constexpr int KS = HD + 8;                 // K row stride (bf16): conflict-free b128 fragment reads
  static constexpr int DP = (HD + 31) / 32 * 32;    // V^T rows padded to whole 32-row MFMA tiles
  static constexpr int VS = AT_T + 8;               // V^T row stride (bf16)
  static constexpr int LDS = (AT_T * KS + DP * VS) * 2;
};

template <int HD>
__global__ void __launch_bounds__(384) vit_attn_kernel(const bf16* __restrict__ qkv, long ldq, bf16* __restrict__ out,
                                                       long ldo, int D, int heads, float scale_log2) {
  using C = AttnCfg<HD>;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  bf16* Ks = reinterpret_cast<bf16*>(lds);
  bf16* Vt = Ks + AT_T * C::KS;
  const int f = blockIdx.x / heads, hd = blockIdx.x % heads;
  const size_t tok0 = (size_t)f * AT_T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, i = lane & 31;
  constexpr int CH = HD / 8;
  const bf16* kbase = qkv + tok0 * ldq + D + hd * HD;
  const bf16* vbase = kbase + D;
  for (int c = tid; c < AT_T * CH; c += 384) {
    const int row = c / CH, ch = c % CH;
    *reinterpret_cast<bf16x8*>(Ks + row * C::KS + ch * 8) =
        *reinterpret_cast<const bf16x8*>(kbase + (size_t)row * ldq + ch * 8);
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(vbase + (size_t)row * ldq + ch * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) Vt[(ch * 8 + j) * C::VS + row] = v[j];
  }
  for (int c = tid; c < (C::DP - HD) * AT_T; c += 384) Vt[(HD + c / AT_T) * C::VS + c % AT_T] = (bf16)0.f;

  // this lane's query row: B fragments of Q^T
  const int q = wave * 32 + i;
  bf16x8 qf[HD / 16];
  const bf16* qrow = qkv + (tok0 + q) * ldq + hd * HD + 8 * h;
#pragma unroll
  for (int s = 0; s < HD / 16; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qrow + 16 * s);
  __syncthreads();

  floatx16 st[AT_T / 32];  // S^T tiles: [key][query], lane = query
#pragma unroll
  for (int kt = 0; kt < AT_T / 32; ++kt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) st[kt][r] = 0.f;
    const bf16* krow = Ks + (kt * 32 + i) * C::KS + 8 * h;
#pragma unroll
    for (int s = 0; s < HD / 16; ++s)
      st[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(krow + 16 * s), qf[s], st[kt],
                                                       0, 0, 0);
  }
  float m = -3.0e38f;
#pragma unroll
  for (int kt = 0; kt < AT_T / 32; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, st[kt][r]);
  {
    const auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    m = fmaxf(__uint_as_float(r2[0]), __uint_as_float(r2[1]));
  }
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < AT_T / 32; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = __builtin_amdgcn_exp2f((st[kt][r] - m) * scale_log2);
      st[kt][r] = p;
      sum += p;
    }
  {
    const auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(sum), __float_as_uint(sum), false, false);
    sum = __uint_as_float(r2[0]) + __uint_as_float(r2[1]);
  }

  // O^T[d][query] = V^T P^T: k-step (kt, sub) takes accumulator registers 8 sub .. 8 sub + 7 of S^T tile kt as
  // the B fragment; its element j of lane half h is key kt*32 + 16 sub + 8 (j >> 2) + 4 h + (j & 3)
  floatx16 o[C::DP / 32];
#pragma unroll
  for (int dt = 0; dt < C::DP / 32; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
#pragma unroll
  for (int kt = 0; kt < AT_T / 32; ++kt)
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      bf16x8 pb;
#pragma unroll
      for (int j = 0; j < 8; ++j) pb[j] = (bf16)st[kt][8 * sub + j];
      const int key = kt * 32 + 16 * sub + 4 * h;
#pragma unroll
      for (int dt = 0; dt < C::DP / 32; ++dt) {
        const bf16* vr = Vt + (dt * 32 + i) * C::VS + key;
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vr);
        const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vr + 8);
        const bf16x8 va = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pb, o[dt], 0, 0, 0);
      }
    }
  const float inv = 1.0f / sum;
  bf16* orow = out + (tok0 + q) * ldo + hd * HD;
#pragma unroll
  for (int dt = 0; dt < C::DP / 32; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d = dt * 32 + 8 * g4 + 4 * h;
      if (d < HD) {
        bf16x4 ob;
#pragma unroll
        for (int j = 0; j < 4; ++j) ob[j] = (bf16)(o[dt][4 * g4 + j] * inv);
        *reinterpret_cast<bf16x4*>(orow + d) = ob;
      }
    }
}

// One-query cross-attention of the decoder (HMR2 pose_transformer CrossAttention with a single token): per
// (frame, head), scores over the frame's 192 context tokens, softmax, weighted sum of v.  One wave, dim_head 64.
__global__ void __launch_bounds__(64) xattn1_kernel(const bf16* __restrict__ qv, long ldq, const bf16* __restrict__ kv,
                                                    long ldkv, bf16* __restrict__ out, long ldo, int inner, int heads,
                                                    int ctx, float scale) {
  __shared__ float p[256];
  const int f = blockIdx.x / heads, hd = blockIdx.x % heads, lane = threadIdx.x;
  const bf16* qr = qv + (size_t)f * ldq + hd * 64;
  float qreg[64];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(qr + 8 * c);
#pragma unroll
    for (int j = 0; j < 8; ++j) qreg[8 * c + j] = (float)t[j];
  }
  float m = -3.0e38f;
  for (int k = lane; k < ctx; k += 64) {
    const bf16* kr = kv + ((size_t)f * ctx + k) * ldkv + hd * 64;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const bf16x8 t = *reinterpret_cast<const bf16x8*>(kr + 8 * c);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += qreg[8 * c + j] * (float)t[j];
    }
    s *= scale;
    p[k] = s;
    m = fmaxf(m, s);
  }
  m = wave_max(m);
  float sum = 0.f;
  for (int k = lane; k < ctx; k += 64) {
    const float e = __expf(p[k] - m);
    p[k] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  __syncthreads();
  float acc = 0.f;
  const bf16* vb = kv + (size_t)f * ctx * ldkv + inner + hd * 64 + lane;
  for (int k = 0; k < ctx; ++k) acc += p[k] * (float)vb[(size_t)k * ldkv];
  out[(size_t)f * ldo + hd * 64 + lane] = (bf16)(acc / sum);
}

// softmax over each row of C logits (f32 in, bf16 out), one wave per row
__global__ void __launch_bounds__(256) softmax_rows_kernel(const float* __restrict__ x, bf16* __restrict__ y, int rows,
                                                           int C) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (size_t)row * C;
  float m = -3.0e38f;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, xr[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf(xr[c] - m);
  const float inv = 1.0f / wave_sum(s);
  for (int c = lane; c < C; c += 64) y[(size_t)row * C + c] = (bf16)(__expf(xr[c] - m) * inv);
}

// Readout (token_head.py:207-246): body 6D = [grot | decoded body pose | hands] + init_body_pose, HMR2
// rot6d_to_rotmat (Gram-Schmidt, F.normalize eps 1e-12), global_orient = joint 0, body_pose = joints 1..23;
// betas = decshape + init_betas; vit = token_out.  One thread per (frame, joint); joint 0 also writes betas.
struct ReadoutArgs {
  const float* rd;        // [Fp][ldrd]: grot 0..5 | hands 6..17 | shape 18..27 | cam 28..30
  const float* bp;        // [Fp][ldbp]: decoded body pose 6D, 21 joints
  const float* init_pose; // [24 * 6]
  const float* init_betas;// [10]
  float* pose;            // [F][207]
  float* gori;            // [F][9]
  float* betas;           // [F][10]
  int F, ldrd, ldbp;
};

__global__ void readout_kernel(ReadoutArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.F * 24) return;
  const int f = i / 24, j = i % 24;
  const float* src = j == 0 ? a.rd + (size_t)f * a.ldrd : j <= 21 ? a.bp + (size_t)f * a.ldbp + (j - 1) * 6
                                                                   : a.rd + (size_t)f * a.ldrd + 6 + (j - 22) * 6;
  float x[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = src[k] + a.init_pose[j * 6 + k];
  // x.reshape(2, 3).T: a1 = (x0, x1, x2), a2 = (x3, x4, x5)
  float n1 = fmaxf(sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), 1e-12f);
  const float b1[3] = {x[0] / n1, x[1] / n1, x[2] / n1};
  const float d = b1[0] * x[3] + b1[1] * x[4] + b1[2] * x[5];
  float u[3] = {x[3] - d * b1[0], x[4] - d * b1[1], x[5] - d * b1[2]};
  const float n2 = fmaxf(sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), 1e-12f);
  const float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
  const float b3[3] = {b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
  float* o = j == 0 ? a.gori + (size_t)f * 9 : a.pose + (size_t)f * 207 + (j - 1) * 9;
#pragma unroll
  for (int r = 0; r < 3; ++r) {  // R[r][c] = b_c[r]
    o[r * 3 + 0] = b1[r];
    o[r * 3 + 1] = b2[r];
    o[r * 3 + 2] = b3[r];
  }
  if (j == 0)
    for (int k = 0; k < 10; ++k) a.betas[(size_t)f * 10 + k] = a.rd[(size_t)f * a.ldrd + 18 + k] + a.init_betas[k];
}

// token_out (the decoder's f32 residual stream) -> vit rows of the frame store
__global__ void copy_rows_kernel(const float* __restrict__ x, long ldx, float* __restrict__ y, long ldy, int rows,
                                 int D) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (long)rows * D) y[(i / D) * ldy + i % D] = x[(i / D) * ldx + i % D];
}

}  // namespace

// ================================================================================== host launchers
namespace vge {

// The epilogues the GEMM kernels are instantiated for.  with_epi hands the runtime id to f as a compile-time constant,
// f(EpiC<EPI>{}); the launchers and the dynamic-LDS setup all go through it (an id outside the list runs as GEMM_F32).
template <int E>
using EpiC = std::integral_constant<int, E>;
constexpr int GEMM_EPIS[] = {GEMM_BF16, GEMM_GELU_BF16, GEMM_RES_F32,   GEMM_PE_F32,
                             GEMM_F32,  GEMM_RELU_BF16, GEMM_RESB_BF16, GEMM_RESB_RELU_BF16};
template <class F>
void with_epi(int epi, F&& f) {
  switch (epi) {
    case GEMM_BF16: return f(EpiC<GEMM_BF16>{});
    case GEMM_GELU_BF16: return f(EpiC<GEMM_GELU_BF16>{});
    case GEMM_RES_F32: return f(EpiC<GEMM_RES_F32>{});
    case GEMM_PE_F32: return f(EpiC<GEMM_PE_F32>{});
    case GEMM_RELU_BF16: return f(EpiC<GEMM_RELU_BF16>{});
    case GEMM_RESB_BF16: return f(EpiC<GEMM_RESB_BF16>{});
    case GEMM_RESB_RELU_BF16: return f(EpiC<GEMM_RESB_RELU_BF16>{});
    default: return f(EpiC<GEMM_F32>{});
  }
}
template <int EPI>
constexpr bool GEMMP_EPI = EPI == GEMM_BF16 || EPI == GEMM_GELU_BF16 || EPI == GEMM_RELU_BF16;  // gemmp_bf16_kernel's

// the dynamic-LDS limit of kernel_of(EpiC<EPI>{}) for every epilogue (null = no such instantiation)
template <class K>
hipError_t gemm_lds_setup(int bytes, K kernel_of) {
  hipError_t e = hipSuccess;
  for (const int epi : GEMM_EPIS)
    with_epi(epi, [&](auto E) {
      const void* k = kernel_of(E);
      if (k && e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    });
  return e;
}
template <int NW, int SH = 0, bool PM = false>
hipError_t gemm_setup() {
  return gemm_lds_setup(GB_LDS, [](auto E) { return (const void*)gemm_bf16_kernel<decltype(E)::value, NW, SH, PM>; });
}
template <bool PM>
hipError_t gemm2_setup() {
  return gemm_lds_setup(G2_LDS, [](auto E) { return (const void*)gemm2_bf16_kernel<decltype(E)::value, PM>; });
}
template <bool PM>
hipError_t gemmp_setup() {
  return gemm_lds_setup(GB_LDS, [](auto E) -> const void* {
    if constexpr (GEMMP_EPI<decltype(E)::value>) return (const void*)gemmp_bf16_kernel<decltype(E)::value, PM>;
    return nullptr;
  });
}

hipError_t vit_kernels_setup_dev();

// the dynamic-LDS attributes of every GEMM / attention kernel of this file, once per device (any launch path may be the
// first on a device: the extractors' create calls, the conv tuner's GEMM candidate, the op-level test hooks)
hipError_t vit_kernels_setup() {
  static std::atomic<unsigned long long> done{0};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const unsigned long long bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
  e = vit_kernels_setup_dev();
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
  return e;
}

hipError_t vit_kernels_setup_dev() {
  hipError_t e = gemm_setup<8>();
  if (e == hipSuccess) e = gemm2_setup<false>();
  if (e == hipSuccess) e = gemm2_setup<true>();
  if (e == hipSuccess) e = gemm_setup<8, 0, true>();  // the partial-M kernels (8 waves): 1x1 convs over n x H x W rows
  if (e == hipSuccess) e = gemm_setup<8, 1, true>();
  if (e == hipSuccess) e = gemm_setup<4>();
  if (e == hipSuccess) e = gemm_setup<8, 1>();
  if (e == hipSuccess) e = gemmp_setup<false>();
  if (e == hipSuccess) e = gemmp_setup<true>();
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)vit_attn_kernel<80>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          AttnCfg<80>::LDS);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute((const void*)vit_attn_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             AttnCfg<64>::LDS);
}

// VGE_GEMM_WAVES, read once: 1 (default) = by epilogue: the bf16-output epilogues (bias, GELU, the 1x1 convs' ReLU /
// residual) on the 16x16x32 form of the 8-wave kernel, the f32-output ones on 32x32x16 (the 16x16x32 form is
// bit-identical and the chip holds a higher clock on it: qkv +4-8 %, fc1 +2-3 %; proj / fc2 with their f32 residual
// 0-3 % slower: profiles/ab_r05p_gemm_ablation.json, ab_r05q_gemm2.json); 8 / 16 = always 32x32x16 / 16x16x32;
// 4 = 4 waves of 128 x 128; 2 = gemm2
static int g_gemm_waves = 0;

template <int NW, int SH = 0, bool PM = false>
void launch_gemm_nw(int epi, dim3 grid, const GemmBf16Args& g, hipStream_t s) {
  with_epi(epi, [&](auto E) {
    hipLaunchKernelGGL((gemm_bf16_kernel<decltype(E)::value, NW, SH, PM>), grid, dim3(64 * NW), GB_LDS, s, g);
  });
}

template <bool PM>
void launch_gemm2(int epi, const GemmBf16Args& g, hipStream_t s) {
  const dim3 grid(((g.M + G2_M - 1) / G2_M) * (g.N / G2_N));
  with_epi(epi, [&](auto E) {
    hipLaunchKernelGGL((gemm2_bf16_kernel<decltype(E)::value, PM>), grid, dim3(256), G2_LDS, s, g);
  });
}

// shapes are validated by the callers (vge_hmr.cpp, vge_cnn.hip): N % 256 == K % 64 == 0, 16-B aligned rows; any M
// VGE_GEMMP, read once: 1 = the residual-free bf16 epilogues run on the persistent kernel (gemmp_bf16_kernel) whenever
// it applies (gemm_persist_ok); 0 (default) = only where a caller asks for it (the conv tuner's variant 10)
static int g_gemm_persist = -1;

static int device_cus() {
  const int c = device_cu_count();
  return c > 0 ? c : 256;
}

// the persistent kernel's conditions: a residual-free bf16 epilogue with a bias, K / 32 >= 6, more tiles than CUs (one
// workgroup per CU, a multiple of 8 of them), a tile's stores inside a 32-bit buffer range
bool gemm_persist_ok(int epi, const GemmBf16& a) {
  if ((epi != GEMM_BF16 && epi != GEMM_GELU_BF16 && epi != GEMM_RELU_BF16) || !a.bias || a.K / GB_K < 6 || a.N % GB_N ||
      a.K % 64 || a.M < 1)
    return false;
  const long ntiles = (long)((a.M + GB_M - 1) / GB_M) * (a.N / GB_N);
  return ntiles > device_cus() && (long)GB_M * a.ldo * 2 < (1L << 31);
}

static GemmBf16Args to_args(const GemmBf16& a) {
  GemmBf16Args g;
  g.A = reinterpret_cast<const bf16*>(a.A);
  g.W = reinterpret_cast<const bf16*>(a.W);
  g.out = a.out;
  g.bias = a.bias;
  g.res = a.res;
  g.pos = a.pos;
  g.lda = a.lda; g.ldw = a.ldw; g.ldo = a.ldo; g.ldr = a.ldr;
  g.M = a.M; g.N = a.N; g.K = a.K; g.tokens = a.tokens;
  g.resb = reinterpret_cast<const bf16*>(a.resb);
  return g;
}

hipError_t launch_gemm_bf16_persistent(int epi, const GemmBf16& a, hipStream_t s) {
  if (!gemm_persist_ok(epi, a)) return hipErrorInvalidValue;
  if (const hipError_t e = vit_kernels_setup(); e != hipSuccess) return e;
  const GemmBf16Args g = to_args(a);
  const dim3 grid(device_cus() & ~7);  // one workgroup per CU, a multiple of 8 (the XCD-grouped tile walk)
  const bool pm = g.M % GB_M != 0;
  with_epi(epi, [&](auto E) {
    constexpr int EPI = decltype(E)::value;
    if constexpr (GEMMP_EPI<EPI>) {  // (gemm_persist_ok: no other id comes here)
      if (pm)
        hipLaunchKernelGGL((gemmp_bf16_kernel<EPI, true>), grid, dim3(512), GB_LDS, s, g);
      else
        hipLaunchKernelGGL((gemmp_bf16_kernel<EPI, false>), grid, dim3(512), GB_LDS, s, g);
    }
  });
  return hipGetLastError();
}

hipError_t launch_gemm_bf16(int epi, const GemmBf16& a, hipStream_t s) {
  if (g_gemm_persist < 0) {
    const char* e = getenv("VGE_GEMMP");
    g_gemm_persist = (e && e[0] == '1') ? 1 : 0;
  }
  if (g_gemm_persist == 1 && gemm_persist_ok(epi, a)) return launch_gemm_bf16_persistent(epi, a, s);
  const GemmBf16Args g = to_args(a);
  const bool rb = epi == GEMM_RESB_BF16 || epi == GEMM_RESB_RELU_BF16;
  if (a.M < 1 || a.N % GB_N || a.K % 64 || (rb && !a.resb) || (epi == GEMM_PE_F32 && a.tokens != AT_T))
    return hipErrorInvalidValue;
  if (const hipError_t e = vit_kernels_setup(); e != hipSuccess) return e;
  if (g_gemm_waves == 0) {
    const char* e = getenv("VGE_GEMM_WAVES");
    g_gemm_waves = (e && (atoi(e) == 2 || atoi(e) == 4 || atoi(e) == 8 || atoi(e) == 16)) ? atoi(e) : 1;
  }
  if (g_gemm_waves == 2) {  // two 128 x 256 workgroups per CU
    if (a.M % G2_M)
      launch_gemm2<true>(epi, g, s);
    else
      launch_gemm2<false>(epi, g, s);
    return hipGetLastError();
  }
  const dim3 grid(((a.M + GB_M - 1) / GB_M) * (a.N / GB_N));
  const bool sh = g_gemm_waves == 16 || (g_gemm_waves == 1 && epi != GEMM_RES_F32 && epi != GEMM_PE_F32 && epi != GEMM_F32);
  if (a.M % GB_M) {
    if (sh)
      launch_gemm_nw<8, 1, true>(epi, grid, g, s);
    else
      launch_gemm_nw<8, 0, true>(epi, grid, g, s);
  } else if (g_gemm_waves == 4)
    launch_gemm_nw<4>(epi, grid, g, s);
  else if (sh)
    launch_gemm_nw<8, 1>(epi, grid, g, s);
  else
    launch_gemm_nw<8>(epi, grid, g, s);
  return hipGetLastError();
}

extern "C" int vge_debug_set_gemm_persist(int on) {  // tests / A/B: the persistent kernel wherever it applies (1) or not
  g_gemm_persist = on ? 1 : 0;
  return 0;
}

extern "C" int vge_debug_set_gemm_waves(int nw) {  // A/B timing (tools/gemm_bench.py)
  g_gemm_waves = (nw == 1 || nw == 2 || nw == 4 || nw == 16) ? nw : 8;
  return 0;
}

hipError_t launch_ln_bf16(const float* x, long ldx, void* y, long ldy, const float* w, const float* b, int rows, int D,
                          float eps, hipStream_t s) {
  const dim3 grid((rows + 3) / 4);
  bf16* yy = reinterpret_cast<bf16*>(y);
  switch (D) {
    case 256: hipLaunchKernelGGL(ln_bf16_kernel<1>, grid, dim3(256), 0, s, x, ldx, yy, ldy, w, b, rows, eps); break;
    case 512: hipLaunchKernelGGL(ln_bf16_kernel<2>, grid, dim3(256), 0, s, x, ldx, yy, ldy, w, b, rows, eps); break;
    case 768: hipLaunchKernelGGL(ln_bf16_kernel<3>, grid, dim3(256), 0, s, x, ldx, yy, ldy, w, b, rows, eps); break;
    case 1024: hipLaunchKernelGGL(ln_bf16_kernel<4>, grid, dim3(256), 0, s, x, ldx, yy, ldy, w, b, rows, eps); break;
    case 1280: hipLaunchKernelGGL(ln_bf16_kernel<5>, grid, dim3(256), 0, s, x, ldx, yy, ldy, w, b, rows, eps); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_cast_bf16(const float* x, long ldx, void* y, long ldy, int rows, int D, hipStream_t s) {
  const long n = (long)rows * (D / 4);
  hipLaunchKernelGGL(cast_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, ldx,
                     reinterpret_cast<bf16*>(y), ldy, rows, D);
  return hipGetLastError();
}

hipError_t launch_bcast_rows(const float* vec, float* y, int rows, int D, hipStream_t s) {
  const long n = (long)rows * D;
  hipLaunchKernelGGL(bcast_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, vec, y, rows, D);
  return hipGetLastError();
}

hipError_t launch_patchify(const uint8_t* frames, int F, int in_h, int in_w, int x0, int img_h, int img_w, int P,
                           int pad, int gh, int gw, const float* mean, const float* stdv, void* out, hipStream_t s) {
  PatchArgs a;
  a.frames = frames; a.out = reinterpret_cast<bf16*>(out);
  a.F = F; a.in_h = in_h; a.in_w = in_w; a.x0 = x0; a.img_h = img_h; a.img_w = img_w; a.P = P; a.pad = pad;
  a.gh = gh; a.gw = gw;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.stdv[c] = stdv[c]; }
  const long n = (long)F * gh * gw * (3 * P * P / 8);
  hipLaunchKernelGGL(patchify_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_vit_attn(const void* qkv, long ldq, void* out, long ldo, int F, int D, int heads, int hd,
                           hipStream_t s) {
  const float scale_log2 = 1.4426950408889634f / sqrtf((float)hd);
  const bf16* q = reinterpret_cast<const bf16*>(qkv);
  bf16* o = reinterpret_cast<bf16*>(out);
  if (hd == 80)
    hipLaunchKernelGGL(vit_attn_kernel<80>, dim3(F * heads), dim3(384), AttnCfg<80>::LDS, s, q, ldq, o, ldo, D, heads,
                       scale_log2);
  else if (hd == 64)
    hipLaunchKernelGGL(vit_attn_kernel<64>, dim3(F * heads), dim3(384), AttnCfg<64>::LDS, s, q, ldq, o, ldo, D, heads,
                       scale_log2);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_xattn1(const void* q, long ldq, const void* kv, long ldkv, void* out, long ldo, int F, int inner,
                         int heads, int ctx, hipStream_t s) {
  if (ctx < 1 || ctx > 256) return hipErrorInvalidValue;  // the kernel's score buffer: __shared__ float p[256]
  hipLaunchKernelGGL(xattn1_kernel, dim3(F * heads), dim3(64), 0, s, reinterpret_cast<const bf16*>(q), ldq,
                     reinterpret_cast<const bf16*>(kv), ldkv, reinterpret_cast<bf16*>(out), ldo, inner, heads, ctx,
                     0.125f);
  return hipGetLastError();
}

hipError_t launch_softmax_rows(const float* x, void* y, int rows, int C, hipStream_t s) {
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, reinterpret_cast<bf16*>(y), rows,
                     C);
  return hipGetLastError();
}

hipError_t launch_readout(const float* rd, int ldrd, const float* bp, int ldbp, const float* init_pose,
                          const float* init_betas, float* pose, float* gori, float* betas, int F, hipStream_t s) {
  ReadoutArgs a{rd, bp, init_pose, init_betas, pose, gori, betas, F, ldrd, ldbp};
  hipLaunchKernelGGL(readout_kernel, dim3((F * 24 + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_copy_rows(const float* x, long ldx, float* y, long ldy, int rows, int D, hipStream_t s) {
  const long n = (long)rows * D;
  hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, ldx, y, ldy, rows, D);
  return hipGetLastError();
}

}  // namespace vge
