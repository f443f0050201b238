// Shared device pieces of the bf16 matrix-core kernels: gemm_bf16_kernel / gemmp_bf16_kernel / gemm2_bf16_kernel
// (vge_vit.hip) and conv_bf16_kernel / conv2_bf16_kernel / conv2p_bf16_kernel (vge_cnn.hip).  Device only, everything
// inlined.  Here: the vector typedefs, the grouped panel walk, the swizzled LDS stage of dense 64-B rows, the
// sched_group_barrier interleave, the quad transpose, the small epilogue conversions and the LDS ordering point.
// (xcd_remap: vge_common.h.)  Each kernel keeps what differs -- ring depth and slot layout, its vmcnt accounting,
// gathered or dense A staging, persistent or one-tile control flow, its epilogue policy -- and, still, its own fragment
// reads, MFMA loops and C-layout spill (DESIGN 3.7 says why a wave-tile type is not here yet).
//
// LDS image of a stage (both operands): 64-B rows (32 k), 16 rows per 1-KB wave instruction, lane L -> row L / 4,
// physical 16-B chunk L % 4.  Physical chunk p of row r holds logical chunk p ^ ((r >> 2) & 3): the SOURCE address is
// pre-swizzled, the LDS image stays lane-linear (global_load_lds), and the 16 rows a ds_read_b128 lane group reads land
// on 16 distinct 16-B slots.
#pragma once
#include "vge_common.h"

typedef __bf16 bf16;
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned uintx2_t __attribute__((ext_vector_type(2)));
typedef unsigned uintx4_t __attribute__((ext_vector_type(4)));

// Tile id -> (row panel mt, column panel nt): groups of GM row panels walk the ntn column panels with the row panel
// fastest, so the ~32 consecutive ids an XCD runs at once (xcd_remap) cover ~8 row panels x ~4 column panels and read
// the same K slices at about the same time (L2 hits instead of fabric re-fetches).  mtn = row panels in all.
template <int GM>
__device__ __forceinline__ void panel_tile(int bid, int ntn, int mtn, int& mt, int& nt) {
  const int grp = bid / (GM * ntn), rem = bid - grp * (GM * ntn);
  const int gm = min(GM, mtn - grp * GM);
  mt = rem % gm + grp * GM;
  nt = rem / gm;
}

// Stage a ROWS x 32-k tile of the dense row-major operand X (rows r0.., k0..) with NW waves: wave instruction q fills
// LDS bytes [1024 q, 1024 q + 1024) = rows 16 q .. 16 q + 15.  CLAMP: rows past rmax re-read row rmax (a partial last
// row tile).
template <int ROWS, int NW, bool CLAMP>
__device__ __forceinline__ void stage_rows(const bf16* __restrict__ X, long ld, int r0, int k0, char* tile, int wave,
                                           int lane, int rmax) {
  constexpr int PW = ROWS / 16 / NW;  // wave instructions per wave
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    const int q = wave * PW + j;
    const int row = 16 * q + (lane >> 2);
    const int ch = (lane & 3) ^ ((row >> 2) & 3);
    glds16(X + (size_t)(CLAMP ? min(r0 + row, rmax) : r0 + row) * ld + k0 + ch * 8, tile + q * 1024);
  }
}

// The issue order of one pipeline step, handed to the scheduler: NV groups of (MV MFMAs, one global_load_lds), then
// ND groups of (MD MFMAs, NDS LDS fragment reads, NVALU VALU ops), so loads and LDS reads issue between MFMAs instead
// of in a burst in front of them
template <int NV, int MV, int ND, int MD, int NDS, int NVALU = 0>
__device__ __forceinline__ void mfma_interleave() {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    __builtin_amdgcn_sched_group_barrier(0x008, MV, 0);  // MFMA
    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read (global_load_lds)
  }
#pragma unroll
  for (int j = 0; j < ND; ++j) {
    __builtin_amdgcn_sched_group_barrier(0x008, MD, 0);   // MFMA
    __builtin_amdgcn_sched_group_barrier(0x100, NDS, 0);  // DS read
    if constexpr (NVALU > 0) __builtin_amdgcn_sched_group_barrier(0x002, NVALU, 0);  // VALU
  }
}

// Compiler-only ordering point for LDS traffic that crosses lanes inside one wave.  The hardware runs a wave's LDS
// instructions in order, but the compiler keeps only the order of accesses that may alias within ONE lane, and a
// transpose through LDS writes a row from some lanes and reads it from others: without this between the writes and the
// reads (and before the next round's writes) hipcc may sink a ds_write below the ds_read of the same bytes.  Emits no
// instruction.
__device__ __forceinline__ void wave_lds_order() { asm volatile("" ::: "memory"); }

template <int CTRL>
__device__ __forceinline__ float quad_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// 4x4 transpose inside each quad of lanes (o1 = lane & 1, o2 = lane & 2): on entry lane i holds column i of rows 0..3
// (v0..v3), on exit row i, columns 0..3
__device__ __forceinline__ void quad_t4(float& v0, float& v1, float& v2, float& v3, bool o1, bool o2) {
  float x = o1 ? v0 : v1, y = quad_dpp<0xB1>(x);  // quad_perm [1,0,3,2]
  v0 = o1 ? y : v0;
  v1 = o1 ? v1 : y;
  x = o1 ? v2 : v3;
  y = quad_dpp<0xB1>(x);
  v2 = o1 ? y : v2;
  v3 = o1 ? v3 : y;
  x = o2 ? v0 : v2;
  y = quad_dpp<0x4E>(x);  // quad_perm [2,3,0,1]
  v0 = o2 ? y : v0;
  v2 = o2 ? v2 : y;
  x = o2 ? v1 : v3;
  y = quad_dpp<0x4E>(x);
  v1 = o2 ? y : v1;
  v3 = o2 ? v3 : y;
}
__device__ __forceinline__ floatx4 quad_t4(floatx4 v, bool o1, bool o2) {
  float v0 = v.x, v1 = v.y, v2 = v.z, v3 = v.w;
  quad_t4(v0, v1, v2, v3, o1, o2);
  return floatx4{v0, v1, v2, v3};
}

// ---- epilogue conversions
__device__ __forceinline__ bf16x4 to_bf16x4(floatx4 v) { return bf16x4{(bf16)v.x, (bf16)v.y, (bf16)v.z, (bf16)v.w}; }
__device__ __forceinline__ floatx4 to_floatx4(bf16x4 r) { return floatx4{(float)r[0], (float)r[1], (float)r[2], (float)r[3]}; }
__device__ __forceinline__ floatx4 relu4(floatx4 v) {
  return floatx4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
}
