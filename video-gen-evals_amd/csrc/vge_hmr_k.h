// Launchers of the TokenHMR extractor's kernels (vge_vit.hip, vge_hmr_front.hip) as vge_hmr.cpp calls them; the bf16
// GEMM is in vge_gemm.h.  bf16 buffers travel as void*.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vge {

// the dynamic-LDS attributes of every GEMM / attention kernel of vge_vit.hip, once per device
hipError_t vit_kernels_setup();

// vge_hmr_front.hip: ViTDetDataset's person crops of uint8 frames
hipError_t launch_hmr_crop(const uint8_t* frames, int H, int W, const float* boxes, const int* frame_of, int n,
                           uint8_t* out, hipStream_t s);

// vge_vit.hip
hipError_t launch_ln_bf16(const float* x, long ldx, void* y, long ldy, const float* w, const float* b, int rows, int D,
                          float eps, hipStream_t s);
hipError_t launch_cast_bf16(const float* x, long ldx, void* y, long ldy, int rows, int D, hipStream_t s);
hipError_t launch_bcast_rows(const float* vec, float* y, int rows, int D, hipStream_t s);
hipError_t launch_patchify(const uint8_t* frames, int F, int in_h, int in_w, int x0, int img_h, int img_w, int P,
                           int pad, int gh, int gw, const float* mean, const float* stdv, void* out, hipStream_t s);
hipError_t launch_vit_attn(const void* qkv, long ldq, void* out, long ldo, int F, int D, int heads, int hd,
                           hipStream_t s);
hipError_t launch_xattn1(const void* q, long ldq, const void* kv, long ldkv, void* out, long ldo, int F, int inner,
                         int heads, int ctx, hipStream_t s);
hipError_t launch_softmax_rows(const float* x, void* y, int rows, int C, hipStream_t s);
hipError_t launch_readout(const float* rd, int ldrd, const float* bp, int ldbp, const float* init_pose,
                          const float* init_betas, float* pose, float* gori, float* betas, int F, hipStream_t s);
hipError_t launch_copy_rows(const float* x, long ldx, float* y, long ldy, int rows, int D, hipStream_t s);

}  // namespace vge
