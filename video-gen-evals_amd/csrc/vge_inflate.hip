// Device inflate for the feature front end (include/vge_ingest.h): raw .npz / .npy bytes in device memory -> the rows
// of the device frame store, with no decoded floats staged on the host.
//
// One wave (one 64-thread workgroup) owns one stream -- one array of one video -- and inflates it with the shared core
// (vge_inflate_core.h: the LDS history ring, the staged bit reader, the code tables, the batch decode and copy stages).
// What is this file's own:
//   history   the ring is indexed by the uncompressed position, npy header included: matches that reach into the
//             header (numpy's space padding is coded as matches; a payload can repeat header bytes) read it there,
//             and only positions at or beyond `skip` are ever written to the destination.
//   output    whole dwords (float32: the rows; float64: the workspace, converted by a second kernel).
// Bounds: every descriptor is checked against the buffer sizes and row counts the host passed; the reader never leaves
// [src, src + csize) (bytes beyond read as zero and the bit position is checked after every symbol); stores stay below
// `count` elements; every loop consumes at least one input bit or produces at least one byte.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vge_ingest.h"
#include "vge_error.h"
#include "vge_inflate_core.h"

namespace {

using namespace vge_inflate;
using vge::set_last_error;

constexpr int ERR_HIP = 2;

struct Args {
  const uint8_t* data;
  int64_t data_bytes;
  const vge_inflate_desc* descs;
  int64_t n_rows, kp_rows;
  float* arr[5];
  uint8_t* ws;
  int64_t ws_bytes;
  int32_t* status;
  int32_t n_descs, n_videos, vit_dim;
};

__device__ inline int array_width(int a, int vit_dim) { return a == 0 ? 207 : a == 1 ? 9 : a == 2 ? 10 : a == 3 ? vit_dim : 120; }

// 0: run it; -1: an unused slot; else the status code of a descriptor that does not fit what the host passed.
__device__ int check_desc(const Args& A, const vge_inflate_desc& d) {
  if (d.array < 0) return -1;
  if (d.array > 4 || d.video < 0 || d.video >= A.n_videos) return -1;  // nobody to report to
  if ((d.method != 0 && d.method != 8) || (d.itemsize != 4 && d.itemsize != 8) || d.skip < 0 || d.count < 0 ||
      d.csize < 0 || d.csize >= (1ll << 28) || d.src_off < 0 || d.src_off > A.data_bytes ||
      d.csize > A.data_bytes - d.src_off || d.dst_off < 0)
    return VGE_INGEST_ERR_ARG;
  const int64_t cap = (d.array == 4 ? A.kp_rows : A.n_rows) * (int64_t)array_width(d.array, A.vit_dim);
  if (d.dst_off > cap || d.count > cap - d.dst_off || A.arr[d.array] == nullptr) return VGE_INGEST_ERR_ARG;
  if (d.itemsize == 8 && (d.ws_off < 0 || (d.ws_off & 7) || d.ws_off > A.ws_bytes || d.count > (A.ws_bytes - d.ws_off) / 8))
    return VGE_INGEST_ERR_ARG;
  return 0;
}

__device__ inline void fail(const Args& A, int video, int code) {
  if (threadIdx.x == 0) atomicCAS(&A.status[video], 0, code);
}

__global__ __launch_bounds__(WAVE) void inflate_kernel(Args A) {
  __shared__ Shared S;
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_inflate_desc d = A.descs[blockIdx.x];
  const int chk = check_desc(A, d);
  if (chk < 0) return;
  if (chk > 0) return fail(A, d.video, chk);
  if (uni((uint32_t)A.status[d.video]) != 0) return;  // a sibling stream has failed already: the video is lost
  const int lane = threadIdx.x;
  const uint8_t* src = A.data + d.src_off;
  const int64_t skip = d.skip, total = skip + d.count * d.itemsize;
  uint32_t* dst = d.itemsize == 4 ? reinterpret_cast<uint32_t*>(A.arr[d.array] + d.dst_off)
                                  : reinterpret_cast<uint32_t*>(A.ws + d.ws_off);
  const int64_t n_dw = (total - skip) >> 2;

  if (d.method == 0) {  // stored member / plain .npy: the copy path
    if (total > d.csize) return fail(A, d.video, VGE_INGEST_ERR_IO);
    for (int64_t k = lane; k < n_dw; k += WAVE) dst[k] = load32(src, skip + 4 * k);
    return;
  }

  Reader R;
  R.src = src;
  R.csize = (int32_t)d.csize;
  R.bp = 0;
  R.cached = false;
  R.cbit = 0;
  R.cache = 0;
  int64_t flushed;
  if (inflate_stream<false>(R, S, DwordSink{dst, skip}, total, &flushed) == STREAM_FAIL)
    return fail(A, d.video, VGE_INGEST_ERR_IO);
}

// float64 streams: workspace -> rows, with the host's (float) rounding.
__global__ __launch_bounds__(256) void convert_kernel(Args A) {
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_inflate_desc d = A.descs[blockIdx.x];
  if (check_desc(A, d) != 0 || d.itemsize != 8 || A.status[d.video] != 0) return;
  const double* in = reinterpret_cast<const double*>(A.ws + d.ws_off);
  float* out = A.arr[d.array] + d.dst_off;
  for (int64_t i = threadIdx.x; i < d.count; i += 256) out[i] = (float)in[i];
}

}  // namespace

extern "C" int vge_ingest_decode_device_batch_symbols(void) { return WAVE; }
extern "C" int vge_ingest_decode_device_ring_bytes(void) { return RING; }
extern "C" int vge_ingest_decode_device_stage_bytes(void) { return STAGE; }

extern "C" size_t vge_ingest_decode_device_workspace_bytes(const vge_inflate_desc* descs, int n_descs) {
  int64_t ws = 0;
  if (descs)
    for (int k = 0; k < n_descs; ++k)
      if (descs[k].array >= 0 && descs[k].itemsize == 8 && descs[k].count > 0) ws += descs[k].count * 8;
  return (size_t)(ws > 8 ? ws : 8);
}

extern "C" int vge_ingest_decode_device(const uint8_t* data, int64_t data_bytes, const vge_inflate_desc* descs,
                                        int n_descs, int n_videos, int64_t n_rows, int64_t kp_rows, int vit_dim,
                                        float* pose, float* gori, float* betas, float* vit, float* kp, void* workspace,
                                        int64_t workspace_bytes, int32_t* status, void* stream) {
  if (n_descs < 0 || n_videos < 0 || data_bytes < 0 || n_rows < 0 || kp_rows < 0 || vit_dim < 1 ||
      workspace_bytes < 0) {
    set_last_error("vge_ingest_decode_device: bad argument (negative count or size)");
    return VGE_INGEST_ERR_ARG;
  }
  if (n_videos == 0 || n_descs == 0) return VGE_INGEST_OK;
  if (!data || !descs || !status || !workspace || !pose || !gori || !betas || !vit || ((uintptr_t)descs & 7) ||
      ((uintptr_t)workspace & 7) || ((uintptr_t)status & 3) || ((uintptr_t)pose & 3) || ((uintptr_t)gori & 3) ||
      ((uintptr_t)betas & 3) || ((uintptr_t)vit & 3) || ((uintptr_t)kp & 3)) {
    set_last_error("vge_ingest_decode_device: bad argument (null or misaligned buffer)");
    return VGE_INGEST_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, (size_t)n_videos * 4, s) != hipSuccess) {
    set_last_error(std::string("vge_ingest_decode_device: ") + hipGetErrorString(hipGetLastError()));
    return ERR_HIP;
  }
  Args A;
  A.data = data;
  A.data_bytes = data_bytes;
  A.descs = descs;
  A.n_rows = n_rows;
  A.kp_rows = kp_rows;
  A.arr[0] = pose;
  A.arr[1] = gori;
  A.arr[2] = betas;
  A.arr[3] = vit;
  A.arr[4] = kp;
  A.ws = static_cast<uint8_t*>(workspace);
  A.ws_bytes = workspace_bytes;
  A.status = status;
  A.n_descs = n_descs;
  A.n_videos = n_videos;
  A.vit_dim = vit_dim;
  hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  hipLaunchKernelGGL(convert_kernel, dim3((unsigned)n_descs), dim3(256), 0, s, A);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error(std::string("vge_ingest_decode_device: ") + hipGetErrorString(e));
    return ERR_HIP;
  }
  return VGE_INGEST_OK;
}
