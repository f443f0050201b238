/* vge_ingest.h -- on-disk feature ingest for the AC/TC scoring path.
 *
 * C ABI without HIP types (host code, except the device inflate at the end of this file), exported by libvge.so.
 * Replaces the reference's per-video readers:
 *   np.load(<video>.npz) -> pose [T,23,3,3], global_orient [T,1,3,3], betas [T,10], vit [T,Dv]
 *                                               (utils.py:383-409 WindowDataset._try_one; the npz is
 *                                                extract_mesh.py:35-43's np.savez_compressed output)
 *   np.load(<kp_dir>/.../keypoints.npy) -> [T',120]        (utils.py:410-424)
 * as a multithreaded native decoder: the zip central directory is parsed (zip64 included), each member
 * is raw-deflate inflated (zlib) straight into caller-provided -- typically pinned -- host buffers at
 * the frame-store offsets the GPU path uses (vge.data.FrameStore / vge_frame_store), with no Python
 * objects or intermediate copies per array.  float64 members are converted to float32 (the reference
 * feeds float32 tensors to the model).
 *
 * Two calls per set of videos:
 *   vge_ingest_probe  -- shapes from the npy headers only (inflates the first few hundred bytes of
 *                        two members per file); the caller lays out the frame store from them
 *   vge_ingest_decode -- full decode into the laid-out buffers
 * Per-video failures are reported per video (status[i]), so the Python driver can mirror the
 * reference's error behaviour: an unreadable npz is skipped with a message (eval.py:93-95), a missing
 * keypoint file raises in the scoring path (utils.py:416-417) and is tolerated for the stats
 * (utils.py:669-678).
 */
#ifndef VGE_INGEST_H
#define VGE_INGEST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-video status codes (also the return value of the calls: VGE_OK or the first failure) */
enum {
  VGE_INGEST_OK = 0,
  VGE_INGEST_ERR_ARG = 1,         /* bad argument */
  VGE_INGEST_ERR_IO = 7,          /* npz unreadable / malformed (not a zip, missing member, bad npy) */
  VGE_INGEST_ERR_SHAPE = 8,       /* a member's shape disagrees with the layout (pose/gori/betas/vit T, dims) */
  VGE_INGEST_ERR_KP = 9           /* keypoints.npy present but unreadable / not [T',120] */
};

typedef struct {
  int32_t n_frames;  /* pose.shape[0] */
  int32_t vit_dim;   /* vit.shape[1] */
  int32_t kp_frames; /* keypoints.npy rows; -1 when kp_paths[i] is NULL or the file does not exist */
  int32_t status;    /* VGE_INGEST_OK or an error code above */
} vge_clip_info;

/* npz_paths[n]; kp_paths[n] (entries may be NULL; kp_paths itself may be NULL).  n_threads <= 0:
 * vge_ingest_default_threads().  Fills info[n]; returns VGE_INGEST_OK if every video probed cleanly, else the
 * first failing video's code (the others are still probed). */
/* Thread count the calls use when n_threads <= 0: VGE_INGEST_THREADS, else OMP_NUM_THREADS if > 1, else
 * the process's CPU share (cgroup quota / affinity mask) divided by LOCAL_WORLD_SIZE; at most 64. */
int vge_ingest_default_threads(void);

int vge_ingest_probe(const char* const* npz_paths, const char* const* kp_paths, int n, int n_threads,
                     vge_clip_info* info);

/* Decode video i into rows [videos[4i], videos[4i] + videos[4i+1]) of pose [*,207], gori [*,9],
 * betas [*,10], vit [*,vit_dim] and, when videos[4i+3] > 0, rows [videos[4i+2], +videos[4i+3]) of
 * kp [*,120].  videos[4i+1] must equal the file's T (and videos[4i+3] its T').  status[n] (may be NULL)
 * receives the per-video codes. */
int vge_ingest_decode(const char* const* npz_paths, const char* const* kp_paths, int n, int n_threads,
                      const int32_t* videos, int vit_dim, float* pose, float* gori, float* betas, float* vit,
                      float* kp, int32_t* status);

/* ---- Files held in memory: the probe's and the decoder's twins for a packed buffer.
 *
 * File j is sizes[j] bytes at data + offsets[j] of a buffer of data_bytes bytes (the contract of vge_frames.h's _mem
 * calls; vge_jpeg_file_sizes / vge_jpeg_read_files fill such a buffer).  Video i owns two entries: 2i its npz, 2i + 1
 * its keypoints.npy, with sizes[2i + 1] < 0 for a keypoint file that does not exist (kp_frames -1, as for a NULL or
 * absent path).  Files may be packed with gaps and in any order.  A video with an entry that has a negative offset, an
 * npz of negative size, or a file that does not lie inside [0, data_bytes) gets VGE_INGEST_ERR_ARG and none of its
 * bytes is read; an empty file is unreadable, as an empty file on disk is (_ERR_IO for the npz, _ERR_KP for the
 * keypoints).  Everything else is vge_ingest_probe's and vge_ingest_decode's contract, to the bit: the path calls map
 * the files and run the same code. */
int vge_ingest_probe_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                         int n_threads, vge_clip_info* info);
int vge_ingest_decode_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                          int n_threads, const int32_t* videos, int vit_dim, float* pose, float* gori, float* betas,
                          float* vit, float* kp, int32_t* status);

/* ---- Device inflate (csrc/vge_inflate.hip): the same files in device memory -> the frame store in device memory.
 *
 * One stream is one array of one video: a zip member (pose, global_orient, betas, vit) or the keypoint file.  Plain
 * data, copied to the device as bytes. */
typedef struct {
  int64_t src_off;   /* the stream's first byte inside the buffer (compressed bytes / the npy file's first byte) */
  int64_t csize;     /* bytes of it */
  int64_t count;     /* elements to produce */
  int64_t dst_off;   /* element offset inside the destination array */
  int64_t ws_off;    /* itemsize 8: byte offset of the stream's count * 8 bytes inside the workspace; else -1 */
  int32_t method;    /* 0 stored, 8 deflate */
  int32_t skip;      /* uncompressed bytes before the first element (the npy header) */
  int32_t itemsize;  /* 4 (float32) or 8 (float64, converted) */
  int32_t array;     /* 0 pose, 1 gori, 2 betas, 3 vit, 4 kp; -1: an unused slot */
  int32_t video;     /* owner: index into status[] */
  int32_t reserved;
} vge_inflate_desc;

/* Host: parse the central directories and inflate the four npy headers only, parse the keypoint header, check shapes
 * and counts against videos[n,4] (vge_ingest_decode's table) with vge_ingest_decode's codes, and fill info[n] as the
 * probe does plus descs[5n]: video i's streams in slots 5i .. 5i + 4 in the order of `array` above.  A video that fails
 * gets no streams (all five slots unused) and its status is final; a video without keypoints (videos[4i + 3] == 0)
 * leaves slot 5i + 4 unused.  A stream of 2^28 compressed bytes or more gives its video VGE_INGEST_ERR_ARG (the
 * kernel's bit positions are 32-bit).  *workspace_bytes (may be NULL): what the decode below needs for these streams. */
int vge_ingest_plan_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                        int n_threads, const int32_t* videos, int vit_dim, vge_inflate_desc* descs,
                        vge_clip_info* info, int64_t* workspace_bytes);

/* Device.  data, descs, the five arrays, workspace and status[n_videos] (int32) are device pointers (descs and
 * workspace 8-byte aligned, the rest 4-byte); n_rows / kp_rows are the rows of pose, gori, betas, vit / of kp.  The call
 * is asynchronous on `stream` (a hipStream_t; NULL: the default stream), allocates nothing and learns nothing from the
 * device: its return value covers the arguments the host can see and the launches (VGE_INGEST_ERR_ARG, or 2 for a HIP
 * failure, named by vge_last_error); the per-video codes are in status[] only, which the call clears first.
 * One wave inflates one stream (stored members and keypoint files take the same kernel's copy path) with a 32 KiB
 * history ring in LDS; float64 streams inflate into the workspace and a second kernel converts them with the host's
 * (float) rounding.  The kernel checks every descriptor against data_bytes, workspace_bytes and the row counts: a
 * stream reads only its own [src_off, src_off + csize), writes only its own elements, and every loop consumes input or
 * produces output.  A stream that fails sets its video's status (VGE_INGEST_ERR_IO; the first failure wins), may leave
 * any bytes in that video's own rows and touches nothing else.
 * Accept / reject equals zlib's (and so vge_ingest_decode_mem's) with one class outside the equality: a member whose
 * stream carries more than its npy header declares.  The device stops at the count and reports OK, as np.load would;
 * the host's verdict there depends on whether zlib had already decoded the next symbol when its output ran full.
 * CRC-32 is checked by neither side. */
int vge_ingest_decode_device(const uint8_t* data, int64_t data_bytes, const vge_inflate_desc* descs, int n_descs,
                             int n_videos, int64_t n_rows, int64_t kp_rows, int vit_dim, float* pose, float* gori,
                             float* betas, float* vit, float* kp, void* workspace, int64_t workspace_bytes,
                             int32_t* status, void* stream);
/* Workspace for host-side descs[n_descs] (the sum of the float64 streams, each 8-byte aligned; at least 8). */
size_t vge_ingest_decode_device_workspace_bytes(const vge_inflate_desc* descs, int n_descs);
/* The kernel's granules, for the tests: symbols decoded per batch (one per lane), bytes of the LDS history ring,
 * compressed bytes staged in LDS per refill. */
int vge_ingest_decode_device_batch_symbols(void);
int vge_ingest_decode_device_ring_bytes(void);
int vge_ingest_decode_device_stage_bytes(void);

/* The code-length rules the kernel applies (csrc/vge_inflate_tables.h), on the host: lens[n] (0..15; n <= 288),
 * kind 0 the code-length code, 1 a length/literal set, 2 a distance set.  Returns 0 when zlib accepts the set, 1 when
 * it rejects it, -1 for a bad argument. */
int vge_inflate_check_lengths(const uint8_t* lens, int n, int kind);

#ifdef __cplusplus
}
#endif
#endif /* VGE_INGEST_H */
