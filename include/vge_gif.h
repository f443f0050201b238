/* vge_gif.h -- animated GIF videos decoded to uint8 RGB frames, on host threads or on the device.
 *
 * The reference opens video files; this project took only folders of still frames.  The animated GIF is the one
 * single-file video format that can be decoded and checked here: it is what diffusers' export_to_gif, imageio's
 * mimsave and ffmpeg's gif muxer write.  A GIF frame is a delta, not a picture: a sub-rectangle of LZW-coded colour
 * indices, a local or global colour table, a transparent index and a disposal method, drawn onto a canvas that is
 * carried from frame to frame.  This ABI decodes it twice with the same verdicts: on host threads, and on the device
 * from the file bytes alone (csrc/vge_gif.hip).  Both run the same per-code LZW step and the same per-pixel
 * composition step (csrc/vge_gif_lzw.h).
 *
 * Conventions are vge_png.h's: files on disk or packed in memory (file j is sizes[j] bytes at data + offsets[j]; gaps
 * and any order are fine); one status per frame; every call returns VGE_GIF_OK or the first failing code;
 * vge_last_error names the first failure; n_threads <= 0: vge_ingest_default_threads().
 *
 * A call's output holds the frames of its files back to back: file j's frames follow those of files 0 .. j - 1, and a
 * file has as many frames as it has image descriptors (the probe's n_frames).  All files of one call share the logical
 * screen (width, height); a file of another size gets VGE_GIF_ERR_SHAPE on all its frames.  A file that fails before
 * its first image descriptor (not a GIF, truncated header or global table, zero-sized screen, no image) has no frames:
 * its code is in file_status[] only.
 *
 * Accept / reject, the same on host and device (and Pillow's):
 *   - a frame is accepted when its LZW stream yields w * h indices; whatever follows the last index is ignored
 *     (further codes, a missing end code, a missing block terminator or trailer byte);
 *   - a stream that does not begin with a clear code is accepted, and so are repeated clear codes;
 *   - when the dictionary is full (4096 entries) codes stay 12 bits wide and nothing is added until a clear code;
 *   - a frame is rejected with VGE_GIF_ERR_IO when a code is greater than the next free entry (a code equal to it is
 *     the legal "KwKwK" case; the first code after a clear code must be a plain colour index), or when the data ends
 *     or an end code arrives before the count is reached;
 *   - a rejected frame takes every later frame of its file with it, each with the same code; the earlier frames stand.
 * Comment, application and plain-text extensions, delays and loop counts are ignored.  GIF87a is accepted.
 *
 * Composition is what PIL.ImageSequence frames give after .convert("RGB"); DESIGN.md section 5b'''' states the rule.
 */
#ifndef VGE_GIF_H
#define VGE_GIF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  VGE_GIF_OK = 0,
  VGE_GIF_ERR_ARG = 1,        /* bad argument; a file of 2^28 bytes or more (bit positions are 32-bit) */
  VGE_GIF_ERR_HIP = 2,        /* a HIP call failed */
  VGE_GIF_ERR_IO = 7,         /* not a GIF, truncated, no image, a zero-sized screen or frame, minimum code size outside
                                 2..8, a corrupt stream */
  VGE_GIF_ERR_SHAPE = 8,      /* the file's logical screen differs from the call's */
  VGE_GIF_ERR_NO_PALETTE = 40, /* a frame has neither a local nor a global colour table */
  VGE_GIF_ERR_BOUNDS = 41     /* a frame rectangle reaches outside the logical screen */
};

typedef struct {
  int32_t width, height; /* the logical screen */
  int32_t n_frames;      /* image descriptors */
  int32_t status;        /* VGE_GIF_OK or the first failing code the parser sees (no LZW code is looked at) */
  int64_t lzw_bytes;     /* payload bytes of all data sub-blocks */
  int64_t n_blocks;      /* non-empty data sub-blocks */
} vge_gif_info;

/* Headers and block structure only; nothing is decoded. */
int vge_gif_probe(const char* const* paths, int n, int n_threads, vge_gif_info* info);
int vge_gif_probe_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                      int n_threads, vge_gif_info* info);

/* The host decoder: rgb is uint8 [frame_cap, height, width, 3] and status int32 [frame_cap] in host memory.  Files are
 * parsed on threads, then the LZW streams of all frames of all files are spread over the threads, then the files are
 * composed on threads.  *n_frames_out (may be NULL): the frames of all files; when that exceeds frame_cap nothing is
 * decoded and the call returns VGE_GIF_ERR_ARG.  file_status[n] (may be NULL): per file, its first failing code.  A
 * failing frame and the later frames of its file have unspecified pixels.  A file that does not lie inside
 * [0, data_bytes) gets VGE_GIF_ERR_ARG and none of its bytes is read. */
int vge_gif_decode(const char* const* paths, int n, int n_threads, int width, int height, int64_t frame_cap,
                   uint8_t* rgb, int32_t* status, int32_t* file_status, int64_t* n_frames_out);
int vge_gif_decode_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                       int n_threads, int width, int height, int64_t frame_cap, uint8_t* rgb, int32_t* status,
                       int32_t* file_status, int64_t* n_frames_out);

/* ---- Device route.  Plain data, copied to the device as bytes. */
typedef struct {
  int64_t file_off;   /* the frame's file inside the buffer: segments and the colour table must lie inside it */
  int64_t file_bytes;
  int64_t gat_off;    /* workspace byte offset of the frame's gathered LZW bytes */
  int64_t gat_bytes;
  int64_t slot_off;   /* workspace byte offset of the frame's index plane, w * h bytes in stored row order (16-aligned) */
  int64_t ct_off;     /* the frame's colour table (local, else global), relative to file_off */
  int32_t ct_size;    /* its entries: 2..256 */
  int32_t file;       /* owner file */
  int32_t index;      /* frame index within it; a file's descriptors are consecutive and start at index 0 */
  int32_t frame;      /* index into status[] and the output's first axis; -1: an unused slot */
  int32_t x, y, w, h; /* rectangle on the logical screen */
  int32_t interlace;
  int32_t min_code_size;
  int32_t transparent; /* index, or -1 */
  int32_t disposal;    /* effective method: 0..3 (an unspecified method inherits the previous frame's) */
  int32_t fill_rgb;    /* what the frame leaves pending as a constant (method 2; method 3 on frame 0):
                          R | G << 8 | B << 16, or -1 for none */
  int32_t first_rgb;   /* frame 0: the canvas before it */
  int32_t plan_status; /* non-zero: the plan refused the frame (or an earlier one of its file) with this code */
  int32_t reserved;
} vge_gif_desc;

typedef struct { /* the shape of vge_png_segment */
  int64_t src_off; /* payload bytes inside the buffer */
  int64_t dst_off; /* where they go inside the workspace */
  int64_t bytes;
  int32_t desc;    /* index of the descriptor the segment belongs to */
  int32_t reserved;
} vge_gif_segment;

/* Host; decodes nothing.  Walks every file and emits one descriptor per frame, file after file, into descs[desc_cap]
 * (frame = position in that order) and one segment per non-empty data sub-block into segs[seg_cap]; either may be NULL
 * with capacity 0 to count only (the sums of the probe's n_frames and n_blocks always suffice).  status[desc_cap] (may
 * be NULL) gets the plan's code per frame: a frame the parser refuses, and every later frame of its file, carries it in
 * plan_status and here, and owns no workspace.  file_status[n] (may be NULL) as in vge_gif_decode_mem.  Returns
 * VGE_GIF_ERR_ARG when a capacity is too small, else VGE_GIF_OK or the first failing code. */
int vge_gif_plan_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                     int n_threads, int width, int height, vge_gif_desc* descs, int64_t desc_cap, int64_t* n_descs,
                     vge_gif_segment* segs, int64_t seg_cap, int64_t* n_segs, int32_t* status, int32_t* file_status,
                     int64_t* workspace_bytes);

/* Device.  data, descs, segs, workspace, rgb (uint8 [n_frames, height, width, 3]) and status[n_frames] (int32) are
 * device pointers (descs and segs 8-byte aligned, workspace 16-byte, status 4-byte).  The call is asynchronous on
 * `stream` (a hipStream_t; NULL: the default stream), allocates nothing and learns nothing from the device: its return
 * value covers the arguments the host can see and the launches; the per-frame codes are in status[] only, which the
 * call clears first.  Three kernels: gather (each frame's sub-blocks into one run of the workspace; the kernel of the
 * PNG route, csrc/vge_gather.h), LZW (one wave per frame, dictionary in LDS, writes the frame's w * h indices into its
 * slot) and compose (a row of workgroups per file; a lane per screen pixel walks the file's frames in order with the canvas and the pending restore
 * in registers, stores every frame's RGB, stops at the first frame whose status is set and gives the later frames of
 * the file that status).  Every descriptor and segment is checked against data_bytes, workspace_bytes, n_frames and
 * the screen: a frame reads only its own file bytes and gathered run, writes only its own slot and output frame, and
 * every loop consumes input or produces output.  The workspace may be reused as it is.
 * n_files: the files of the plan; the compose kernel runs a row of workgroups per file and finds the file's first
 * descriptor by a binary search on the owner field.  The order of descs[] is therefore part of the contract, and it is
 * the order the plan emits: owner files in increasing order, each file's descriptors consecutive with index 0, 1, 2...
 * A descriptor that cannot be reached that way (its run does not start at index 0, its owner is outside [0, n_files),
 * another run of the same owner comes first, the owners are out of order) gets VGE_GIF_ERR_ARG from the LZW kernel,
 * and an unused slot (frame = -1) inside a file gives the later frames of that file VGE_GIF_ERR_ARG: no frame is left
 * with status 0 and no pixels. */
int vge_gif_decode_device(const uint8_t* data, int64_t data_bytes, const vge_gif_desc* descs, int n_descs,
                          const vge_gif_segment* segs, int64_t n_segs, int n_frames, int n_files, int width, int height,
                          void* workspace, int64_t workspace_bytes, uint8_t* rgb, int32_t* status, void* stream);
/* Workspace for host-side descs[n_descs]: the end of the last gathered run or slot (at least 16). */
size_t vge_gif_decode_device_workspace_bytes(const vge_gif_desc* descs, int n_descs);

#ifdef __cplusplus
}
#endif
#endif /* VGE_GIF_H */
