"""The frame front end: folders of baseline-JPEG frames -> uint8 RGB frame tensors (include/vge_frames.h).

The reference writes every frame of a video to frames/<action>/<video>/frame_%06d.jpg and reads the JPEGs back with
cv2.imread (extract_mesh.py:47-82, 200-209), so its models see pixels that went through libjpeg's decoder.  load_frames
gives the same pixels: Huffman decoding on host threads (vge_jpeg_entropy_decode) into pinned memory, one asynchronous
upload on the caller's stream, and dequantise / IDCT / upsample / colour convert in one HIP kernel
(vge_jpeg_reconstruct); without a GPU, or with device="cpu", the plain-C++ reconstruct with the same arithmetic.
Channel order is RGB (the extractors here take RGB; cv2.imread's BGR is the same bytes reversed).

The other direction, for frames that are already in memory: jpeg_roundtrip gives the pixels cv2.imwrite + cv2.imread
would give without leaving the device (vge_jpeg_forward, then vge_jpeg_reconstruct), and save_frames writes the
reference's frame_%06d.jpg cache byte for byte as libjpeg does (vge_jpeg_forward + vge_jpeg_entropy_encode).
encode_frames gives the same files in memory; on a GPU tensor it also Huffman-codes on the device
(vge_jpeg_entropy_plan / vge_jpeg_entropy_emit, csrc/vge_jpeg_huff.hip), and save_frames(entropy="device") writes
its bytes.  decode_frames is the inverse of encode_frames: files held in memory, on either side, back to frames; for
files on a GPU, and for load_frames(entropy="device"), Huffman decoding runs on the device too
(vge_jpeg_entropy_decode_device, csrc/vge_jpeg_dehuff.hip) and what is uploaded is the file bytes.

Folders of PNG frames (include/vge_png.h) take the same calls: a video is JPEG or PNG by its first file's signature;
entropy "host" inflates and unfilters on host threads (vge_png_decode) and uploads the pixels, entropy "device" uploads
the file bytes and runs vge_png_decode_device (csrc/vge_png.hip) on them.

An animated GIF (include/vge_gif.h) is a video in one file: load_frames("clip.gif") gives the frames
PIL.ImageSequence gives after .convert("RGB").  entropy "host" is vge_gif_decode on host threads, entropy "device"
vge_gif_plan_mem and vge_gif_decode_device (csrc/vge_gif.hip) on the uploaded file bytes; decode_gifs takes files
packed in host memory.

A lossless WebP file (include/vge_webp.h) is a video in one file in the same way (load_frames("clip.webp"),
decode_webps; vge_webp_decode on host threads, or vge_webp_plan_mem and vge_webp_decode_device, csrc/vge_webp.hip, on
the uploaded file bytes), and a folder or list of still .webp files is a video of one frame per file.

An animated PNG (include/vge_apng.h) given as the path of one file is a video in the same way (load_frames("clip.png"),
decode_apngs; vge_apng_decode on host threads, or vge_apng_plan_mem and vge_apng_decode_device, csrc/vge_apng.hip, on
the uploaded file bytes): the frames are what PIL.ImageSequence gives after .convert("RGB").
"""
from __future__ import annotations

import ctypes as C
import logging
import os
from functools import partial
from pathlib import Path
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import lib as L

log = logging.getLogger("vge.frames")

PathLike = Union[str, os.PathLike]


class UnsupportedJpegError(L.VgeError):
    """A JPEG of a kind the decoder is not built for (progressive, arithmetic-coded, 12-bit, CMYK, other sampling
    factors); the message names the kind and the file."""


class UnsupportedPngError(L.VgeError):
    """A PNG of a kind the decoders are not built for (interlaced, not 8 bits per sample, palette); the message names
    the kind and the file."""


class UnsupportedWebpError(L.VgeError):
    """A WebP the decoders refuse by name (a lossy VP8 / ALPH frame, a frame outside the canvas or of another size
    than its VP8L header, more prefix-code groups than the table arena holds); the message names the kind and the
    file."""


class UnsupportedGifError(L.VgeError):
    """A GIF the decoders refuse by name (a frame without any colour table, a frame that reaches outside the logical
    screen); the message names the kind and the file."""


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
GIF_SIGNATURES = (b"GIF87a", b"GIF89a")


def list_frames(folder: PathLike, ext: str = ".jpg") -> List[str]:
    """extract_mesh.py:203-205: sorted(join(dir, f) for f in os.listdir(dir) if f.endswith('.jpg')); ext=".png" lists
    a folder of PNG frames the same way."""
    folder = os.fspath(folder)
    return sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.endswith(ext))


def _paths_array(paths: Sequence[str]):
    return (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])


def probe(paths: Sequence[PathLike], threads: int = 0) -> np.ndarray:
    """Headers only: int32 [n, 6] rows of (width, height, components, h0, v0, status)."""
    paths = [os.fspath(p) for p in paths]
    info = (L.JpegInfo * max(len(paths), 1))()
    if paths:
        L.load().vge_jpeg_probe(_paths_array(paths), len(paths), int(threads), info)
    return _info_rows(info, len(paths))


def make_layout(width: int, height: int, n_comp: int, h0: int, v0: int) -> L.JpegLayout:
    lay = L.JpegLayout()
    L.check(L.load().vge_jpeg_make_layout(int(width), int(height), int(n_comp), int(h0), int(v0), C.byref(lay)),
            "vge_jpeg_make_layout")
    return lay


def _resolve_device(device):
    import torch
    if device is None:
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    return torch.device(device)


def _decode_group(paths: List[str], lay: L.JpegLayout, device, threads: int):
    """One layout's frames -> (uint8 [n, H, W, 3] tensor on `device`, int32 status [n])."""
    import torch
    n = len(paths)
    lib = L.load()
    on_gpu = device.type == "cuda"
    coef = torch.empty((n, lay.blocks_per_frame, 64), dtype=torch.int16, pin_memory=on_gpu)
    qtab = torch.empty((n, 3, 64), dtype=torch.int16, pin_memory=on_gpu)  # uint16 bits
    status = np.zeros(n, np.int32)
    lib.vge_jpeg_entropy_decode(_paths_array(paths), n, int(threads), C.byref(lay), coef.data_ptr(), qtab.data_ptr(),
                                status.ctypes.data)
    out = torch.empty((n, lay.height, lay.width, 3), dtype=torch.uint8, device=device)
    if on_gpu:
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            coef_d = coef.to(device, non_blocking=True)   # asynchronous, from pinned memory, ahead of the kernel
            qtab_d = qtab.to(device, non_blocking=True)
            L.check(lib.vge_jpeg_reconstruct(coef_d.data_ptr(), qtab_d.data_ptr(), C.byref(lay), n, out.data_ptr(),
                                             stream.cuda_stream), "vge_jpeg_reconstruct")
    else:
        L.check(lib.vge_jpeg_reconstruct_host(coef.data_ptr(), qtab.data_ptr(), C.byref(lay), n, int(threads),
                                              out.data_ptr()), "vge_jpeg_reconstruct_host")
    return out, status


def _info_rows(info, n: int) -> np.ndarray:
    return np.array([[i.width, i.height, i.n_comp, i.h0, i.v0, i.status] for i in info[:n]],
                    dtype=np.int32).reshape(-1, 6)


def probe_mem(data: np.ndarray, offsets: np.ndarray, sizes: np.ndarray, threads: int = 0) -> np.ndarray:
    """probe() for files in host memory: file i is data[offsets[i]:offsets[i] + sizes[i]] (vge_jpeg_probe_mem)."""
    n = len(offsets)
    info = (L.JpegInfo * max(n, 1))()
    if n:
        L.load().vge_jpeg_probe_mem(data.ctypes.data, data.size, offsets.ctypes.data, sizes.ctypes.data, n,
                                    int(threads), info)
    return _info_rows(info, n)


def _read_files(paths: Sequence[str], threads: int, pin: bool):
    """The raw bytes of the files, back to back in one (pinned) uint8 tensor, read on host threads
    (vge_jpeg_file_sizes / vge_jpeg_read_files) -> (tensor, offsets int64 [n], sizes int64 [n]).  An unreadable file
    has size 0 and one that can no longer be read zero bytes, which decode to ERR_IO as an unreadable path does."""
    import torch
    lib = L.load()
    n = len(paths)
    arr = _paths_array(paths)
    sizes, offsets = np.zeros(n, np.int64), np.zeros(n, np.int64)
    L.check(lib.vge_jpeg_file_sizes(arr, n, int(threads), sizes.ctypes.data), "vge_jpeg_file_sizes")
    np.cumsum(sizes[:-1], out=offsets[1:])
    buf = torch.empty(int(sizes.sum()), dtype=torch.uint8, pin_memory=pin)
    lib.vge_jpeg_read_files(arr, n, int(threads), offsets.ctypes.data, sizes.ctypes.data, buf.data_ptr(),
                            int(buf.numel()), None)   # a file that fails shows in the decoder's status
    return buf, offsets, sizes


def _decode_group_device(data_d, offsets: np.ndarray, sizes: np.ndarray, lay: L.JpegLayout, rounds=None):
    """One layout's files, bytes already on the GPU (data_d: uint8 tensor) -> (uint8 [n, H, W, 3] tensor on that GPU,
    int32 status [n]): vge_jpeg_entropy_decode_device feeds vge_jpeg_reconstruct on the current stream; the one host
    synchronisation is the copy of the statuses at the end.  rounds: an int32 [n] tensor on the device to fill."""
    import torch
    lib = L.load()
    dev = data_d.device
    n = len(offsets)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        table = torch.from_numpy(np.stack([np.ascontiguousarray(offsets, np.int64),
                                           np.ascontiguousarray(sizes, np.int64)])).to(dev)
        nbytes = int(data_d.numel())
        ws = torch.empty(int(lib.vge_jpeg_entropy_decode_workspace_bytes(C.byref(lay), n, nbytes)),
                         dtype=torch.uint8, device=dev)
        coef = torch.empty((n, lay.blocks_per_frame, 64), dtype=torch.int16, device=dev)
        qtab = torch.empty((n, 3, 64), dtype=torch.int16, device=dev)
        status_d = torch.empty(n, dtype=torch.int32, device=dev)
        out = torch.empty((n, lay.height, lay.width, 3), dtype=torch.uint8, device=dev)
        L.check(lib.vge_jpeg_entropy_decode_device(data_d.data_ptr(), nbytes, table[0].data_ptr(), table[1].data_ptr(),
                                                   n, C.byref(lay), ws.data_ptr(), coef.data_ptr(), qtab.data_ptr(),
                                                   status_d.data_ptr(),
                                                   rounds.data_ptr() if rounds is not None else None,
                                                   stream.cuda_stream), "vge_jpeg_entropy_decode_device")
        L.check(lib.vge_jpeg_reconstruct(coef.data_ptr(), qtab.data_ptr(), C.byref(lay), n, out.data_ptr(),
                                         stream.cuda_stream), "vge_jpeg_reconstruct")
        status = status_d.cpu().numpy()
    return out, status


def _decode_group_mem(data, offsets: np.ndarray, sizes: np.ndarray, lay: L.JpegLayout, device, threads: int):
    """_decode_group for files in host memory (data: a uint8 CPU tensor): vge_jpeg_entropy_decode_mem, then the
    reconstruct on `device`."""
    import torch
    n = len(offsets)
    lib = L.load()
    on_gpu = device.type == "cuda"
    coef = torch.empty((n, lay.blocks_per_frame, 64), dtype=torch.int16, pin_memory=on_gpu)
    qtab = torch.empty((n, 3, 64), dtype=torch.int16, pin_memory=on_gpu)  # uint16 bits
    status = np.zeros(n, np.int32)
    offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
    lib.vge_jpeg_entropy_decode_mem(data.data_ptr(), int(data.numel()), offsets.ctypes.data, sizes.ctypes.data, n,
                                    int(threads), C.byref(lay), coef.data_ptr(), qtab.data_ptr(), status.ctypes.data)
    out = torch.empty((n, lay.height, lay.width, 3), dtype=torch.uint8, device=device)
    if on_gpu:
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            coef_d = coef.to(device, non_blocking=True)
            qtab_d = qtab.to(device, non_blocking=True)
            L.check(lib.vge_jpeg_reconstruct(coef_d.data_ptr(), qtab_d.data_ptr(), C.byref(lay), n, out.data_ptr(),
                                             stream.cuda_stream), "vge_jpeg_reconstruct")
    else:
        L.check(lib.vge_jpeg_reconstruct_host(coef.data_ptr(), qtab.data_ptr(), C.byref(lay), n, int(threads),
                                              out.data_ptr()), "vge_jpeg_reconstruct_host")
    return out, status


def _raise_unsupported(names, statuses) -> None:
    for p, s in zip(names, statuses):
        if int(s) in L.JPEG_UNSUPPORTED:
            raise UnsupportedJpegError(f"{p}: unsupported JPEG: {L.JPEG_UNSUPPORTED[int(s)]} "
                                       f"({L.JPEG_STATUS[int(s)]})")


# ---- PNG frames (include/vge_png.h) and the videos in one file: GIF (include/vge_gif.h), lossless WebP
# ---- (include/vge_webp.h), APNG (include/vge_apng.h)

class _VideoFormat(NamedTuple):
    """What differs between the formats whose Python front end is otherwise one text: plain data, no behaviour.  The
    first ten fields describe the format's C interface and its refusals, and the PNG still frames have them too; the
    others belong to the formats in which a file is a video (VIDEO_FILE_FORMATS)."""
    lib: str                         # the prefix of the format's C functions
    info: type                       # L.*Info, a probe's record
    fields: Tuple[str, ...]          # its fields in the order of a probe row's columns; the status is the last
    desc: type                       # L.*Desc, the device plan's record of a frame
    segment: Optional[type]          # L.*Segment, the plan's record of a run of bytes to gather; None: gathers nothing
    n_key: int                       # the leading columns that files of one decode call share
    status: dict                     # the status names of the log lines
    unsupported: dict                # the statuses refused by name ...
    error: type                      # ... the exception they raise ...
    kind: str                        # ... and what its message calls the format
    count_col: Optional[int] = None  # the probe column of a file's frame count
    seg_col: Optional[int] = None    # the probe column of a file's segment count, with `segment`
    raise_in_keep: bool = False      # an unsupported status can also come from the decoders, and is raised then too
    noun: str = ""                   # what decode_*'s refusal of device memory says the plan walks
    public: str = ""                 # the decode_* function that refusal names


_PNG = _VideoFormat("vge_png", L.PngInfo, ("width", "height", "color_type", "bit_depth", "interlace", "n_idat",
                                           "idat_bytes", "status"), L.PngDesc, L.PngSegment, 3, L.PNG_STATUS,
                    L.PNG_UNSUPPORTED, UnsupportedPngError, "PNG")
_GIF = _VideoFormat("vge_gif", L.GifInfo, ("width", "height", "n_frames", "lzw_bytes", "n_blocks", "status"),
                    L.GifDesc, L.GifSegment, 2, L.GIF_STATUS, L.GIF_UNSUPPORTED, UnsupportedGifError, "GIF",
                    count_col=2, seg_col=4, noun="data sub-block", public="decode_gifs")
# raise_in_keep is WebP's alone: only its decoders see that a frame asks for more prefix-code groups than they hold
_WEBP = _VideoFormat("vge_webp", L.WebpInfo, ("width", "height", "n_frames", "vp8l_bytes", "n_chunks", "status"),
                     L.WebpDesc, None, 2, L.WEBP_STATUS, L.WEBP_UNSUPPORTED, UnsupportedWebpError, "WebP",
                     count_col=2, raise_in_keep=True, noun="chunk", public="decode_webps")
# an APNG is refused by name for the kinds the still path refuses, in the same words and under the same status names
_APNG = _VideoFormat("vge_apng", L.ApngInfo, ("width", "height", "color_type", "bit_depth", "interlace", "n_frames",
                                              "default_image", "n_chunks", "data_bytes", "status"),
                     L.ApngDesc, L.ApngSegment, 3, L.APNG_STATUS, L.APNG_UNSUPPORTED, UnsupportedPngError, "PNG",
                     count_col=5, seg_col=7, noun="chunk", public="decode_apngs")
VIDEO_FILE_FORMATS = {"gif": _GIF, "webp": _WEBP, "apng": _APNG}


def _rows(fmt: _VideoFormat, info, n: int) -> np.ndarray:
    return np.array([[getattr(i, f) for f in fmt.fields] for i in info[:n]],
                    dtype=np.int64).reshape(-1, len(fmt.fields))


# the tests' case files read the C probes through these
_png_rows, _gif_rows, _webp_rows, _apng_rows = (partial(_rows, f) for f in (_PNG, _GIF, _WEBP, _APNG))


def _probe(fmt: _VideoFormat, paths: Sequence[PathLike], threads: int) -> np.ndarray:
    paths = [os.fspath(p) for p in paths]
    info = (fmt.info * max(len(paths), 1))()
    if paths:
        getattr(L.load(), fmt.lib + "_probe")(_paths_array(paths), len(paths), int(threads), info)
    return _rows(fmt, info, len(paths))


def _probe_mem(fmt: _VideoFormat, data: np.ndarray, offsets: np.ndarray, sizes: np.ndarray, threads: int) -> np.ndarray:
    n = len(offsets)
    info = (fmt.info * max(n, 1))()
    if n:
        offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
        getattr(L.load(), fmt.lib + "_probe_mem")(data.ctypes.data, data.size, offsets.ctypes.data, sizes.ctypes.data,
                                                  n, int(threads), info)
    return _rows(fmt, info, n)


def png_probe(paths: Sequence[PathLike], threads: int = 0) -> np.ndarray:
    """Headers only: int64 [n, 8] rows of (width, height, colour type, bit depth, interlace, IDAT chunks, IDAT bytes,
    status) (vge_png_probe)."""
    return _probe(_PNG, paths, threads)


def png_probe_mem(data: np.ndarray, offsets: np.ndarray, sizes: np.ndarray, threads: int = 0) -> np.ndarray:
    """png_probe() for files in host memory: file i is data[offsets[i]:offsets[i] + sizes[i]] (vge_png_probe_mem)."""
    return _probe_mem(_PNG, data, offsets, sizes, threads)


def gif_probe(paths: Sequence[PathLike], threads: int = 0) -> np.ndarray:
    """Headers and block structure only: int64 [n, 6] rows of (screen width, screen height, frames, LZW bytes, data
    sub-blocks, status) (vge_gif_probe)."""
    return _probe(_GIF, paths, threads)


def gif_probe_mem(data: np.ndarray, offsets: np.ndarray, sizes: np.ndarray, threads: int = 0) -> np.ndarray:
    """gif_probe() for files in host memory: file i is data[offsets[i]:offsets[i] + sizes[i]] (vge_gif_probe_mem)."""
    return _probe_mem(_GIF, data, offsets, sizes, threads)


def webp_probe(paths: Sequence[PathLike], threads: int = 0) -> np.ndarray:
    """Headers and chunk structure only: int64 [n, 6] rows of (canvas width, canvas height, frames, VP8L payload
    bytes, chunks, status) (vge_webp_probe)."""
    return _probe(_WEBP, paths, threads)


def webp_probe_mem(data: np.ndarray, offsets: np.ndarray, sizes: np.ndarray, threads: int = 0) -> np.ndarray:
    """webp_probe() for files in host memory: file i is data[offsets[i]:offsets[i] + sizes[i]] (vge_webp_probe_mem)."""
    return _probe_mem(_WEBP, data, offsets, sizes, threads)


def apng_probe(paths: Sequence[PathLike], threads: int = 0) -> np.ndarray:
    """Chunk headers only: int64 [n, 10] rows of (canvas width, canvas height, colour type, bit depth, interlace,
    frames, whether frame 0 is a default image outside the animation, non-empty IDAT / fdAT payloads, their bytes,
    status) (vge_apng_probe).  A PNG that is not animated is a video of one frame."""
    return _probe(_APNG, paths, threads)


def apng_probe_mem(data: np.ndarray, offsets: np.ndarray, sizes: np.ndarray, threads: int = 0) -> np.ndarray:
    """apng_probe() for files in host memory: file i is data[offsets[i]:offsets[i] + sizes[i]] (vge_apng_probe_mem)."""
    return _probe_mem(_APNG, data, offsets, sizes, threads)


def _refuse(fmt: _VideoFormat, names, statuses) -> None:
    for p, s in zip(names, statuses):
        if int(s) in fmt.unsupported:
            raise fmt.error(f"{p}: unsupported {fmt.kind}: {fmt.unsupported[int(s)]} ({fmt.status[int(s)]})")


def _png_decode_group(paths, data, offsets, sizes, key, device, threads: int):
    """One (width, height, colour type)'s frames on host threads, from paths or (paths None) from files in host memory
    (data: a uint8 CPU tensor) -> (uint8 [n, H, W, 3] tensor on `device`, int32 status [n]): vge_png_decode /
    vge_png_decode_mem into pinned memory, then one upload."""
    import torch
    lib = L.load()
    w, h, ct = key
    n = len(paths) if paths is not None else len(offsets)
    on_gpu = device.type == "cuda"
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, pin_memory=on_gpu)
    status = np.zeros(n, np.int32)
    if paths is not None:
        lib.vge_png_decode(_paths_array(paths), n, int(threads), w, h, ct, out.data_ptr(), status.ctypes.data)
    else:
        offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
        lib.vge_png_decode_mem(data.data_ptr(), int(data.numel()), offsets.ctypes.data, sizes.ctypes.data, n,
                               int(threads), w, h, ct, out.data_ptr(), status.ctypes.data)
    if on_gpu:
        with torch.cuda.device(device):
            out = out.to(device, non_blocking=True)
    return out, status


def _png_decode_group_device(data_h: np.ndarray, data_d, offsets: np.ndarray, sizes: np.ndarray, key, threads: int):
    """One (width, height, colour type)'s files, their bytes both in host memory (data_h, which only the plan's chunk
    walk reads) and on the GPU (data_d) -> (uint8 [n, H, W, 3] tensor on that GPU, int32 status [n]):
    vge_png_plan_mem on the host, one upload of the descriptors and segments, vge_png_decode_device on the current
    stream; the one host synchronisation is the copy of the statuses at the end."""
    import torch
    lib = L.load()
    dev = data_d.device
    w, h, ct = key
    n = len(offsets)
    offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
    descs = (L.PngDesc * max(n, 1))()
    planned = np.zeros(n, np.int32)
    n_segs, ws_bytes = C.c_int64(0), C.c_int64(0)
    args = (data_h.ctypes.data, data_h.size, offsets.ctypes.data, sizes.ctypes.data, n, int(threads), w, h, ct, descs)
    lib.vge_png_plan_mem(*args, None, 0, C.byref(n_segs), planned.ctypes.data, None)   # the segment count
    segs = (L.PngSegment * max(n_segs.value, 1))()
    lib.vge_png_plan_mem(*args, segs, n_segs.value, C.byref(n_segs), planned.ctypes.data, C.byref(ws_bytes))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        descs_d = torch.frombuffer(descs, dtype=torch.uint8).to(dev)
        segs_d = torch.frombuffer(segs, dtype=torch.uint8).to(dev)
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
        status_d = torch.empty(n, dtype=torch.int32, device=dev)
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        L.check(lib.vge_png_decode_device(data_d.data_ptr(), int(data_d.numel()), descs_d.data_ptr(), n,
                                          segs_d.data_ptr(), n_segs.value, n, w, h, ct, ws.data_ptr(),
                                          int(ws.numel()), out.data_ptr(), status_d.data_ptr(), stream.cuda_stream),
                "vge_png_decode_device")
        status = status_d.cpu().numpy()
    return out, np.where(planned != 0, planned, status).astype(np.int32)


def _video_decode_group(fmt: _VideoFormat, paths, data, offsets, sizes, key, n_frames: int, device, threads: int):
    """The files of one group -- one logical screen or canvas, for APNG also one colour type: `key` -- on host threads,
    from paths or (paths None) from files in host memory (data: a uint8 CPU tensor) -> (uint8 [n_frames, H, W, 3] tensor
    on `device`, int32 status [n_frames]): vge_*_decode / vge_*_decode_mem into pinned memory, then one upload.
    n_frames: the probe's sum."""
    import torch
    lib = L.load()
    w, h = key[:2]
    on_gpu = device.type == "cuda"
    out = torch.empty((n_frames, h, w, 3), dtype=torch.uint8, pin_memory=on_gpu)
    status = np.zeros(n_frames, np.int32)
    if paths is not None:
        getattr(lib, fmt.lib + "_decode")(_paths_array(paths), len(paths), int(threads), *key, n_frames,
                                          out.data_ptr(), status.ctypes.data, None, None)
    else:
        offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
        getattr(lib, fmt.lib + "_decode_mem")(data.data_ptr(), int(data.numel()), offsets.ctypes.data,
                                              sizes.ctypes.data, len(offsets), int(threads), *key, n_frames,
                                              out.data_ptr(), status.ctypes.data, None, None)
    if on_gpu:
        with torch.cuda.device(device):
            out = out.to(device, non_blocking=True)
    return out, status


def _video_decode_group_device(fmt: _VideoFormat, data_h: np.ndarray, data_d, offsets: np.ndarray, sizes: np.ndarray,
                               key, n_frames: int, seg_cap: int, threads: int):
    """The files of one group, their bytes both in host memory (data_h, which only the plan's walk over the blocks or
    chunks reads) and on the GPU (data_d) -> (uint8 [n_frames, H, W, 3] tensor on that GPU, int32 status [n_frames]):
    vge_*_plan_mem on the host, one upload of the descriptors and (a format that gathers) the segments,
    vge_*_decode_device on the current stream; the one host synchronisation is the copy of the statuses at the end.
    n_frames, seg_cap: the probe's sums."""
    import torch
    lib = L.load()
    dev = data_d.device
    w, h = key[:2]
    offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
    descs = (fmt.desc * max(n_frames, 1))()
    planned = np.zeros(max(n_frames, 1), np.int32)
    n_descs, n_segs, ws_bytes = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    seg_args = ()
    if fmt.segment is not None:
        segs = (fmt.segment * max(seg_cap, 1))()
        seg_args = (segs, seg_cap, C.byref(n_segs))
    getattr(lib, fmt.lib + "_plan_mem")(data_h.ctypes.data, data_h.size, offsets.ctypes.data, sizes.ctypes.data,
                                        len(offsets), int(threads), *key, descs, n_frames, C.byref(n_descs), *seg_args,
                                        planned.ctypes.data, None, C.byref(ws_bytes))
    if n_descs.value != n_frames:
        raise L.VgeError(fmt.lib + "_plan_mem: " + lib.vge_last_error().decode(errors="replace"))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        descs_d = torch.frombuffer(descs, dtype=torch.uint8).to(dev)
        if fmt.segment is not None:
            segs_d = torch.frombuffer(segs, dtype=torch.uint8).to(dev)
            seg_args = (segs_d.data_ptr(), n_segs.value)
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
        status_d = torch.empty(n_frames, dtype=torch.int32, device=dev)
        out = torch.empty((n_frames, h, w, 3), dtype=torch.uint8, device=dev)
        L.check(getattr(lib, fmt.lib + "_decode_device")(data_d.data_ptr(), int(data_d.numel()), descs_d.data_ptr(),
                                                         n_frames, *seg_args, n_frames, len(offsets), *key,
                                                         ws.data_ptr(), int(ws.numel()), out.data_ptr(),
                                                         status_d.data_ptr(), stream.cuda_stream),
                fmt.lib + "_decode_device")
        status = status_d.cpu().numpy()
    planned = planned[:n_frames]
    return out, np.where(planned != 0, planned, status).astype(np.int32)


def _keep_video_frames(fmt: _VideoFormat, name, out, status):
    """(frames, kept) of one video in one file: the frames in front of the first one that failed (the later ones are
    deltas on it)."""
    bad = np.flatnonzero(status != 0)
    n = int(bad[0]) if bad.size else len(status)
    if bad.size:
        if fmt.raise_in_keep:   # what only the decoders see
            _refuse(fmt, [name], [status[n]])
        log.warning("dropping frames %d.. of %s: %s", n, name, fmt.status.get(int(status[n]), int(status[n])))
    return out[:n], np.arange(n, dtype=np.int64)


def _empty_video(device):
    import torch
    return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=device), np.zeros(0, np.int64)


def _decode_video_files(fmt: _VideoFormat, names, paths, raw, raw_off, raw_size, info, device, threads: int,
                        entropy: str):
    """The videos of one format of a call, one file each, from paths (host route) or from their bytes in one host
    tensor `raw` -> one (frames, kept) per file.  info: their probe rows.  Files of one key (_VideoFormat.n_key) share
    one call.  A refusal by name is raised for the whole call before any group decodes."""
    import torch
    _refuse(fmt, names, info[:, -1])
    results: List[Optional[Tuple]] = [None] * len(names)
    groups: dict = {}
    for i, row in enumerate(info):
        # A file with frames, of a size the decoders take.  Only a WebP probe can give frames on a canvas without
        # width or height (a still whose VP8L header it could not read); the GIF and APNG probes give a zero width or
        # height only with zero frames (csrc/vge_gif.cpp, csrc/vge_apng.cpp: both return in front of the first frame,
        # and every file of tests/gif_cases.py and tests/apng_cases.py agrees), and vge_gif_decode refuses such a
        # screen outright (screen_ok).
        if int(row[fmt.count_col]) > 0 and int(row[-1]) != 1 and int(row[0]) > 0 and int(row[1]) > 0:
            groups.setdefault(tuple(int(x) for x in row[:fmt.n_key]), []).append(i)
        else:
            log.warning("no decodable frame in %s: %s", names[i], fmt.status.get(int(row[-1]), int(row[-1])))
            results[i] = _empty_video(device)
    raw_d = None
    if entropy == "device" and groups:
        with torch.cuda.device(device):
            raw_d = raw.to(device, non_blocking=True)   # the one upload: every group decodes out of this buffer
    for key, members in groups.items():
        counts = [int(info[i, fmt.count_col]) for i in members]
        total = sum(counts)
        if entropy == "device":
            seg_cap = int(sum(info[i, fmt.seg_col] for i in members)) if fmt.seg_col is not None else 0
            with torch.cuda.device(device):
                out, status = _video_decode_group_device(fmt, raw.numpy(), raw_d, raw_off[members], raw_size[members],
                                                         key, total, seg_cap, threads)
        elif paths is not None:
            out, status = _video_decode_group(fmt, [paths[i] for i in members], None, None, None, key, total, device,
                                              threads)
        else:
            out, status = _video_decode_group(fmt, None, raw, raw_off[members], raw_size[members], key, total, device,
                                              threads)
        o = 0
        for i, n in zip(members, counts):
            results[i] = _keep_video_frames(fmt, names[i], out[o:o + n], status[o:o + n])
            if results[i][1].size == 0:
                log.warning("no decodable frame in %s", names[i])
            o += n
    return results


def _load_video_files(fmt: _VideoFormat, paths: List[str], device, threads: int, entropy: str):
    """load_videos for the videos of one format that are one file each: one (frames, kept) per file."""
    if entropy == "device":
        raw, raw_off, raw_size = _read_files(paths, threads, pin=True)
        info = _probe_mem(fmt, raw.numpy(), raw_off, raw_size, threads)
        return _decode_video_files(fmt, paths, None, raw, raw_off, raw_size, info, device, threads, entropy)
    return _decode_video_files(fmt, paths, paths, None, None, None, _probe(fmt, paths, threads), device, threads,
                               entropy)


def _load_webp_still_videos(vids: List[List[str]], device, threads: int, entropy: str):
    """load_videos for the videos that are folders or lists of still WebP frames: every file is one frame, and all
    frames of a video have one size (a file of another size is refused with a ValueError that names it)."""
    import torch
    flat = [p for v in vids for p in v]
    per_file = _load_video_files(_WEBP, flat, device, threads, entropy)
    results, o = [], 0
    for v in vids:
        frames, kept, size = [], [], None
        for k, p in enumerate(v):
            fr = per_file[o + k][0]
            if fr.shape[0] != 1:
                log.warning("dropping frame %s: %s", p, "unreadable" if fr.shape[0] == 0 else "an animation")
                continue
            if size is not None and tuple(fr.shape[1:3]) != size:
                raise ValueError(f"{p}: a frame of {fr.shape[2]} x {fr.shape[1]} in a video of {size[1]} x {size[0]}: "
                                 "the still WebP frames of one video must have one size")
            size = tuple(fr.shape[1:3])
            frames.append(fr)
            kept.append(k)
        o += len(v)
        results.append((torch.cat(frames), np.asarray(kept, np.int64)) if frames else _empty_video(device))
    return results


def _packed_offsets(data, offsets, fmt: Optional[_VideoFormat] = None) -> np.ndarray:
    """The first check of the decode_* calls: files packed in a one-dimensional uint8 tensor and their offsets[F + 1]
    as a contiguous int64 array.  fmt: a format whose plan needs the file bytes in host memory."""
    import torch
    if not (isinstance(data, torch.Tensor) and data.dtype == torch.uint8 and data.dim() == 1):
        raise ValueError("data must be a one-dimensional uint8 tensor")
    if fmt is not None and data.device.type != "cpu":
        raise ValueError(f"{fmt.public} needs the file bytes in host memory: the plan walks every {fmt.noun} on the "
                         "host; pass a CPU tensor (entropy='device' uploads it once)")
    off = np.ascontiguousarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, np.int64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("offsets must be int64 [F + 1]")
    return off


def _entropy_word(entropy: Optional[str], default: str) -> str:
    if entropy is None:
        entropy = default
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy must be 'host' or 'device', not {entropy!r}")
    return entropy


def _file_spans(data, off: np.ndarray):
    """offsets[F + 1] -> (starts [F], sizes [F]); a call without files is checked no further."""
    F = off.size - 1
    starts, sizes = off[:F].copy(), np.diff(off)
    if F and ((sizes < 0).any() or off[0] < 0 or off[F] > data.numel()):
        raise ValueError("offsets must be non-decreasing and inside data")
    return starts, sizes


def _check_packed(data, offsets, device, entropy: Optional[str], fmt: _VideoFormat):
    """The arguments of decode_gifs / decode_webps / decode_apngs -> (device, entropy, starts [F], sizes [F])."""
    off = _packed_offsets(data, offsets, fmt)
    device = _resolve_device(device)
    entropy = _entropy_word(entropy, "device" if device.type == "cuda" else "host")
    if entropy == "device" and device.type != "cuda":
        raise ValueError("entropy='device' needs a GPU")
    return (device, entropy) + _file_spans(data, off)


def _decode_packed_videos(fmt: _VideoFormat, data, offsets, device, threads: int, entropy: Optional[str]):
    device, entropy, starts, sizes = _check_packed(data, offsets, device, entropy, fmt)
    if starts.size == 0:
        return []
    data = data.contiguous()
    names = [f"file {i}" for i in range(starts.size)]
    info = _probe_mem(fmt, data.numpy(), starts, sizes, threads)
    return _decode_video_files(fmt, names, None, data, starts, sizes, info, device, threads, entropy)


def decode_gifs(data, offsets, device=None, threads: int = 0, entropy: Optional[str] = None):
    """GIF videos packed in host memory -- (data, offsets[F + 1]): file i at data[offsets[i]:offsets[i + 1]] of a
    one-dimensional uint8 CPU tensor -- -> one (frames, kept) per file, as load_videos gives them.  entropy "host" (the
    default without a GPU) decodes on host threads (vge_gif_decode_mem) and uploads the pixels to `device`; entropy
    "device" (the default with one) uploads the file bytes and runs vge_gif_plan_mem and vge_gif_decode_device.  The
    plan walks every sub-block of every file on the host, so a buffer that lives on a GPU is refused, not copied back."""
    return _decode_packed_videos(_GIF, data, offsets, device, threads, entropy)


def decode_webps(data, offsets, device=None, threads: int = 0, entropy: Optional[str] = None):
    """WebP files packed in host memory -- (data, offsets[F + 1]): file i at data[offsets[i]:offsets[i + 1]] of a
    one-dimensional uint8 CPU tensor -- -> one (frames, kept) per file, as load_videos gives them.  entropy "host" (the
    default without a GPU) decodes on host threads (vge_webp_decode_mem) and uploads the pixels to `device`; entropy
    "device" (the default with one) uploads the file bytes and runs vge_webp_plan_mem and vge_webp_decode_device.  The
    plan walks every chunk of every file on the host, so a buffer that lives on a GPU is refused, not copied back."""
    return _decode_packed_videos(_WEBP, data, offsets, device, threads, entropy)


def decode_apngs(data, offsets, device=None, threads: int = 0, entropy: Optional[str] = None):
    """APNG videos packed in host memory -- (data, offsets[F + 1]): file i at data[offsets[i]:offsets[i + 1]] of a
    one-dimensional uint8 CPU tensor -- -> one (frames, kept) per file, as load_videos gives them.  entropy "host" (the
    default without a GPU) decodes on host threads (vge_apng_decode_mem) and uploads the pixels to `device`; entropy
    "device" (the default with one) uploads the file bytes and runs vge_apng_plan_mem and vge_apng_decode_device.  The
    plan walks every chunk of every file on the host, so a buffer that lives on a GPU is refused, not copied back."""
    return _decode_packed_videos(_APNG, data, offsets, device, threads, entropy)


def _first_good_key(rows: np.ndarray, n_key: int):
    """The layout of a video: its first readable frame's leading probe columns (the last column is the status)."""
    good = np.flatnonzero(rows[:, -1] == 0)
    return tuple(int(x) for x in rows[good[0], :n_key]) if good.size else None


def _keep_decoded(names, out, status, status_names, device):
    """(frames, kept) of one video from its decoded rows and statuses; a failed frame is dropped with a log line."""
    import torch
    for p, s in zip(names, status):
        if s != 0:
            log.warning("dropping frame %s: %s", p, status_names.get(int(s), int(s)))
    kept = np.flatnonzero(status == 0)
    if kept.size != len(names):
        out = out[torch.as_tensor(kept, device=device)]
    return out, kept


def _unreadable_video(names, device):
    """The empty video of frames of which none could be read."""
    for p in names:
        log.warning("dropping frame %s: unreadable", p)
    return _empty_video(device)


def _decode_frames_png(data, starts, sizes, names, device, threads: int, entropy: str):
    """decode_frames for PNG files.  The plan walks chunk headers that lie all over a file, so for data on a GPU the
    file bytes are copied to the host once for it (the pixels never are)."""
    import torch
    data_h = data.cpu() if data.device.type == "cuda" else data
    info = png_probe_mem(data_h.numpy(), starts, sizes, threads)
    _refuse(_PNG, names, info[:, -1])
    key = _first_good_key(info, 3)
    if key is None:
        return _unreadable_video(names, device)
    if entropy == "device":
        data_d = data if data.device.type == "cuda" else data.to(device)
        with torch.cuda.device(device):
            out, status = _png_decode_group_device(data_h.numpy(), data_d, starts, sizes, key, threads)
    else:
        out, status = _png_decode_group(None, data_h, starts, sizes, key, device, threads)
    return _keep_decoded(names, out, status, L.PNG_STATUS, device)


_PROBE_HEAD = 1 << 16   # bytes of a device-resident file copied to the host for its header


def _probe_on_device(data, off: int, size: int) -> np.ndarray:
    """The probe row of one device-resident file from its first kilobytes (the whole file only when the header is
    longer than that)."""
    for take in (min(size, _PROBE_HEAD), size):
        head = data[off:off + take].cpu().numpy()
        row = probe_mem(head, np.zeros(1, np.int64), np.array([take], np.int64), 1)[0]
        if int(row[5]) != 7 or take == size:
            break
    return row


def decode_frames(data, offsets, device=None, threads: int = 0, entropy: Optional[str] = None):
    """The inverse of encode_frames: (data, offsets[F + 1]) -- complete JPEG files in one uint8 tensor, file i at
    data[offsets[i]:offsets[i + 1]] -- -> (frames, kept) as load_frames gives them.
    data on a GPU: the layout comes from the header of the first readable file (its first kilobytes are copied to the
    host for vge_jpeg_probe_mem), then vge_jpeg_entropy_decode_device and vge_jpeg_reconstruct run on the current
    stream and one copy of the statuses gives `kept`: no file byte and no coefficient crosses to the host.  The frames
    are on data's device.
    data on the CPU: entropy "host" (the default) decodes on host threads (vge_jpeg_entropy_decode_mem) and
    reconstructs on `device` (default: the current GPU when there is one, else the CPU); entropy "device" uploads the
    file bytes instead and decodes them there.
    Raises UnsupportedJpegError for a file of an unsupported kind; a file that does not decode is dropped with a log
    message.
    PNG files (the first file's signature decides) take the same arguments: entropy "host" is vge_png_decode_mem,
    entropy "device" vge_png_plan_mem and vge_png_decode_device; UnsupportedPngError for an unsupported kind."""
    off = _packed_offsets(data, offsets)
    data_on_gpu = data.device.type == "cuda"   # such data stays where it is, and is decoded there
    entropy = _entropy_word(entropy, "device" if data_on_gpu else "host")
    if entropy == "host" and data_on_gpu:
        raise ValueError("entropy='host' needs data on the CPU")
    device = data.device if data_on_gpu else _resolve_device(device)
    if entropy == "device" and device.type != "cuda":
        raise ValueError("entropy='device' needs a GPU")
    data = data.contiguous()
    starts, sizes = _file_spans(data, off)
    F = starts.size
    if F == 0:
        return _empty_video(device)
    names = [f"file {i}" for i in range(F)]
    if data[int(starts[0]):int(starts[0]) + min(int(sizes[0]), 8)].cpu().numpy().tobytes() == PNG_SIGNATURE:
        return _decode_frames_png(data, starts, sizes, names, device, threads, entropy)
    key = None
    if data_on_gpu:
        for i in range(F):   # the first readable file decides the layout, as in load_videos
            row = _probe_on_device(data, int(starts[i]), int(sizes[i]))
            _raise_unsupported(names[i:i + 1], row[5:6])
            if int(row[5]) == 0:
                key = tuple(int(x) for x in row[:5])
                break
    else:
        info = probe_mem(data.numpy(), starts, sizes, threads)
        _raise_unsupported(names, info[:, 5])
        key = _first_good_key(info, 5)
    if key is None:
        return _unreadable_video(names, device)
    lay = make_layout(*key)
    if entropy == "device":
        data_d = data if data_on_gpu else data.to(device)
        out, status = _decode_group_device(data_d, starts, sizes, lay)
        _raise_unsupported(names, status)
    else:
        out, status = _decode_group_mem(data, starts, sizes, lay, device, threads)
    return _keep_decoded(names, out, status, L.JPEG_STATUS, device)


SUBSAMPLING = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}   # luma sampling factors (h0, v0)
_qtab_cache: dict = {}   # (device, quality) -> int16-bits [3, 64] tensor on the device


def quant_tables(quality: int) -> np.ndarray:
    """libjpeg's quantisation tables for a quality: uint16 [3, 64], natural order (vge_jpeg_quant_tables)."""
    q = np.zeros((3, 64), np.uint16)
    L.check(L.load().vge_jpeg_quant_tables(int(quality), q.ctypes.data), "vge_jpeg_quant_tables")
    return q


def _check_rgb_frames(frames):
    import torch
    if not (isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.dim() == 4
            and frames.shape[3] == 3 and frames.shape[1] > 0 and frames.shape[2] > 0):
        raise ValueError("frames must be a uint8 [F, H, W, 3] RGB tensor")
    return frames.contiguous()


def _forward(frames, quality: int, subsampling: str, threads: int = 0):
    """The lossy half of libjpeg's encoder: frames (contiguous uint8 [F, H, W, 3]) -> (layout, int16 coefficients
    [F, blocks_per_frame, 64] and the tables as int16 bits [3, 64], both on the frames' device).  On a GPU tensor: the
    HIP kernel on the current stream, nothing synchronises."""
    import torch
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLING)}, not {subsampling!r}")
    lib = L.load()
    F, H, W = (int(v) for v in frames.shape[:3])
    lay = make_layout(W, H, 3, *SUBSAMPLING[subsampling])
    coef = torch.empty((F, lay.blocks_per_frame, 64), dtype=torch.int16, device=frames.device)
    key = (str(frames.device), max(1, min(int(quality), 100)))
    qtab = _qtab_cache.get(key)
    if qtab is None:   # uploaded once per device and quality, so that later calls touch no host memory
        qtab = torch.from_numpy(quant_tables(quality).view(np.int16)).to(frames.device)
        if frames.device.type == "cuda":
            torch.cuda.current_stream(frames.device).synchronize()   # any stream may use the cached copy afterwards
        _qtab_cache[key] = qtab
    if frames.device.type == "cuda":
        with torch.cuda.device(frames.device):
            L.check(lib.vge_jpeg_forward(frames.data_ptr(), C.byref(lay), F, qtab.data_ptr(), coef.data_ptr(),
                                         torch.cuda.current_stream(frames.device).cuda_stream), "vge_jpeg_forward")
    else:
        L.check(lib.vge_jpeg_forward_host(frames.data_ptr(), C.byref(lay), F, int(threads), qtab.data_ptr(),
                                          coef.data_ptr()), "vge_jpeg_forward_host")
    return lay, coef, qtab


def jpeg_roundtrip(frames, quality: int = 95, subsampling: str = "420", out=None):
    """The pixels cv2.imread gives back after cv2.imwrite(frame, quality) -- what every model of the reference sees
    (extract_mesh.py:47-82, 200-209) -- without writing a file: Huffman coding is lossless, so the round trip is the
    encoder's lossy half (vge_jpeg_forward) followed by the decoder's (vge_jpeg_reconstruct).  frames: uint8
    [F, H, W, 3] RGB; returns the same shape on the same device (`out`, when given).  On a GPU tensor both kernels run
    on the current stream with no host synchronisation and no host copy; on a CPU tensor, the two host functions."""
    import torch
    frames = _check_rgb_frames(frames)
    if out is None:
        out = torch.empty_like(frames)
    elif not (out.dtype == torch.uint8 and out.shape == frames.shape and out.device == frames.device
              and out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 tensor of the frames' shape on the frames' device")
    F = int(frames.shape[0])
    if F == 0:
        return out
    lay, coef, qtab = _forward(frames, quality, subsampling)
    qtab_f = qtab.unsqueeze(0).expand(F, 3, 64).contiguous()   # the reconstruct takes one set of tables per frame
    lib = L.load()
    if frames.device.type == "cuda":
        with torch.cuda.device(frames.device):
            L.check(lib.vge_jpeg_reconstruct(coef.data_ptr(), qtab_f.data_ptr(), C.byref(lay), F, out.data_ptr(),
                                             torch.cuda.current_stream(frames.device).cuda_stream),
                    "vge_jpeg_reconstruct")
    else:
        L.check(lib.vge_jpeg_reconstruct_host(coef.data_ptr(), qtab_f.data_ptr(), C.byref(lay), F, 0, out.data_ptr()),
                "vge_jpeg_reconstruct_host")
    return out


def _coefficients_on_host(coef):
    """The coefficient tensor in host memory: one copy into pinned memory when it is on a GPU."""
    import torch
    if coef.device.type != "cuda":
        return coef
    host = torch.empty(coef.shape, dtype=torch.int16, pin_memory=True)
    host.copy_(coef, non_blocking=True)
    torch.cuda.current_stream(coef.device).synchronize()
    return host


def encode_frames(frames, quality: int = 95, subsampling: str = "420", entropy: Optional[str] = None,
                  threads: int = 0, keep_on_device: bool = False):
    """frames (uint8 [F, H, W, 3] RGB, GPU or CPU) -> (data, offsets): the complete JPEG files save_frames writes, in
    memory.  data is a uint8 tensor, offsets int64 [F + 1]; file i is data[offsets[i]:offsets[i + 1]].
    entropy "device" (the default for a GPU tensor): the forward kernel, vge_jpeg_entropy_plan, one copy of the F file
    sizes to the host (the call's only host synchronisation before the result), an exclusive scan, and
    vge_jpeg_entropy_emit; then one copy of the files into pinned memory, or none with keep_on_device=True (data is then
    a tensor on the frames' device).  entropy "host" (the default, and the only choice, for a CPU tensor): the
    coefficients are copied to the host and coded there (vge_jpeg_entropy_encode_mem: once for the sizes, once for the
    bytes).  Raises VgeError for a frame that cannot be coded."""
    import torch
    frames = _check_rgb_frames(frames)
    on_gpu = frames.device.type == "cuda"
    if entropy is None:
        entropy = "device" if on_gpu else "host"
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy must be 'host' or 'device', not {entropy!r}")
    if entropy == "device" and not on_gpu:
        raise ValueError("entropy='device' needs frames on a GPU")
    F = int(frames.shape[0])
    offsets = np.zeros(F + 1, np.int64)
    if F == 0:
        if subsampling not in SUBSAMPLING:
            raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLING)}, not {subsampling!r}")
        dev = frames.device if keep_on_device else "cpu"
        return torch.empty(0, dtype=torch.uint8, device=dev), torch.from_numpy(offsets)
    lib = L.load()
    lay, coef, qtab = _forward(frames, quality, subsampling, threads)
    if entropy == "host":
        coef = _coefficients_on_host(coef)
        q = quant_tables(quality)
        sizes = np.zeros(F, np.int64)
        L.check(lib.vge_jpeg_entropy_encode_mem(coef.data_ptr(), q.ctypes.data, C.byref(lay), F, int(threads), None,
                                                None, 0, sizes.ctypes.data, None), "vge_jpeg_entropy_encode_mem")
        np.cumsum(sizes, out=offsets[1:])
        data = torch.empty(int(offsets[F]), dtype=torch.uint8, pin_memory=on_gpu and keep_on_device)
        L.check(lib.vge_jpeg_entropy_encode_mem(coef.data_ptr(), q.ctypes.data, C.byref(lay), F, int(threads),
                                                offsets.ctypes.data, data.data_ptr(), int(offsets[F]), None, None),
                "vge_jpeg_entropy_encode_mem")
        if keep_on_device and on_gpu:
            data = data.to(frames.device)
        return data, torch.from_numpy(offsets)
    dev = frames.device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws = torch.empty(int(lib.vge_jpeg_entropy_workspace_bytes(C.byref(lay), F)), dtype=torch.uint8, device=dev)
        sizes_d = torch.empty(F, dtype=torch.int64, device=dev)
        status_d = torch.empty(F, dtype=torch.int32, device=dev)
        L.check(lib.vge_jpeg_entropy_plan(coef.data_ptr(), C.byref(lay), F, ws.data_ptr(), sizes_d.data_ptr(),
                                          status_d.data_ptr(), stream.cuda_stream), "vge_jpeg_entropy_plan")
        sizes = sizes_d.cpu().numpy()   # the host has to learn the sizes before it can place the files
        if (sizes <= 0).any():          # a refused frame has size 0 (status VGE_JPEG_ERR_ARG)
            raise L.VgeError(f"vge_jpeg_entropy_plan: frame {int(np.flatnonzero(sizes <= 0)[0])} holds a coefficient "
                             "baseline Huffman coding cannot carry")
        np.cumsum(sizes, out=offsets[1:])
        offsets_d = torch.from_numpy(offsets[:F]).to(dev, non_blocking=True)
        data = torch.empty(int(offsets[F]), dtype=torch.uint8, device=dev)
        L.check(lib.vge_jpeg_entropy_emit(ws.data_ptr(), qtab.data_ptr(), C.byref(lay), F, offsets_d.data_ptr(),
                                          data.data_ptr(), int(offsets[F]), stream.cuda_stream),
                "vge_jpeg_entropy_emit")
        if not keep_on_device:
            host = torch.empty(data.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(data, non_blocking=True)
            stream.synchronize()
            data = host
    return data, torch.from_numpy(offsets)


def save_frames(frames, folder: PathLike, quality: int = 95, subsampling: str = "420", start: int = 0,
                threads: int = 0, entropy: str = "host") -> List[str]:
    """Write frames (uint8 [F, H, W, 3] RGB, GPU or CPU) as <folder>/frame_%06d.jpg numbered from `start`: the frame
    cache extract_mesh.py:47-69 writes with cv2.imwrite, byte for byte what libjpeg writes.  entropy "host": the forward
    kernel, one copy of the coefficients into pinned memory, then Huffman coding and file writing on host threads
    (vge_jpeg_entropy_encode).  entropy "device" (GPU frames only): encode_frames codes the files on the device, one
    copy of the finished files, and the host threads only write them (vge_jpeg_write_files).  list_frames /
    load_frames read the folder back.  Returns the paths; raises VgeError naming the first file that could not be
    written (the other files are written)."""
    frames = _check_rgb_frames(frames)
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy must be 'host' or 'device', not {entropy!r}")
    if entropy == "device" and frames.device.type != "cuda":
        raise ValueError("entropy='device' needs frames on a GPU")
    folder = os.fspath(folder)
    os.makedirs(folder, exist_ok=True)
    F = int(frames.shape[0])
    paths = [os.path.join(folder, f"frame_{int(start) + i:06d}.jpg") for i in range(F)]
    if F == 0:
        return paths
    if entropy == "device":
        data, offsets = encode_frames(frames, quality, subsampling, entropy="device", threads=threads)
        off = offsets.numpy()
        sizes = np.ascontiguousarray(np.diff(off))
        L.check(L.load().vge_jpeg_write_files(data.data_ptr(), off.ctypes.data, sizes.ctypes.data, F, int(threads),
                                              _paths_array(paths), None), "vge_jpeg_write_files")
        return paths
    lay, coef, qtab = _forward(frames, quality, subsampling, threads)
    coef = _coefficients_on_host(coef)
    L.check(L.load().vge_jpeg_entropy_encode(coef.data_ptr(), quant_tables(quality).ctypes.data, C.byref(lay), F,
                                             int(threads), _paths_array(paths), None, None),
            "vge_jpeg_entropy_encode")
    return paths


def load_videos(videos: Sequence[Union[PathLike, Sequence[PathLike]]], device=None, threads: int = 0,
                entropy: str = "host"):
    """Several videos in one go: each entry is a frame folder or a list of JPEG paths.  Videos of one frame size and
    sampling share one entropy-decode call, one upload and one kernel launch.  Returns a list of (frames, kept) as
    load_frames does.  entropy "host": Huffman decoding on host threads, the coefficients are uploaded.  entropy
    "device" (needs a GPU): host threads only read the raw files into one pinned buffer, the file bytes are uploaded
    once -- a quarter of the coefficients' bytes -- and vge_jpeg_entropy_decode_device decodes them; frames, kept,
    dropped frames and errors are the same.
    A video may also be a folder or list of PNG frames (a folder without *.jpg files gives its *.png files in sorted
    order).  A video is JPEG or PNG by its first file's signature, and files of the other kind inside it are dropped as
    unreadable.  PNG videos of one (width, height, colour type) share one call: entropy "host" decodes on host threads
    into pinned memory and uploads the pixels (vge_png_decode); entropy "device" uploads the file bytes once and
    inflates and unfilters them there (vge_png_plan_mem, vge_png_decode_device).  UnsupportedPngError names an
    interlaced, non-8-bit or palette file.
    An entry that is a path to a regular file whose first six bytes are GIF87a or GIF89a is a GIF video
    (include/vge_gif.h): its frames are the video's frames and `kept` indexes them.  GIF videos of one logical screen
    share one call: entropy "host" decodes on host threads into pinned memory and uploads the pixels (vge_gif_decode);
    entropy "device" uploads the file bytes once and runs vge_gif_plan_mem and vge_gif_decode_device.  A frame that
    does not decode is dropped with every later frame of its file (they are deltas on it), with a log line;
    UnsupportedGifError names a file with a frame that has no colour table or that overflows the logical screen.
    An entry that is a path to a regular file with the RIFF....WEBP signature is a lossless WebP video
    (include/vge_webp.h), handled as a GIF video is: vge_webp_decode on host threads, or vge_webp_plan_mem and
    vge_webp_decode_device on the uploaded file bytes.  A folder without *.jpg and *.png files gives its *.webp files,
    and a list whose first file is a WebP is a list of still WebP frames: every file is one frame, and all must have
    one size.  UnsupportedWebpError names a file with a lossy frame, a frame outside its canvas or more prefix-code
    groups than the decoders hold.
    An entry that is a path to a regular file with the PNG signature is an APNG video (include/vge_apng.h), handled as a
    GIF video is: vge_apng_decode on host threads, or vge_apng_plan_mem and vge_apng_decode_device on the uploaded file
    bytes; APNG videos of one (canvas, colour type) share one call, and a PNG file that is not animated is a video of
    one frame.  UnsupportedPngError names an interlaced, non-8-bit or palette file.  Inside a folder or a list, a PNG
    file stays one still frame (its IDAT picture), animated or not."""
    device = _resolve_device(device)
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy must be 'host' or 'device', not {entropy!r}")
    if entropy == "device" and device.type != "cuda":
        raise ValueError("entropy='device' needs a GPU")
    # what each entry is: a video in one file ("gif", "webp", "apng": no frame list), or a folder or list of still WebP
    # frames ("stills"), of PNG frames ("png") or of JPEG frames ("jpg") by its first file
    kinds = [_file_signature(os.fspath(v)) if isinstance(v, (str, os.PathLike)) else None for v in videos]
    vids = [[] if kind else _list_video(v) if isinstance(v, (str, os.PathLike)) else [os.fspath(p) for p in v]
            for v, kind in zip(videos, kinds)]
    kinds = [kind or {"webp": "stills", "apng": "png"}.get(_file_signature(v[0]) if v else None, "jpg")
             for v, kind in zip(vids, kinds)]
    loaders = [(name, partial(_load_video_files, VIDEO_FILE_FORMATS[name])) for name in ("apng", "gif", "webp")]
    loaders += [("stills", _load_webp_still_videos), ("jpg", _load_jpeg_videos), ("png", _load_png_videos)]
    results: List[Optional[Tuple]] = [None] * len(vids)
    for kind, load in loaders:   # in this order: of several files that are refused, the first loader's is raised
        which = [vi for vi, k in enumerate(kinds) if k == kind]
        if which:
            entries = [os.fspath(videos[vi]) if kind in VIDEO_FILE_FORMATS else vids[vi] for vi in which]
            for vi, r in zip(which, load(entries, device, threads, entropy)):
                results[vi] = r
    return results


def _list_video(folder: PathLike) -> List[str]:
    """A frame folder's files: its *.jpg, or when it has none its *.png, or when it has neither its *.webp, in sorted
    order."""
    return list_frames(folder) or list_frames(folder, ext=".png") or list_frames(folder, ext=".webp")


def _file_signature(path: str) -> Optional[str]:
    """What a path to a regular file is by its first bytes: "webp" (RIFF....WEBP: a WebP video or still), else "gif"
    (GIF87a or GIF89a: a GIF video), else "apng" (the PNG signature: an APNG video, or a still PNG, which is a video of
    one frame); None for any other file and for what is not a regular file."""
    try:
        if not os.path.isfile(path):
            return None
        with open(path, "rb") as f:
            head = f.read(12)
    except OSError:
        return None
    if len(head) == 12 and head[:4] == b"RIFF" and head[8:] == b"WEBP":
        return "webp"
    if head[:6] in GIF_SIGNATURES:
        return "gif"
    return "apng" if head[:8] == PNG_SIGNATURE else None


def _load_png_videos(vids: List[List[str]], device, threads: int, entropy: str):
    """load_videos for the PNG videos of a call."""
    import torch
    flat = [p for v in vids for p in v]
    first_of = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
    if entropy == "device":
        raw, raw_off, raw_size = _read_files(flat, threads, pin=True)
        info = png_probe_mem(raw.numpy(), raw_off, raw_size, threads)
        with torch.cuda.device(device):
            raw_d = raw.to(device, non_blocking=True)   # the one upload: every group decodes out of this buffer
    else:
        info = png_probe(flat, threads)
    _refuse(_PNG, flat, info[:, -1])
    keys = [_first_good_key(info[first_of[vi]:first_of[vi + 1]], 3) for vi in range(len(vids))]
    groups: dict = {}
    for vi, key in enumerate(keys):
        if key is not None:
            groups.setdefault(key, []).append(vi)
    results: List[Optional[Tuple]] = [None] * len(vids)
    for key, members in groups.items():
        if entropy == "device":
            idx = np.concatenate([np.arange(first_of[vi], first_of[vi + 1]) for vi in members])
            with torch.cuda.device(device):
                out, status = _png_decode_group_device(raw.numpy(), raw_d, raw_off[idx], raw_size[idx], key, threads)
        else:
            out, status = _png_decode_group([p for vi in members for p in vids[vi]], None, None, None, key, device,
                                            threads)
        o = 0
        for vi in members:
            n = len(vids[vi])
            results[vi] = _keep_decoded(vids[vi], out[o:o + n], status[o:o + n], L.PNG_STATUS, device)
            o += n
    for vi, key in enumerate(keys):
        if key is None:
            results[vi] = _unreadable_video(vids[vi], device)
    return results


def _load_jpeg_videos(vids: List[List[str]], device, threads: int, entropy: str):
    """load_videos for the JPEG videos of a call."""
    import torch
    flat = [p for v in vids for p in v]
    first_of = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
    if entropy == "device":
        raw, raw_off, raw_size = _read_files(flat, threads, pin=True)
        info = probe_mem(raw.numpy(), raw_off, raw_size, threads)
        with torch.cuda.device(device):
            raw_d = raw.to(device, non_blocking=True)   # the one upload: every group decodes out of this buffer
    else:
        info = probe(flat, threads)
    _raise_unsupported(flat, info[:, 5])
    # a video's layout is its first readable frame's; frames of another size get the shape status and are dropped
    keys = [_first_good_key(info[first_of[vi]:first_of[vi + 1]], 5) for vi in range(len(vids))]
    groups: dict = {}
    for vi, key in enumerate(keys):
        if key is not None:
            groups.setdefault(key, []).append(vi)
    results: List[Optional[Tuple]] = [None] * len(vids)
    for key, members in groups.items():
        lay = make_layout(*key)
        if entropy == "device":
            idx = np.concatenate([np.arange(first_of[vi], first_of[vi + 1]) for vi in members])
            with torch.cuda.device(device):
                out, status = _decode_group_device(raw_d, raw_off[idx], raw_size[idx], lay)
        else:
            out, status = _decode_group([p for vi in members for p in vids[vi]], lay, device, threads)
        o = 0
        for vi in members:
            n = len(vids[vi])
            results[vi] = _keep_decoded(vids[vi], out[o:o + n], status[o:o + n], L.JPEG_STATUS, device)
            o += n
    for vi, key in enumerate(keys):
        if key is None:
            results[vi] = _unreadable_video(vids[vi], device)
    return results


def load_frames(paths_or_dir: Union[PathLike, Sequence[PathLike]], device=None, threads: int = 0,
                entropy: str = "host"):
    """load_frames_from_images (extract_mesh.py:72-82) on the GPU.  paths_or_dir: a frame folder (its *.jpg files in
    sorted order; its *.png files when it has no *.jpg), a list of JPEG paths, or of PNG paths, or the path of an
    animated GIF, of a lossless WebP file or of an animated PNG, whose frames are the video's frames, or a folder or
    list of still WebP frames.
    Returns (frames, kept): uint8 [F', H, W, 3] RGB on `device` (default: the
    current GPU when there is one, else the CPU) and the indices of the frames that decoded.  A frame that fails to
    decode is dropped with a log message, as the reference drops a None from cv2.imread; an unsupported kind of JPEG
    raises UnsupportedJpegError naming the kind and the file.  entropy: where Huffman decoding runs, "host" or "device"
    (load_videos)."""
    return load_videos([paths_or_dir], device=device, threads=threads, entropy=entropy)[0]
