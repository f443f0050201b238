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
from pathlib import Path
from typing import List, Optional, Sequence, Tuple, Union

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


# ---- PNG frames (include/vge_png.h)

def _png_rows(info, n: int) -> np.ndarray:
    return np.array([[i.width, i.height, i.color_type, i.bit_depth, i.interlace, i.n_idat, i.idat_bytes, i.status]
                     for i in info[:n]], dtype=np.int64).reshape(-1, 8)


def png_probe(paths: Sequence[PathLike], threads: int = 0) -> np.ndarray:
    """Headers only: int64 [n, 8] rows of (width, height, colour type, bit depth, interlace, IDAT chunks, IDAT bytes,
    status) (vge_png_probe)."""
    paths = [os.fspath(p) for p in paths]
    info = (L.PngInfo * max(len(paths), 1))()
    if paths:
        L.load().vge_png_probe(_paths_array(paths), len(paths), int(threads), info)
    return _png_rows(info, len(paths))


def png_probe_mem(data: np.ndarray, offsets: np.ndarray, sizes: np.ndarray, threads: int = 0) -> np.ndarray:
    """png_probe() for files in host memory: file i is data[offsets[i]:offsets[i] + sizes[i]] (vge_png_probe_mem)."""
    n = len(offsets)
    info = (L.PngInfo * max(n, 1))()
    if n:
        offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
        L.load().vge_png_probe_mem(data.ctypes.data, data.size, offsets.ctypes.data, sizes.ctypes.data, n,
                                   int(threads), info)
    return _png_rows(info, n)


def _raise_unsupported_png(names, statuses) -> None:
    for p, s in zip(names, statuses):
        if int(s) in L.PNG_UNSUPPORTED:
            raise UnsupportedPngError(f"{p}: unsupported PNG: {L.PNG_UNSUPPORTED[int(s)]} ({L.PNG_STATUS[int(s)]})")


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


# ---- GIF videos (include/vge_gif.h)

def _gif_rows(info, n: int) -> np.ndarray:
    return np.array([[i.width, i.height, i.n_frames, i.lzw_bytes, i.n_blocks, i.status] for i in info[:n]],
                    dtype=np.int64).reshape(-1, 6)


def gif_probe(paths: Sequence[PathLike], threads: int = 0) -> np.ndarray:
    """Headers and block structure only: int64 [n, 6] rows of (screen width, screen height, frames, LZW bytes, data
    sub-blocks, status) (vge_gif_probe)."""
    paths = [os.fspath(p) for p in paths]
    info = (L.GifInfo * max(len(paths), 1))()
    if paths:
        L.load().vge_gif_probe(_paths_array(paths), len(paths), int(threads), info)
    return _gif_rows(info, len(paths))


def gif_probe_mem(data: np.ndarray, offsets: np.ndarray, sizes: np.ndarray, threads: int = 0) -> np.ndarray:
    """gif_probe() for files in host memory: file i is data[offsets[i]:offsets[i] + sizes[i]] (vge_gif_probe_mem)."""
    n = len(offsets)
    info = (L.GifInfo * max(n, 1))()
    if n:
        offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
        L.load().vge_gif_probe_mem(data.ctypes.data, data.size, offsets.ctypes.data, sizes.ctypes.data, n,
                                   int(threads), info)
    return _gif_rows(info, n)


def _raise_unsupported_gif(names, statuses) -> None:
    for p, s in zip(names, statuses):
        if int(s) in L.GIF_UNSUPPORTED:
            raise UnsupportedGifError(f"{p}: unsupported GIF: {L.GIF_UNSUPPORTED[int(s)]} ({L.GIF_STATUS[int(s)]})")


def _gif_decode_group(paths, data, offsets, sizes, screen, n_frames: int, device, threads: int):
    """The GIF files of one logical screen on host threads, from paths or (paths None) from files in host memory
    (data: a uint8 CPU tensor) -> (uint8 [n_frames, H, W, 3] tensor on `device`, int32 status [n_frames]):
    vge_gif_decode / vge_gif_decode_mem into pinned memory, then one upload.  n_frames: the probe's sum."""
    import torch
    lib = L.load()
    w, h = screen
    on_gpu = device.type == "cuda"
    out = torch.empty((n_frames, h, w, 3), dtype=torch.uint8, pin_memory=on_gpu)
    status = np.zeros(n_frames, np.int32)
    if paths is not None:
        lib.vge_gif_decode(_paths_array(paths), len(paths), int(threads), w, h, n_frames, out.data_ptr(),
                           status.ctypes.data, None, None)
    else:
        offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
        lib.vge_gif_decode_mem(data.data_ptr(), int(data.numel()), offsets.ctypes.data, sizes.ctypes.data,
                               len(offsets), int(threads), w, h, n_frames, out.data_ptr(), status.ctypes.data, None,
                               None)
    if on_gpu:
        with torch.cuda.device(device):
            out = out.to(device, non_blocking=True)
    return out, status


def _gif_decode_group_device(data_h: np.ndarray, data_d, offsets: np.ndarray, sizes: np.ndarray, screen,
                             n_frames: int, n_blocks: int, threads: int):
    """The GIF files of one logical screen, their bytes both in host memory (data_h, which only the plan's block walk
    reads) and on the GPU (data_d) -> (uint8 [n_frames, H, W, 3] tensor on that GPU, int32 status [n_frames]):
    vge_gif_plan_mem on the host, one upload of the descriptors and segments, vge_gif_decode_device on the current
    stream; the one host synchronisation is the copy of the statuses at the end.  n_frames, n_blocks: the probe's sums."""
    import torch
    lib = L.load()
    dev = data_d.device
    w, h = screen
    offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
    descs = (L.GifDesc * max(n_frames, 1))()
    segs = (L.GifSegment * max(n_blocks, 1))()
    planned = np.zeros(max(n_frames, 1), np.int32)
    n_descs, n_segs, ws_bytes = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    lib.vge_gif_plan_mem(data_h.ctypes.data, data_h.size, offsets.ctypes.data, sizes.ctypes.data, len(offsets),
                         int(threads), w, h, descs, n_frames, C.byref(n_descs), segs, n_blocks, C.byref(n_segs),
                         planned.ctypes.data, None, C.byref(ws_bytes))
    if n_descs.value != n_frames:
        raise L.VgeError("vge_gif_plan_mem: " + lib.vge_last_error().decode(errors="replace"))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        descs_d = torch.frombuffer(descs, dtype=torch.uint8).to(dev)
        segs_d = torch.frombuffer(segs, dtype=torch.uint8).to(dev)
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
        status_d = torch.empty(n_frames, dtype=torch.int32, device=dev)
        out = torch.empty((n_frames, h, w, 3), dtype=torch.uint8, device=dev)
        L.check(lib.vge_gif_decode_device(data_d.data_ptr(), int(data_d.numel()), descs_d.data_ptr(), n_frames,
                                          segs_d.data_ptr(), n_segs.value, n_frames, len(offsets), w, h, ws.data_ptr(),
                                          int(ws.numel()), out.data_ptr(), status_d.data_ptr(), stream.cuda_stream),
                "vge_gif_decode_device")
        status = status_d.cpu().numpy()
    planned = planned[:n_frames]
    return out, np.where(planned != 0, planned, status).astype(np.int32)


def _keep_gif_frames(name, out, status, device):
    """(frames, kept) of one GIF video: the frames in front of the first one that failed."""
    bad = np.flatnonzero(status != 0)
    n = int(bad[0]) if bad.size else len(status)
    if bad.size:
        log.warning("dropping frames %d.. of %s: %s", n, name, L.GIF_STATUS.get(int(status[n]), int(status[n])))
    return out[:n], np.arange(n, dtype=np.int64)


def _empty_video(device):
    import torch
    return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=device), np.zeros(0, np.int64)


def _decode_gif_files(names, paths, raw, raw_off, raw_size, info, device, threads: int, entropy: str):
    """The GIF videos of a call, from paths (host route) or from their bytes in one host tensor `raw` -> one
    (frames, kept) per file.  info: their probe rows.  Files of one logical screen share one call."""
    import torch
    _raise_unsupported_gif(names, info[:, 5])
    results: List[Optional[Tuple]] = [None] * len(names)
    groups: dict = {}
    for i, row in enumerate(info):
        if int(row[2]) > 0 and int(row[5]) != 1:   # a file with frames, of a size the decoders take
            groups.setdefault((int(row[0]), int(row[1])), []).append(i)
        else:
            log.warning("no decodable frame in %s: %s", names[i], L.GIF_STATUS.get(int(row[5]), int(row[5])))
            results[i] = _empty_video(device)
    raw_d = None
    if entropy == "device" and groups:
        with torch.cuda.device(device):
            raw_d = raw.to(device, non_blocking=True)   # the one upload: every group decodes out of this buffer
    for screen, members in groups.items():
        counts = [int(info[i, 2]) for i in members]
        total, blocks = sum(counts), int(sum(info[i, 4] for i in members))
        if entropy == "device":
            with torch.cuda.device(device):
                out, status = _gif_decode_group_device(raw.numpy(), raw_d, raw_off[members], raw_size[members], screen,
                                                       total, blocks, threads)
        elif paths is not None:
            out, status = _gif_decode_group([paths[i] for i in members], None, None, None, screen, total, device,
                                            threads)
        else:
            out, status = _gif_decode_group(None, raw, raw_off[members], raw_size[members], screen, total, device,
                                            threads)
        o = 0
        for i, n in zip(members, counts):
            results[i] = _keep_gif_frames(names[i], out[o:o + n], status[o:o + n], device)
            if results[i][1].size == 0:
                log.warning("no decodable frame in %s", names[i])
            o += n
    return results


def _load_gif_videos(paths: List[str], device, threads: int, entropy: str):
    """load_videos for the GIF videos of a call."""
    if entropy == "device":
        raw, raw_off, raw_size = _read_files(paths, threads, pin=True)
        info = gif_probe_mem(raw.numpy(), raw_off, raw_size, threads)
        return _decode_gif_files(paths, None, raw, raw_off, raw_size, info, device, threads, entropy)
    return _decode_gif_files(paths, paths, None, None, None, gif_probe(paths, threads), device, threads, entropy)


def decode_gifs(data, offsets, device=None, threads: int = 0, entropy: Optional[str] = None):
    """GIF videos packed in host memory -- (data, offsets[F + 1]): file i at data[offsets[i]:offsets[i + 1]] of a
    one-dimensional uint8 CPU tensor -- -> one (frames, kept) per file, as load_videos gives them.  entropy "host" (the
    default without a GPU) decodes on host threads (vge_gif_decode_mem) and uploads the pixels to `device`; entropy
    "device" (the default with one) uploads the file bytes and runs vge_gif_plan_mem and vge_gif_decode_device.  The
    plan walks every sub-block of every file on the host, so a buffer that lives on a GPU is refused, not copied back."""
    import torch
    if not (isinstance(data, torch.Tensor) and data.dtype == torch.uint8 and data.dim() == 1):
        raise ValueError("data must be a one-dimensional uint8 tensor")
    if data.device.type != "cpu":
        raise ValueError("decode_gifs needs the file bytes in host memory: the plan walks every data sub-block on "
                         "the host; pass a CPU tensor (entropy='device' uploads it once)")
    off = np.ascontiguousarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, np.int64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("offsets must be int64 [F + 1]")
    device = _resolve_device(device)
    if entropy is None:
        entropy = "device" if device.type == "cuda" else "host"
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy must be 'host' or 'device', not {entropy!r}")
    if entropy == "device" and device.type != "cuda":
        raise ValueError("entropy='device' needs a GPU")
    F = off.size - 1
    if F == 0:
        return []
    starts, sizes = off[:F].copy(), np.diff(off)
    if (sizes < 0).any() or off[0] < 0 or off[F] > data.numel():
        raise ValueError("offsets must be non-decreasing and inside data")
    data = data.contiguous()
    names = [f"file {i}" for i in range(F)]
    info = gif_probe_mem(data.numpy(), starts, sizes, threads)
    return _decode_gif_files(names, None, data, starts, sizes, info, device, threads, entropy)


# ---- lossless WebP videos and frames (include/vge_webp.h)

def _webp_rows(info, n: int) -> np.ndarray:
    return np.array([[i.width, i.height, i.n_frames, i.vp8l_bytes, i.n_chunks, i.status] for i in info[:n]],
                    dtype=np.int64).reshape(-1, 6)


def webp_probe(paths: Sequence[PathLike], threads: int = 0) -> np.ndarray:
    """Headers and chunk structure only: int64 [n, 6] rows of (canvas width, canvas height, frames, VP8L payload
    bytes, chunks, status) (vge_webp_probe)."""
    paths = [os.fspath(p) for p in paths]
    info = (L.WebpInfo * max(len(paths), 1))()
    if paths:
        L.load().vge_webp_probe(_paths_array(paths), len(paths), int(threads), info)
    return _webp_rows(info, len(paths))


def webp_probe_mem(data: np.ndarray, offsets: np.ndarray, sizes: np.ndarray, threads: int = 0) -> np.ndarray:
    """webp_probe() for files in host memory: file i is data[offsets[i]:offsets[i] + sizes[i]] (vge_webp_probe_mem)."""
    n = len(offsets)
    info = (L.WebpInfo * max(n, 1))()
    if n:
        offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
        L.load().vge_webp_probe_mem(data.ctypes.data, data.size, offsets.ctypes.data, sizes.ctypes.data, n,
                                    int(threads), info)
    return _webp_rows(info, n)


def _raise_unsupported_webp(names, statuses) -> None:
    for p, s in zip(names, statuses):
        if int(s) in L.WEBP_UNSUPPORTED:
            raise UnsupportedWebpError(
                f"{p}: unsupported WebP: {L.WEBP_UNSUPPORTED[int(s)]} ({L.WEBP_STATUS[int(s)]})")


def _webp_decode_group(paths, data, offsets, sizes, canvas, n_frames: int, device, threads: int):
    """The WebP files of one canvas on host threads, from paths or (paths None) from files in host memory (data: a
    uint8 CPU tensor) -> (uint8 [n_frames, H, W, 3] tensor on `device`, int32 status [n_frames]): vge_webp_decode /
    vge_webp_decode_mem into pinned memory, then one upload.  n_frames: the probe's sum."""
    import torch
    lib = L.load()
    w, h = canvas
    on_gpu = device.type == "cuda"
    out = torch.empty((n_frames, h, w, 3), dtype=torch.uint8, pin_memory=on_gpu)
    status = np.zeros(n_frames, np.int32)
    if paths is not None:
        lib.vge_webp_decode(_paths_array(paths), len(paths), int(threads), w, h, n_frames, out.data_ptr(),
                            status.ctypes.data, None, None)
    else:
        offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
        lib.vge_webp_decode_mem(data.data_ptr(), int(data.numel()), offsets.ctypes.data, sizes.ctypes.data,
                                len(offsets), int(threads), w, h, n_frames, out.data_ptr(), status.ctypes.data, None,
                                None)
    if on_gpu:
        with torch.cuda.device(device):
            out = out.to(device, non_blocking=True)
    return out, status


def _webp_decode_group_device(data_h: np.ndarray, data_d, offsets: np.ndarray, sizes: np.ndarray, canvas,
                              n_frames: int, threads: int):
    """The WebP files of one canvas, their bytes both in host memory (data_h, which only the plan's chunk walk reads)
    and on the GPU (data_d) -> (uint8 [n_frames, H, W, 3] tensor on that GPU, int32 status [n_frames]):
    vge_webp_plan_mem on the host, one upload of the descriptors, vge_webp_decode_device on the current stream; the
    one host synchronisation is the copy of the statuses at the end.  n_frames: the probe's sum."""
    import torch
    lib = L.load()
    dev = data_d.device
    w, h = canvas
    offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
    descs = (L.WebpDesc * max(n_frames, 1))()
    planned = np.zeros(max(n_frames, 1), np.int32)
    n_descs, ws_bytes = C.c_int64(0), C.c_int64(0)
    lib.vge_webp_plan_mem(data_h.ctypes.data, data_h.size, offsets.ctypes.data, sizes.ctypes.data, len(offsets),
                          int(threads), w, h, descs, n_frames, C.byref(n_descs), planned.ctypes.data, None,
                          C.byref(ws_bytes))
    if n_descs.value != n_frames:
        raise L.VgeError("vge_webp_plan_mem: " + lib.vge_last_error().decode(errors="replace"))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        descs_d = torch.frombuffer(descs, dtype=torch.uint8).to(dev)
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
        status_d = torch.empty(n_frames, dtype=torch.int32, device=dev)
        out = torch.empty((n_frames, h, w, 3), dtype=torch.uint8, device=dev)
        L.check(lib.vge_webp_decode_device(data_d.data_ptr(), int(data_d.numel()), descs_d.data_ptr(), n_frames,
                                           n_frames, len(offsets), w, h, ws.data_ptr(), int(ws.numel()),
                                           out.data_ptr(), status_d.data_ptr(), stream.cuda_stream),
                "vge_webp_decode_device")
        status = status_d.cpu().numpy()
    planned = planned[:n_frames]
    return out, np.where(planned != 0, planned, status).astype(np.int32)


def _keep_webp_frames(name, out, status, device):
    """(frames, kept) of one WebP video: the frames in front of the first one that failed."""
    bad = np.flatnonzero(status != 0)
    n = int(bad[0]) if bad.size else len(status)
    if bad.size:
        if int(status[n]) in L.WEBP_UNSUPPORTED:   # what only the decoders see: the group capacity
            _raise_unsupported_webp([name], [status[n]])
        log.warning("dropping frames %d.. of %s: %s", n, name, L.WEBP_STATUS.get(int(status[n]), int(status[n])))
    return out[:n], np.arange(n, dtype=np.int64)


def _decode_webp_files(names, paths, raw, raw_off, raw_size, info, device, threads: int, entropy: str):
    """The WebP files of a call, from paths (host route) or from their bytes in one host tensor `raw` -> one
    (frames, kept) per file.  info: their probe rows.  Files of one canvas share one call."""
    import torch
    _raise_unsupported_webp(names, info[:, 5])
    results: List[Optional[Tuple]] = [None] * len(names)
    groups: dict = {}
    for i, row in enumerate(info):
        if int(row[2]) > 0 and int(row[5]) != 1 and int(row[0]) > 0 and int(row[1]) > 0:
            groups.setdefault((int(row[0]), int(row[1])), []).append(i)
        else:
            log.warning("no decodable frame in %s: %s", names[i], L.WEBP_STATUS.get(int(row[5]), int(row[5])))
            results[i] = _empty_video(device)
    raw_d = None
    if entropy == "device" and groups:
        with torch.cuda.device(device):
            raw_d = raw.to(device, non_blocking=True)   # the one upload: every group decodes out of this buffer
    for canvas, members in groups.items():
        counts = [int(info[i, 2]) for i in members]
        total = sum(counts)
        if entropy == "device":
            with torch.cuda.device(device):
                out, status = _webp_decode_group_device(raw.numpy(), raw_d, raw_off[members], raw_size[members],
                                                        canvas, total, threads)
        elif paths is not None:
            out, status = _webp_decode_group([paths[i] for i in members], None, None, None, canvas, total, device,
                                             threads)
        else:
            out, status = _webp_decode_group(None, raw, raw_off[members], raw_size[members], canvas, total, device,
                                             threads)
        o = 0
        for i, n in zip(members, counts):
            results[i] = _keep_webp_frames(names[i], out[o:o + n], status[o:o + n], device)
            if results[i][1].size == 0:
                log.warning("no decodable frame in %s", names[i])
            o += n
    return results


def _load_webp_files(paths: List[str], device, threads: int, entropy: str):
    """One (frames, kept) per WebP file of a call."""
    if entropy == "device":
        raw, raw_off, raw_size = _read_files(paths, threads, pin=True)
        info = webp_probe_mem(raw.numpy(), raw_off, raw_size, threads)
        return _decode_webp_files(paths, None, raw, raw_off, raw_size, info, device, threads, entropy)
    return _decode_webp_files(paths, paths, None, None, None, webp_probe(paths, threads), device, threads, entropy)


def _load_webp_still_videos(vids: List[List[str]], device, threads: int, entropy: str):
    """load_videos for the videos that are folders or lists of still WebP frames: every file is one frame, and all
    frames of a video have one size (a file of another size is refused with a ValueError that names it)."""
    import torch
    flat = [p for v in vids for p in v]
    per_file = _load_webp_files(flat, device, threads, entropy)
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


def decode_webps(data, offsets, device=None, threads: int = 0, entropy: Optional[str] = None):
    """WebP files packed in host memory -- (data, offsets[F + 1]): file i at data[offsets[i]:offsets[i + 1]] of a
    one-dimensional uint8 CPU tensor -- -> one (frames, kept) per file, as load_videos gives them.  entropy "host" (the
    default without a GPU) decodes on host threads (vge_webp_decode_mem) and uploads the pixels to `device`; entropy
    "device" (the default with one) uploads the file bytes and runs vge_webp_plan_mem and vge_webp_decode_device.  The
    plan walks every chunk of every file on the host, so a buffer that lives on a GPU is refused, not copied back."""
    import torch
    if not (isinstance(data, torch.Tensor) and data.dtype == torch.uint8 and data.dim() == 1):
        raise ValueError("data must be a one-dimensional uint8 tensor")
    if data.device.type != "cpu":
        raise ValueError("decode_webps needs the file bytes in host memory: the plan walks every chunk on the host; "
                         "pass a CPU tensor (entropy='device' uploads it once)")
    off = np.ascontiguousarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, np.int64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("offsets must be int64 [F + 1]")
    device = _resolve_device(device)
    if entropy is None:
        entropy = "device" if device.type == "cuda" else "host"
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy must be 'host' or 'device', not {entropy!r}")
    if entropy == "device" and device.type != "cuda":
        raise ValueError("entropy='device' needs a GPU")
    F = off.size - 1
    if F == 0:
        return []
    starts, sizes = off[:F].copy(), np.diff(off)
    if (sizes < 0).any() or off[0] < 0 or off[F] > data.numel():
        raise ValueError("offsets must be non-decreasing and inside data")
    data = data.contiguous()
    names = [f"file {i}" for i in range(F)]
    info = webp_probe_mem(data.numpy(), starts, sizes, threads)
    return _decode_webp_files(names, None, data, starts, sizes, info, device, threads, entropy)


# ---- APNG videos (include/vge_apng.h)

def _apng_rows(info, n: int) -> np.ndarray:
    return np.array([[i.width, i.height, i.color_type, i.bit_depth, i.interlace, i.n_frames, i.default_image,
                      i.n_chunks, i.data_bytes, i.status] for i in info[:n]], dtype=np.int64).reshape(-1, 10)


def apng_probe(paths: Sequence[PathLike], threads: int = 0) -> np.ndarray:
    """Chunk headers only: int64 [n, 10] rows of (canvas width, canvas height, colour type, bit depth, interlace,
    frames, whether frame 0 is a default image outside the animation, non-empty IDAT / fdAT payloads, their bytes,
    status) (vge_apng_probe).  A PNG that is not animated is a video of one frame."""
    paths = [os.fspath(p) for p in paths]
    info = (L.ApngInfo * max(len(paths), 1))()
    if paths:
        L.load().vge_apng_probe(_paths_array(paths), len(paths), int(threads), info)
    return _apng_rows(info, len(paths))


def apng_probe_mem(data: np.ndarray, offsets: np.ndarray, sizes: np.ndarray, threads: int = 0) -> np.ndarray:
    """apng_probe() for files in host memory: file i is data[offsets[i]:offsets[i] + sizes[i]] (vge_apng_probe_mem)."""
    n = len(offsets)
    info = (L.ApngInfo * max(n, 1))()
    if n:
        offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
        L.load().vge_apng_probe_mem(data.ctypes.data, data.size, offsets.ctypes.data, sizes.ctypes.data, n,
                                    int(threads), info)
    return _apng_rows(info, n)


def _apng_decode_group(paths, data, offsets, sizes, key, n_frames: int, device, threads: int):
    """The APNG files of one (canvas width, canvas height, colour type) on host threads, from paths or (paths None)
    from files in host memory (data: a uint8 CPU tensor) -> (uint8 [n_frames, H, W, 3] tensor on `device`, int32
    status [n_frames]): vge_apng_decode / vge_apng_decode_mem into pinned memory, then one upload.  n_frames: the
    probe's sum."""
    import torch
    lib = L.load()
    w, h, ct = key
    on_gpu = device.type == "cuda"
    out = torch.empty((n_frames, h, w, 3), dtype=torch.uint8, pin_memory=on_gpu)
    status = np.zeros(n_frames, np.int32)
    if paths is not None:
        lib.vge_apng_decode(_paths_array(paths), len(paths), int(threads), w, h, ct, n_frames, out.data_ptr(),
                            status.ctypes.data, None, None)
    else:
        offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
        lib.vge_apng_decode_mem(data.data_ptr(), int(data.numel()), offsets.ctypes.data, sizes.ctypes.data,
                                len(offsets), int(threads), w, h, ct, n_frames, out.data_ptr(), status.ctypes.data,
                                None, None)
    if on_gpu:
        with torch.cuda.device(device):
            out = out.to(device, non_blocking=True)
    return out, status


def _apng_decode_group_device(data_h: np.ndarray, data_d, offsets: np.ndarray, sizes: np.ndarray, key, n_frames: int,
                              n_chunks: int, threads: int):
    """The APNG files of one (canvas width, canvas height, colour type), their bytes both in host memory (data_h, which
    only the plan's chunk walk reads) and on the GPU (data_d) -> (uint8 [n_frames, H, W, 3] tensor on that GPU, int32
    status [n_frames]): vge_apng_plan_mem on the host, one upload of the descriptors and segments,
    vge_apng_decode_device on the current stream; the one host synchronisation is the copy of the statuses at the end.
    n_frames, n_chunks: the probe's sums."""
    import torch
    lib = L.load()
    dev = data_d.device
    w, h, ct = key
    offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
    descs = (L.ApngDesc * max(n_frames, 1))()
    segs = (L.ApngSegment * max(n_chunks, 1))()
    planned = np.zeros(max(n_frames, 1), np.int32)
    n_descs, n_segs, ws_bytes = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    lib.vge_apng_plan_mem(data_h.ctypes.data, data_h.size, offsets.ctypes.data, sizes.ctypes.data, len(offsets),
                          int(threads), w, h, ct, descs, n_frames, C.byref(n_descs), segs, n_chunks, C.byref(n_segs),
                          planned.ctypes.data, None, C.byref(ws_bytes))
    if n_descs.value != n_frames:
        raise L.VgeError("vge_apng_plan_mem: " + lib.vge_last_error().decode(errors="replace"))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        descs_d = torch.frombuffer(descs, dtype=torch.uint8).to(dev)
        segs_d = torch.frombuffer(segs, dtype=torch.uint8).to(dev)
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
        status_d = torch.empty(n_frames, dtype=torch.int32, device=dev)
        out = torch.empty((n_frames, h, w, 3), dtype=torch.uint8, device=dev)
        L.check(lib.vge_apng_decode_device(data_d.data_ptr(), int(data_d.numel()), descs_d.data_ptr(), n_frames,
                                           segs_d.data_ptr(), n_segs.value, n_frames, len(offsets), w, h, ct,
                                           ws.data_ptr(), int(ws.numel()), out.data_ptr(), status_d.data_ptr(),
                                           stream.cuda_stream),
                "vge_apng_decode_device")
        status = status_d.cpu().numpy()
    planned = planned[:n_frames]
    return out, np.where(planned != 0, planned, status).astype(np.int32)


def _keep_apng_frames(name, out, status, device):
    """(frames, kept) of one APNG video: the frames in front of the first one that failed."""
    bad = np.flatnonzero(status != 0)
    n = int(bad[0]) if bad.size else len(status)
    if bad.size:
        log.warning("dropping frames %d.. of %s: %s", n, name, L.APNG_STATUS.get(int(status[n]), int(status[n])))
    return out[:n], np.arange(n, dtype=np.int64)


def _decode_apng_files(names, paths, raw, raw_off, raw_size, info, device, threads: int, entropy: str):
    """The APNG videos of a call, from paths (host route) or from their bytes in one host tensor `raw` -> one
    (frames, kept) per file.  info: their probe rows.  Files of one canvas and colour type share one call."""
    import torch
    _raise_unsupported_png(names, info[:, -1])
    results: List[Optional[Tuple]] = [None] * len(names)
    groups: dict = {}
    for i, row in enumerate(info):
        if int(row[5]) > 0 and int(row[-1]) != 1:   # a file with frames, of a size the decoders take
            groups.setdefault((int(row[0]), int(row[1]), int(row[2])), []).append(i)
        else:
            log.warning("no decodable frame in %s: %s", names[i], L.APNG_STATUS.get(int(row[-1]), int(row[-1])))
            results[i] = _empty_video(device)
    raw_d = None
    if entropy == "device" and groups:
        with torch.cuda.device(device):
            raw_d = raw.to(device, non_blocking=True)   # the one upload: every group decodes out of this buffer
    for key, members in groups.items():
        counts = [int(info[i, 5]) for i in members]
        total, chunks = sum(counts), int(sum(info[i, 7] for i in members))
        if entropy == "device":
            with torch.cuda.device(device):
                out, status = _apng_decode_group_device(raw.numpy(), raw_d, raw_off[members], raw_size[members], key,
                                                        total, chunks, threads)
        elif paths is not None:
            out, status = _apng_decode_group([paths[i] for i in members], None, None, None, key, total, device,
                                             threads)
        else:
            out, status = _apng_decode_group(None, raw, raw_off[members], raw_size[members], key, total, device,
                                             threads)
        o = 0
        for i, n in zip(members, counts):
            results[i] = _keep_apng_frames(names[i], out[o:o + n], status[o:o + n], device)
            if results[i][1].size == 0:
                log.warning("no decodable frame in %s", names[i])
            o += n
    return results


def _load_apng_videos(paths: List[str], device, threads: int, entropy: str):
    """load_videos for the APNG videos of a call."""
    if entropy == "device":
        raw, raw_off, raw_size = _read_files(paths, threads, pin=True)
        info = apng_probe_mem(raw.numpy(), raw_off, raw_size, threads)
        return _decode_apng_files(paths, None, raw, raw_off, raw_size, info, device, threads, entropy)
    return _decode_apng_files(paths, paths, None, None, None, apng_probe(paths, threads), device, threads, entropy)


def decode_apngs(data, offsets, device=None, threads: int = 0, entropy: Optional[str] = None):
    """APNG videos packed in host memory -- (data, offsets[F + 1]): file i at data[offsets[i]:offsets[i + 1]] of a
    one-dimensional uint8 CPU tensor -- -> one (frames, kept) per file, as load_videos gives them.  entropy "host" (the
    default without a GPU) decodes on host threads (vge_apng_decode_mem) and uploads the pixels to `device`; entropy
    "device" (the default with one) uploads the file bytes and runs vge_apng_plan_mem and vge_apng_decode_device.  The
    plan walks every chunk of every file on the host, so a buffer that lives on a GPU is refused, not copied back."""
    import torch
    if not (isinstance(data, torch.Tensor) and data.dtype == torch.uint8 and data.dim() == 1):
        raise ValueError("data must be a one-dimensional uint8 tensor")
    if data.device.type != "cpu":
        raise ValueError("decode_apngs needs the file bytes in host memory: the plan walks every chunk on the host; "
                         "pass a CPU tensor (entropy='device' uploads it once)")
    off = np.ascontiguousarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, np.int64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("offsets must be int64 [F + 1]")
    device = _resolve_device(device)
    if entropy is None:
        entropy = "device" if device.type == "cuda" else "host"
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy must be 'host' or 'device', not {entropy!r}")
    if entropy == "device" and device.type != "cuda":
        raise ValueError("entropy='device' needs a GPU")
    F = off.size - 1
    if F == 0:
        return []
    starts, sizes = off[:F].copy(), np.diff(off)
    if (sizes < 0).any() or off[0] < 0 or off[F] > data.numel():
        raise ValueError("offsets must be non-decreasing and inside data")
    data = data.contiguous()
    names = [f"file {i}" for i in range(F)]
    info = apng_probe_mem(data.numpy(), starts, sizes, threads)
    return _decode_apng_files(names, None, data, starts, sizes, info, device, threads, entropy)


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


def _decode_frames_png(data, starts, sizes, names, device, threads: int, entropy: str):
    """decode_frames for PNG files.  The plan walks chunk headers that lie all over a file, so for data on a GPU the
    file bytes are copied to the host once for it (the pixels never are)."""
    import torch
    data_h = data.cpu() if data.device.type == "cuda" else data
    info = png_probe_mem(data_h.numpy(), starts, sizes, threads)
    _raise_unsupported_png(names, info[:, -1])
    key = _first_good_key(info, 3)
    if key is None:
        for p in names:
            log.warning("dropping frame %s: unreadable", p)
        return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=device), np.zeros(0, np.int64)
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
    import torch
    if not (isinstance(data, torch.Tensor) and data.dtype == torch.uint8 and data.dim() == 1):
        raise ValueError("data must be a one-dimensional uint8 tensor")
    off = np.ascontiguousarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, np.int64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("offsets must be int64 [F + 1]")
    data_on_gpu = data.device.type == "cuda"
    if entropy is None:
        entropy = "device" if data_on_gpu else "host"
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy must be 'host' or 'device', not {entropy!r}")
    if entropy == "host" and data_on_gpu:
        raise ValueError("entropy='host' needs data on the CPU")
    device = data.device if data_on_gpu else _resolve_device(device)
    if entropy == "device" and device.type != "cuda":
        raise ValueError("entropy='device' needs a GPU")
    data = data.contiguous()
    F = off.size - 1
    starts, sizes = off[:F].copy(), np.diff(off)
    names = [f"file {i}" for i in range(F)]
    empty = (torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=device), np.zeros(0, np.int64))
    if F == 0:
        return empty
    if (sizes < 0).any() or off[0] < 0 or off[F] > data.numel():
        raise ValueError("offsets must be non-decreasing and inside data")
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
        good = np.flatnonzero(info[:, 5] == 0)
        key = tuple(int(x) for x in info[good[0], :5]) if good.size else None
    if key is None:
        for p in names:
            log.warning("dropping frame %s: unreadable", p)
        return empty
    lay = make_layout(*key)
    if entropy == "device":
        data_d = data if data_on_gpu else data.to(device)
        out, status = _decode_group_device(data_d, starts, sizes, lay)
        _raise_unsupported(names, status)
    else:
        out, status = _decode_group_mem(data, starts, sizes, lay, device, threads)
    for p, s in zip(names, status):
        if s != 0:
            log.warning("dropping frame %s: %s", p, L.JPEG_STATUS.get(int(s), int(s)))
    kept = np.flatnonzero(status == 0)
    if kept.size != F:
        out = out[torch.as_tensor(kept, device=device)]
    return out, kept


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
    is_webp = [isinstance(v, (str, os.PathLike)) and _is_webp_file(os.fspath(v)) for v in videos]
    is_gif = [isinstance(v, (str, os.PathLike)) and not wp and _is_gif_file(os.fspath(v))
              for v, wp in zip(videos, is_webp)]
    is_apng = [isinstance(v, (str, os.PathLike)) and not wp and not g and _is_apng_file(os.fspath(v))
               for v, wp, g in zip(videos, is_webp, is_gif)]
    one_file = [g or wp or a for g, wp, a in zip(is_gif, is_webp, is_apng)]   # a video in one file: no frame list
    vids = [[] if one else _list_video(v) if isinstance(v, (str, os.PathLike)) else [os.fspath(p) for p in v]
            for v, one in zip(videos, one_file)]
    is_png = [_is_png_file(v[0]) if v else False for v in vids]
    is_stills = [bool(v) and _is_webp_file(v[0]) for v in vids]
    results: List[Optional[Tuple]] = [None] * len(vids)
    apngs = [vi for vi, a in enumerate(is_apng) if a]
    if apngs:
        for vi, r in zip(apngs, _load_apng_videos([os.fspath(videos[vi]) for vi in apngs], device, threads, entropy)):
            results[vi] = r
    gifs = [vi for vi, g in enumerate(is_gif) if g]
    if gifs:
        for vi, r in zip(gifs, _load_gif_videos([os.fspath(videos[vi]) for vi in gifs], device, threads, entropy)):
            results[vi] = r
    webps = [vi for vi, wp in enumerate(is_webp) if wp]
    if webps:
        for vi, r in zip(webps, _load_webp_files([os.fspath(videos[vi]) for vi in webps], device, threads, entropy)):
            results[vi] = r
    stills = [vi for vi, k in enumerate(is_stills) if k]
    if stills:
        for vi, r in zip(stills, _load_webp_still_videos([vids[vi] for vi in stills], device, threads, entropy)):
            results[vi] = r
    for png, load in ((False, _load_jpeg_videos), (True, _load_png_videos)):
        which = [vi for vi, k in enumerate(is_png) if k == png and not one_file[vi] and not is_stills[vi]]
        if which:
            for vi, r in zip(which, load([vids[vi] for vi in which], device, threads, entropy)):
                results[vi] = r
    return results


def _list_video(folder: PathLike) -> List[str]:
    """A frame folder's files: its *.jpg, or when it has none its *.png, or when it has neither its *.webp, in sorted
    order."""
    return list_frames(folder) or list_frames(folder, ext=".png") or list_frames(folder, ext=".webp")


def _is_webp_file(path: str) -> bool:
    """A path to a regular file that begins RIFF....WEBP: a WebP video or still."""
    try:
        if not os.path.isfile(path):
            return False
        with open(path, "rb") as f:
            head = f.read(12)
        return len(head) == 12 and head[:4] == b"RIFF" and head[8:] == b"WEBP"
    except OSError:
        return False


def _is_gif_file(path: str) -> bool:
    """A path to a regular file whose first six bytes are a GIF signature: a GIF video."""
    try:
        if not os.path.isfile(path):
            return False
        with open(path, "rb") as f:
            return f.read(6) in GIF_SIGNATURES
    except OSError:
        return False


def _is_apng_file(path: str) -> bool:
    """A path to a regular file with the PNG signature: an APNG video (a still PNG is a video of one frame)."""
    try:
        return os.path.isfile(path) and _is_png_file(path)
    except OSError:
        return False


def _is_png_file(path: str) -> bool:
    try:
        with open(path, "rb") as f:
            return f.read(8) == PNG_SIGNATURE
    except OSError:
        return False


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
    _raise_unsupported_png(flat, info[:, -1])
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
            for p in vids[vi]:
                log.warning("dropping frame %s: unreadable", p)
            results[vi] = (torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=device), np.zeros(0, np.int64))
    return results


def _load_jpeg_videos(vids: List[List[str]], device, threads: int, entropy: str):
    """load_videos for the JPEG videos of a call."""
    import torch
    flat = [p for v in vids for p in v]
    if entropy == "device":
        raw, raw_off, raw_size = _read_files(flat, threads, pin=True)
        info = probe_mem(raw.numpy(), raw_off, raw_size, threads)
        with torch.cuda.device(device):
            raw_d = raw.to(device, non_blocking=True)   # the one upload: every group decodes out of this buffer
        first_of = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
    else:
        info = probe(flat, threads)
    _raise_unsupported(flat, info[:, 5])
    # a video's layout is its first readable frame's; frames of another size get the shape status and are dropped
    groups, keys, f0 = {}, [], 0
    for vi, v in enumerate(vids):
        rows = info[f0:f0 + len(v)]
        good = np.flatnonzero(rows[:, 5] == 0)
        key = tuple(int(x) for x in rows[good[0], :5]) if good.size else None
        keys.append(key)
        if key is not None:
            groups.setdefault(key, []).append(vi)
        f0 += len(v)
    results: List[Optional[Tuple]] = [None] * len(vids)
    for key, members in groups.items():
        lay = make_layout(*key)
        paths = [p for vi in members for p in vids[vi]]
        if entropy == "device":
            idx = np.concatenate([np.arange(first_of[vi], first_of[vi + 1]) for vi in members])
            with torch.cuda.device(device):
                out, status = _decode_group_device(raw_d, raw_off[idx], raw_size[idx], lay)
        else:
            out, status = _decode_group(paths, lay, device, threads)
        o = 0
        for vi in members:
            n = len(vids[vi])
            st = status[o:o + n]
            for p, s in zip(vids[vi], st):
                if s != 0:
                    log.warning("dropping frame %s: %s", p, L.JPEG_STATUS.get(int(s), int(s)))
            kept = np.flatnonzero(st == 0)
            fr = out[o:o + n]
            if kept.size != n:
                fr = fr[torch.as_tensor(kept, device=device)]
            results[vi] = (fr, kept)
            o += n
    for vi, key in enumerate(keys):
        if key is None:
            for p in vids[vi]:
                log.warning("dropping frame %s: unreadable", p)
            results[vi] = (torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=device), np.zeros(0, np.int64))
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
