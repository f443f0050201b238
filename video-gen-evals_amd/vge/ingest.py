"""On-disk feature ingest on libvge's native decoder (include/vge_ingest.h).

The reference reads every video with np.load (utils.py:383-424: the npz of extract_mesh.py:35-43 and the
keypoints.npy), in DataLoader worker processes.  Here one call decodes a whole list of videos with a pool
of native threads: the zip central directory is parsed and each member raw-deflate inflated straight into
the frame-store arrays (vge.data.FrameStore), allocated in pinned host memory when a GPU is present so the
upload to HBM is a plain DMA.

    load_frame_store_native(items, keypoint_dir, require_kp)   -> FrameStore   (same contents as
                                                                   eval.load_frame_store's numpy reader)
    load_device_frame_store(items, keypoint_dir, require_kp, device) -> ops.DeviceFrameStore: the same contents in
                                                                   HBM, inflated on the device from the raw file bytes
    save_sidecar(store, path) / load_sidecar(path)             -> a packed, uncompressed frame-store file:
                                                                   repeated evaluations skip zlib entirely

Error behaviour follows vge.data.load_clip: a missing keypoints.npy raises FileNotFoundError when
require_kp (utils.py:416-417) and leaves the video without keypoints otherwise (utils.py:669-678); an
unreadable keypoints.npy raises RuntimeError when require_kp; an unreadable npz raises RuntimeError.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as L
from .data import FrameStore, VideoItem, keypoint_path

SIDECAR_MAGIC = b"VGEFS001"


def _alloc(shape, pinned: bool) -> np.ndarray:
    if pinned:
        return torch.empty(shape, dtype=torch.float32, pin_memory=True).numpy()
    return np.empty(shape, np.float32)


def _cstrs(strs):
    arr = (C.c_char_p * len(strs))()
    arr[:] = [None if s is None else s.encode() for s in strs]
    return arr


def _keypoint_paths(items, keypoint_dir):
    kps = [None] * len(items)
    if keypoint_dir is not None:
        for i, it in enumerate(items):
            kps[i] = keypoint_path(keypoint_dir, it.cls, os.path.splitext(os.path.basename(it.path))[0])
    return kps


def _probed_lengths(info, npz, kps, keypoint_dir, require_kp):
    """The probe's verdicts as load_clip's exceptions -> (frames per video, keypoint frames per video, vit dim, the
    videos whose keypoint file is unreadable and tolerated: they go on without keypoints)."""
    n = len(npz)
    lens, klens, dropped = [], [], []
    for i in range(n):
        st, kf = info[i].status, info[i].kp_frames
        if st in (1, 7, 8):
            raise RuntimeError(f"vge_ingest: cannot read '{npz[i]}' ({L.INGEST_STATUS.get(st, st)})")
        if st == 9:  # keypoints.npy present but unreadable
            if require_kp:
                raise RuntimeError(f"Failed to load keypoints from '{kps[i]}' for video "
                                   f"'{os.path.splitext(os.path.basename(npz[i]))[0]}'")
            kf = -1
            dropped.append(i)
        if kf < 0 and keypoint_dir is not None and require_kp:
            stem = os.path.splitext(os.path.basename(npz[i]))[0]
            raise FileNotFoundError(f"Expected keypoints at '{kps[i]}' for video '{stem}' but file does not exist.")
        lens.append(int(info[i].n_frames))
        klens.append(max(int(kf), 0))
    vit_dim = int(info[0].vit_dim) if n else 1024
    if any(int(info[i].vit_dim) != vit_dim for i in range(n)):
        raise RuntimeError("vge_ingest: videos with different vit dims cannot share one frame store")
    return lens, klens, vit_dim, dropped


def _video_table(lens, klens) -> np.ndarray:
    videos = np.zeros((len(lens), 4), np.int32)
    off = koff = 0
    for i in range(len(lens)):
        videos[i] = (off, lens[i], koff, klens[i])
        off += lens[i]
        koff += klens[i]
    return videos


def load_frame_store_native(items: Sequence[VideoItem], keypoint_dir: Optional[str], require_kp: bool,
                            threads: int = 0, pinned: Optional[bool] = None) -> FrameStore:
    lib = L.load()
    n = len(items)
    if pinned is None:
        pinned = torch.cuda.is_available()
    npz = [it.path for it in items]
    kps = _keypoint_paths(items, keypoint_dir)
    c_npz, c_kp = _cstrs(npz), _cstrs(kps)
    info = (L.ClipInfo * max(n, 1))()
    lib.vge_ingest_probe(c_npz, c_kp, n, threads, info)
    lens, klens, vit_dim, dropped = _probed_lengths(info, npz, kps, keypoint_dir, require_kp)
    for i in dropped:
        kps[i] = None
    F, Fk = sum(lens), sum(klens)
    store = FrameStore(pose=_alloc((F, 207), pinned), gori=_alloc((F, 9), pinned), betas=_alloc((F, 10), pinned),
                       vit=_alloc((F, vit_dim), pinned), kp=_alloc((max(Fk, 1), 120), pinned),
                       videos=_video_table(lens, klens), names=[it.name for it in items],
                       classes=[it.cls for it in items])
    status = np.zeros(max(n, 1), np.int32)
    c_kp = _cstrs(kps)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.vge_ingest_decode(c_npz, c_kp, n, threads, ptr(store.videos), vit_dim, ptr(store.pose),
                               ptr(store.gori), ptr(store.betas), ptr(store.vit), ptr(store.kp), ptr(status))
    if rc != 0:
        bad = int(np.flatnonzero(status[:n])[0])
        raise RuntimeError(f"vge_ingest: decoding '{npz[bad]}' failed ({L.INGEST_STATUS.get(int(status[bad]))})")
    return store


# ----------------------------------------------------------------------------- device inflate

FILE_ALIGN = 16  # files start on 16-byte boundaries of the packed buffer: the kernel stages aligned dwords


def read_video_files(npz: Sequence[str], kps: Sequence[Optional[str]], threads: int = 0, pinned: Optional[bool] = None,
                     tail_bytes: int = 0):
    """The raw files of n videos in one (pinned) buffer, as vge_ingest_*_mem take them: entry 2i the npz, 2i + 1 the
    keypoint file (size -1 when there is none).  -> (uint8 tensor [file bytes + tail_bytes], offsets, sizes [2n] int64,
    file bytes); the tail is the caller's (the descriptors travel in it)."""
    lib = L.load()
    n = len(npz)
    if pinned is None:
        pinned = torch.cuda.is_available()
    slots = [2 * i for i in range(n)] + [2 * i + 1 for i in range(n) if kps[i] is not None and os.path.exists(kps[i])]
    paths = [npz[s // 2] if s % 2 == 0 else kps[s // 2] for s in slots]
    fsz = np.zeros(max(len(paths), 1), np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lib.vge_jpeg_file_sizes(_cstrs(paths), len(paths), threads, ptr(fsz))
    sizes = np.full(2 * n, -1, np.int64)
    offsets = np.zeros(2 * n, np.int64)
    pos = 0
    foff = np.zeros(max(len(paths), 1), np.int64)
    for k, s in enumerate(slots):
        sizes[s], offsets[s], foff[k] = fsz[k], pos, pos
        pos = (pos + int(fsz[k]) + FILE_ALIGN - 1) // FILE_ALIGN * FILE_ALIGN
    buf = torch.empty(max(pos + tail_bytes, 1), dtype=torch.uint8, pin_memory=bool(pinned))
    lib.vge_jpeg_read_files(_cstrs(paths), len(paths), threads, ptr(foff), ptr(fsz), buf.data_ptr(), pos, None)
    return buf, offsets, sizes, pos


def read_item_files(items: Sequence[VideoItem], keypoint_dir: Optional[str], threads: int = 0):
    """The host half of load_device_frame_store that needs no GPU: the raw files of `items` in one pinned buffer with
    room for the stream descriptors behind them (pass the result as `raw`, e.g. from a background thread)."""
    npz = [it.path for it in items]
    kps = _keypoint_paths(items, keypoint_dir)
    return read_video_files(npz, kps, threads, tail_bytes=5 * len(items) * C.sizeof(L.InflateDesc) + 8)


def load_device_frame_store(items: Sequence[VideoItem], keypoint_dir: Optional[str], require_kp: bool, device,
                            threads: int = 0, raw=None, timings: Optional[dict] = None):
    """load_frame_store_native + DeviceFrameStore.from_host without the host decode: the raw .npz / .npy bytes are
    read into one pinned buffer, planned on the host (central directories and npy headers only), uploaded once
    together with the stream descriptors and inflated on the device straight into the frame-store rows
    (csrc/vge_inflate.hip).  Same contents, same exceptions.  raw: read_item_files' result when the files were read
    ahead.  timings (a dict, for tools/bench_ingest.py): receives read_s, plan_s (probe + plan), upload_ms and kernel_ms
    (device events; taking them adds a synchronisation) and the byte counts."""
    import time
    t0 = time.perf_counter()
    from .ops import DeviceFrameStore
    lib = L.load()
    n = len(items)
    device = torch.device(device)
    npz = [it.path for it in items]
    kps = _keypoint_paths(items, keypoint_dir)
    buf, offsets, sizes, nbytes = raw if raw is not None else read_item_files(items, keypoint_dir, threads)
    t1 = time.perf_counter()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    info = (L.ClipInfo * max(n, 1))()
    lib.vge_ingest_probe_mem(buf.data_ptr(), nbytes, ptr(offsets), ptr(sizes), n, threads, info)
    lens, klens, vit_dim, dropped = _probed_lengths(info, npz, kps, keypoint_dir, require_kp)
    for i in dropped:
        sizes[2 * i + 1] = -1
    videos = _video_table(lens, klens)
    F, Fk = sum(lens), sum(klens)
    desc_at = (nbytes + 7) // 8 * 8
    descs = (L.InflateDesc * max(5 * n, 1)).from_address(buf.data_ptr() + desc_at)
    ws_bytes = C.c_int64(8)
    rc = lib.vge_ingest_plan_mem(buf.data_ptr(), nbytes, ptr(offsets), ptr(sizes), n, threads, ptr(videos), vit_dim,
                                 descs, info, C.byref(ws_bytes))
    if rc != 0:
        bad = next(i for i in range(n) if info[i].status != 0)
        raise RuntimeError(f"vge_ingest: decoding '{npz[bad]}' failed ({L.INGEST_STATUS.get(int(info[bad].status))})")
    t2 = time.perf_counter()
    with torch.cuda.device(device):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timings is not None else None
        if ev:
            ev[0].record()
        dbuf = buf.to(device, non_blocking=True)  # the one upload: file bytes and descriptors
        if ev:
            ev[1].record()
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)  # noqa: E731
        store = DeviceFrameStore(pose=f32(F, 207), gori=f32(F, 9), betas=f32(F, 10), vit=f32(F, vit_dim),
                                 kp=f32(Fk, 120) if Fk else torch.zeros(1, 120, device=device),
                                 videos=torch.from_numpy(videos).to(device), host_videos=videos,
                                 names=[it.name for it in items], classes=[it.cls for it in items])
        work = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=device)
        status = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        rc = lib.vge_ingest_decode_device(dbuf.data_ptr(), nbytes, dbuf.data_ptr() + desc_at, 5 * n, n, F, max(Fk, 1),
                                          vit_dim, store.pose.data_ptr(), store.gori.data_ptr(),
                                          store.betas.data_ptr(), store.vit.data_ptr(), store.kp.data_ptr(),
                                          work.data_ptr(), int(ws_bytes.value), status.data_ptr(),
                                          torch.cuda.current_stream(device).cuda_stream)
        L.check(rc, "vge_ingest_decode_device")
        if ev:
            ev[2].record()
        st = status[:n].cpu().numpy()  # waits for the kernels; buf, dbuf and work are free from here on
        if ev:
            timings.update(read_s=t1 - t0, plan_s=t2 - t1, upload_ms=ev[0].elapsed_time(ev[1]),
                           kernel_ms=ev[1].elapsed_time(ev[2]), file_bytes=int(nbytes), frames=int(F))
    if st.any():
        bad = int(np.flatnonzero(st)[0])
        raise RuntimeError(f"vge_ingest: decoding '{npz[bad]}' failed ({L.INGEST_STATUS.get(int(st[bad]))})")
    return store


# ----------------------------------------------------------------------------- packed sidecar

_ARRAYS = ("pose", "gori", "betas", "vit", "kp", "videos")


def _layout(meta: dict, data_start: int):
    offs, pos = {}, data_start
    for k in _ARRAYS:
        spec = meta["arrays"][k]
        pos = (pos + 4095) // 4096 * 4096
        offs[k] = pos
        pos += int(np.prod(spec["shape"])) * np.dtype(spec["dtype"]).itemsize
    return offs


def save_sidecar(store: FrameStore, path: str) -> None:
    """One uncompressed file: magic, u64 header length, JSON header (names, classes, shapes), then the
    arrays in _ARRAYS order, each starting on a 4 KiB boundary."""
    arrays = {k: np.ascontiguousarray(getattr(store, k)) for k in _ARRAYS}
    meta = {"names": list(store.names), "classes": list(store.classes),
            "arrays": {k: {"shape": list(a.shape), "dtype": a.dtype.str} for k, a in arrays.items()}}
    head = json.dumps(meta).encode()
    offs = _layout(meta, len(SIDECAR_MAGIC) + 8 + len(head))
    with open(path, "wb") as f:
        f.write(SIDECAR_MAGIC)
        f.write(np.uint64(len(head)).tobytes())
        f.write(head)
        for k in _ARRAYS:
            f.seek(offs[k])
            f.write(arrays[k].tobytes())


def load_sidecar(path: str, pinned: Optional[bool] = None) -> FrameStore:
    if pinned is None:
        pinned = torch.cuda.is_available()
    with open(path, "rb") as f:
        if f.read(len(SIDECAR_MAGIC)) != SIDECAR_MAGIC:
            raise RuntimeError(f"'{path}' is not a vge frame-store sidecar")
        hl = int(np.frombuffer(f.read(8), np.uint64)[0])
        meta = json.loads(f.read(hl))
        offs = _layout(meta, len(SIDECAR_MAGIC) + 8 + hl)
        out = {}
        for k in _ARRAYS:
            spec = meta["arrays"][k]
            a = (_alloc(tuple(spec["shape"]), pinned) if spec["dtype"] == "<f4"
                 else np.empty(tuple(spec["shape"]), np.dtype(spec["dtype"])))
            f.seek(offs[k])
            if f.readinto(memoryview(a).cast("B")) != a.nbytes:
                raise RuntimeError(f"'{path}': truncated array {k}")
            out[k] = a
    return FrameStore(names=meta["names"], classes=meta["classes"], **out)
