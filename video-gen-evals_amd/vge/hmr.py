"""Per-frame mesh extraction (TokenHMR) on the GPU: the host side of include/vge_hmr.h.

Mirrors the reference's extractor boundary -- MeshGenerator.process_video (modifications/mesh_generator.py:
119-171) feeding SMPLTokenDecoderHead (modifications/token_head.py:180-246) and extract_mesh.py:35-43's npz
arrays -- as ``HmrExtractor.process_video(frames)`` returning {pose, global_orient, betas, vit} per frame, and
``extract_into`` writing straight into an HBM frame store for the scoring path (no npz round trip).
The detector gate (mesh_generator.py:103-117) and the crop warp are upstream of this boundary: frames arrive
as 256x256 RGB person crops.  All arithmetic runs in libvge's HIP kernels (vge_vit.hip); there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import asdict, dataclass
from typing import Dict, Optional

import numpy as np
import torch

from . import lib as L
from .ops import _ptr, _stream


@dataclass(frozen=True)
class HmrConfig:
    in_h: int = 256
    in_w: int = 256
    img_h: int = 256
    img_w: int = 192
    patch: int = 16
    pad: int = 2
    embed_dim: int = 1280
    depth: int = 32
    heads: int = 16
    mlp_dim: int = 5120
    dec_dim: int = 1024
    dec_depth: int = 6
    dec_heads: int = 8
    dec_dim_head: int = 64
    dec_mlp: int = 1024
    tok_num: int = 160
    tok_classes: int = 2048
    tok_code_dim: int = 256


TOKENHMR = HmrConfig()  # ViT-H/16 backbone + 6-layer decoder (HMR2 / TokenHMR shapes)


class HmrConfigC(C.Structure):
    _fields_ = [(k, C.c_int) for k in HmrConfig.__dataclass_fields__]


def _cfg_c(cfg: HmrConfig) -> HmrConfigC:
    return HmrConfigC(**asdict(cfg))


_vp, _i32 = C.c_void_p, C.c_int
_SIG = {
    "vge_hmr_create": [C.POINTER(HmrConfigC), C.POINTER(L.TensorView), _i32, C.POINTER(_vp)],
    "vge_hmr_reserve": [_vp, _i32],
    "vge_hmr_destroy": [_vp],
    "vge_hmr_extract": [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp],
    "vge_hmr_profile_begin": [_vp, _i32],
    "vge_hmr_profile_read": [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double)],
    "vge_op_gemm_bf16": [_i32, _vp, C.c_long, _vp, C.c_long, _vp, C.c_long, _vp, _vp, C.c_long, _vp, _i32, _i32, _i32,
                         _i32, _vp],
    "vge_op_gemm_lib": [_i32, _vp, C.c_long, _vp, C.c_long, _vp, C.c_long, _vp, _vp, C.c_long, _i32, _i32, _i32, _vp],
    "vge_op_vit_attention": [_vp, _vp, _i32, _i32, _i32, _vp],
    "vge_hmr_crop": [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp],
    "vge_op_layernorm_bf16": [_vp, _vp, _vp, _vp, _i32, _i32, C.c_float, _vp],
    "vge_op_patchify": [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "vge_op_xattn1": [_vp, C.c_long, _vp, C.c_long, _vp, C.c_long, _i32, _i32, _i32, _vp],
    "vge_op_softmax_rows_bf16": [_vp, _vp, _i32, _i32, _vp],
    "vge_op_hmr_readout": [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp],
    "vge_op_cast_rows_bf16": [_vp, C.c_long, _vp, C.c_long, _i32, _i32, _vp],
    "vge_op_bcast_rows": [_vp, _vp, _i32, _i32, _vp],
    "vge_op_copy_rows": [_vp, C.c_long, _vp, C.c_long, _i32, _i32, _vp],
}


def _sig(lib):
    return L.bind(lib, "hmr", _SIG)


class HmrExtractor(L.NativeModel):
    """One TokenHMR model resident in HBM (bf16 weights) + its activation workspace."""
    PREFIX = "hmr"

    def __init__(self, state_dict: Dict[str, np.ndarray], cfg: HmrConfig = TOKENHMR, device="cuda", max_frames: int = 256):
        self._create(_sig(L.load()), cfg, _cfg_c(cfg), state_dict, device)
        self.reserve(max_frames)

    max_frames = property(lambda self: self._reserved[0])

    def reserve(self, max_frames: int) -> None:
        self._reserve(max_frames)

    def extract(self, frames: torch.Tensor, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """frames: uint8 [F, 256, 256, 3] RGB on the device -> {pose [F,207], global_orient [F,9], betas [F,10],
        vit [F, dec_dim]} float32 (the npz arrays of extract_mesh.py:35-43, flattened rotation matrices)."""
        if frames.dtype != torch.uint8 or frames.dim() != 4 or tuple(frames.shape[1:]) != (self.cfg.in_h, self.cfg.in_w, 3):
            raise L.VgeError(f"frames must be uint8 [F,{self.cfg.in_h},{self.cfg.in_w},3]")
        n = int(frames.shape[0])
        self.reserve(n)
        if out is None:
            dev = frames.device
            out = {"pose": torch.empty((n, 207), device=dev), "global_orient": torch.empty((n, 9), device=dev),
                   "betas": torch.empty((n, 10), device=dev), "vit": torch.empty((n, self.cfg.dec_dim), device=dev)}
        L.check(self.lib.vge_hmr_extract(self.h, _ptr(frames), n, _ptr(out["pose"]), _ptr(out["global_orient"]),
                                         _ptr(out["betas"]), _ptr(out["vit"]), _stream(frames.device)),
                "vge_hmr_extract")
        return out

    def process_video(self, frames: torch.Tensor) -> Dict[int, Dict[str, np.ndarray]]:
        """MeshGenerator.process_video's output shape (mesh_generator.py:160-169): {frame_idx: {pose [23,3,3],
        betas [10], global_orient [1,3,3], vit [1024]}} for frames that passed the (upstream) detector gate."""
        o = self.extract(frames)
        h = {k: v.cpu().numpy() for k, v in o.items()}
        return {i: {"pose": h["pose"][i].reshape(23, 3, 3), "betas": h["betas"][i],
                    "global_orient": h["global_orient"][i].reshape(1, 3, 3), "vit": h["vit"][i]}
                for i in range(frames.shape[0])}

    def profile_read(self):
        return self._profile_read(("gemm", "attention", "layernorm_patchify", "head"))


# ---- op-level entry points (parity tests) ---------------------------------------------------------
EPI = {"bf16": 0, "gelu_bf16": 1, "res_f32": 2, "pe_f32": 3, "f32": 4}


def gemm_bf16(A: torch.Tensor, W: torch.Tensor, epi: str = "bf16", bias=None, res=None, pos=None, tokens: int = 192,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = epilogue(A @ W^T) with A [M,K], W [N,K] bf16 device tensors (the extractor's GEMM kernel)."""
    lib = _sig(L.load())
    M, K = A.shape
    N = W.shape[0]
    if out is None:
        dt = torch.bfloat16 if epi in ("bf16", "gelu_bf16") else torch.float32
        out = torch.empty((M, N), device=A.device, dtype=dt)
    L.check(lib.vge_op_gemm_bf16(EPI[epi], _ptr(A), A.stride(0), _ptr(W), W.stride(0), _ptr(out), out.stride(0),
                                 _ptr(bias), _ptr(res), res.stride(0) if res is not None else 0, _ptr(pos), tokens,
                                 M, N, K, _stream(A.device)), "vge_op_gemm_bf16")
    return out


def gemm_lib(A: torch.Tensor, W: torch.Tensor, epi: str = "bf16", bias=None, res=None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The same product through the library path (hipBLASLt; vge_blaslt.cpp) for the "bf16", "res_f32" and "f32"
    epilogues; raises VGE_ERR_UNSUPPORTED for the others."""
    lib = _sig(L.load())
    M, K = A.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty((M, N), device=A.device, dtype=torch.bfloat16 if epi == "bf16" else torch.float32)
    L.check(lib.vge_op_gemm_lib(EPI[epi], _ptr(A), A.stride(0), _ptr(W), W.stride(0), _ptr(out), out.stride(0),
                                _ptr(bias), _ptr(res), res.stride(0) if res is not None else 0, M, N, K,
                                _stream(A.device)), "vge_op_gemm_lib")
    return out


def vit_attention(qkv: torch.Tensor, heads: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out: bf16, at least [rows, D] contiguous; rows behind qkv's are not written."""
    lib = _sig(L.load())
    rows, D3 = qkv.shape
    D = D3 // 3
    if out is None:
        out = torch.empty((rows, D), device=qkv.device, dtype=torch.bfloat16)
    L.check(lib.vge_op_vit_attention(_ptr(qkv), _ptr(out), rows // 192, D, heads, _stream(qkv.device)),
            "vge_op_vit_attention")
    return out


def layernorm_bf16(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float,
                   out: Optional[torch.Tensor] = None, rows: Optional[int] = None) -> torch.Tensor:
    """out: bf16, at least [rows, D] contiguous; rows behind x's are not written.  rows: the leading rows of x to
    normalise (all of them when None)."""
    lib = _sig(L.load())
    D = x.shape[1]
    rows = x.shape[0] if rows is None else rows
    if out is None:
        out = torch.empty((rows, D), device=x.device, dtype=torch.bfloat16)
    L.check(lib.vge_op_layernorm_bf16(_ptr(x), _ptr(out), _ptr(w), _ptr(b), rows, D, eps, _stream(x.device)),
            "vge_op_layernorm_bf16")
    return out


# The kernels around the GEMMs.  Tensors are passed by their first element with explicit row strides, so a caller may
# hand in a view into a larger buffer (canary rows behind it, a row stride wider than the columns used).
def _dp(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise L.VgeError("vge ops need device (cuda/HIP) tensors")
    return t.data_ptr()


def _op(name: str, *args) -> None:
    L.check(getattr(_sig(L.load()), name)(*args), name)


def patchify(frames: torch.Tensor, out: torch.Tensor, img_w: int = 192, pad: int = 2, patch: int = 16) -> None:
    """frames uint8 [F, in_h, in_w, 3] -> out bf16 [F * 192, 768] patch-embed rows (img_h = in_h)."""
    F_, in_h, in_w = (int(v) for v in frames.shape[:3])
    _op("vge_op_patchify", _ptr(frames), F_, in_h, in_w, in_h, img_w, patch, pad, _dp(out), _stream(frames.device))


def xattn1(q, ldq: int, kv, ldkv: int, out, ldo: int, F_: int, heads: int, ctx: int) -> None:
    _op("vge_op_xattn1", _dp(q), ldq, _dp(kv), ldkv, _dp(out), ldo, F_, heads, ctx, _stream(q.device))


def softmax_rows_bf16(x: torch.Tensor, out: torch.Tensor, rows: int, Cc: int) -> None:
    _op("vge_op_softmax_rows_bf16", _dp(x), _dp(out), rows, Cc, _stream(x.device))


def hmr_readout(rd, ldrd: int, bp, ldbp: int, init_pose, init_betas, pose, gori, betas, F_: int) -> None:
    _op("vge_op_hmr_readout", _dp(rd), ldrd, _dp(bp), ldbp, _dp(init_pose), _dp(init_betas), _dp(pose), _dp(gori),
        _dp(betas), F_, _stream(rd.device))


def cast_rows_bf16(x, ldx: int, y, ldy: int, rows: int, D: int) -> None:
    _op("vge_op_cast_rows_bf16", _dp(x), ldx, _dp(y), ldy, rows, D, _stream(x.device))


def bcast_rows(vec, y, rows: int, D: int) -> None:
    _op("vge_op_bcast_rows", _dp(vec), _dp(y), rows, D, _stream(vec.device))


def copy_rows(x, ldx: int, y, ldy: int, rows: int, D: int) -> None:
    _op("vge_op_copy_rows", _dp(x), ldx, _dp(y), ldy, rows, D, _stream(x.device))


def crop_persons(frames: torch.Tensor, boxes, frame_of=None) -> torch.Tensor:
    """ViTDetDataset's person crop (mesh_generator.py:119-145; vge_hmr_crop): frames uint8 [F, H, W, 3] RGB on the
    device, boxes host float [n, 4] xyxy, frame_of host int [n] (None: crop i from frame i) -> uint8 [n, 256, 256, 3]
    device crops, the input of HmrExtractor.extract."""
    lib = _sig(L.load())
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise L.VgeError("frames must be uint8 [F,H,W,3]")
    b = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 4))
    n = b.shape[0]
    fo = None if frame_of is None else np.ascontiguousarray(np.asarray(frame_of, np.int32).reshape(-1))
    if fo is not None and fo.shape[0] != n:
        raise L.VgeError("frame_of must have one entry per box")
    out = torch.empty((n, 256, 256, 3), dtype=torch.uint8, device=frames.device)
    F_, H_, W_ = (int(v) for v in frames.shape[:3])
    L.check(lib.vge_hmr_crop(_ptr(frames), F_, H_, W_, b.ctypes.data, None if fo is None else fo.ctypes.data, n,
                             _ptr(out), _stream(frames.device)), "vge_hmr_crop")
    return out

