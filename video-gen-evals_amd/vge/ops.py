"""Torch-facing wrappers over libvge.so.  torch supplies device memory and the current HIP stream;
all arithmetic happens in the HIP kernels behind the C ABI (vge.lib)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L
from .data import FrameStore

FEAT_DIM = 2596
D_MODEL = 256
MODALITIES = ("vit", "global", "pose", "beta", "kp2d")
DIMS_RAW = (1024, 9, 207, 10, 120)
DIMS_DIFF = (1024, 3, 69, 10, 120)
# Feature layouts (utils.py:496-514): "kp" when the reference runs with a keypoint_dir (5 modalities, rows of 2596),
# "nokp" when keypoint_dir is None (no kp2d columns: 4 modalities, rows of 2356)
LAYOUTS = {"kp": 0, "nokp": 1}
FEAT_DIMS = {"kp": 2596, "nokp": 2356}
N_MODALITIES = {"kp": 5, "nokp": 4}


def layout_of(keypoint_dir) -> str:
    """The feats layout the reference builds for a keypoint directory (None -> keypoint-less)."""
    return "kp" if keypoint_dir is not None else "nokp"


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise L.VgeError("vge ops need device (cuda/HIP) tensors")
    if not t.is_contiguous():
        raise L.VgeError("vge ops need contiguous tensors")
    return t.data_ptr()


def _stream(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


@dataclass
class DeviceFrameStore:
    """The frame store resident in HBM (see vge.data.FrameStore) + its C view."""
    pose: torch.Tensor
    gori: torch.Tensor
    betas: torch.Tensor
    vit: torch.Tensor
    kp: torch.Tensor
    videos: torch.Tensor            # int32 [V,4] on device
    host_videos: np.ndarray         # int32 [V,4]
    names: list
    classes: list

    @classmethod
    def from_host(cls, st: FrameStore, device) -> "DeviceFrameStore":
        def dev(a, dtype=torch.float32):
            return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
        return cls(pose=dev(st.pose), gori=dev(st.gori), betas=dev(st.betas), vit=dev(st.vit), kp=dev(st.kp),
                   videos=dev(st.videos, torch.int32), host_videos=np.ascontiguousarray(st.videos, np.int32),
                   names=list(st.names), classes=list(st.classes))

    @property
    def n_videos(self) -> int:
        return int(self.host_videos.shape[0])

    def cview(self) -> L.FrameStoreC:
        return L.FrameStoreC(_ptr(self.pose), _ptr(self.gori), _ptr(self.betas), _ptr(self.vit), _ptr(self.kp),
                             _ptr(self.videos), self.n_videos)


def featurize(store: DeviceFrameStore, windows: torch.Tensor, mean: torch.Tensor, std: torch.Tensor,
              out: Optional[torch.Tensor] = None, layout: str = "kp") -> torch.Tensor:
    """WindowDataset._try_one for a batch of windows -> feats [Nw,32,2596] (utils.py:383-516); layout "nokp"
    (keypoint_dir None): feats [Nw,32,2356] and mean/std [2356] in that layout."""
    lib = L.load()
    n = int(windows.shape[0])
    D = FEAT_DIMS[layout]
    if mean.numel() != D or std.numel() != D:
        raise L.VgeError(f"featurize: mean/std must have {D} entries for layout {layout!r}")
    if out is None:
        out = torch.empty((n, 32, D), device=windows.device, dtype=torch.float32)
    elif tuple(out.shape[1:]) != (32, D) or out.shape[0] < n:
        raise L.VgeError(f"featurize: out must be [>= {n}, 32, {D}] for layout {layout!r}")
    if n:
        cv = store.cview()
        L.check(lib.vge_featurize_layout(C.byref(cv), _ptr(windows), n, _ptr(mean), _ptr(std), LAYOUTS[layout],
                                         _ptr(out), _stream(windows.device)), "vge_featurize")
    return out


def stats_accumulate(store: DeviceFrameStore, video_sel: Sequence[int], sums: torch.Tensor, counts: np.ndarray,
                     workspace_tiles: int = 512) -> None:
    """compute_stats_from_npz's float64 sum / sum-of-squares (utils.py:595-744), accumulated into
    sums [2,2596] f64 (device) and counts int64[2] (host)."""
    lib = L.load()
    sel = np.ascontiguousarray(np.asarray(video_sel, np.int32))
    wsb = lib.vge_stats_workspace_bytes(workspace_tiles)
    ws = torch.empty(wsb, dtype=torch.uint8, device=sums.device)
    cnt = (C.c_int64 * 2)(int(counts[0]), int(counts[1]))
    cv = store.cview()
    L.check(lib.vge_stats_accumulate(C.byref(cv), store.host_videos.ctypes.data, sel.ctypes.data, len(sel),
                                      _ptr(sums), cnt, _ptr(ws), wsb, _stream(sums.device)), "vge_stats_accumulate")
    counts[0], counts[1] = cnt[0], cnt[1]


def stats_finalize(sums: torch.Tensor, counts: np.ndarray, layout: str = "kp") -> Tuple[torch.Tensor, torch.Tensor]:
    """mean / std in the layout's feats column order (layout "nokp": [2356], the keypoint-less ModalityStats)."""
    lib = L.load()
    mean = torch.empty(FEAT_DIMS[layout], device=sums.device, dtype=torch.float32)
    std = torch.empty_like(mean)
    cnt = (C.c_int64 * 2)(int(counts[0]), int(counts[1]))
    L.check(lib.vge_stats_finalize_layout(_ptr(sums), cnt, LAYOUTS[layout], _ptr(mean), _ptr(std),
                                          _stream(sums.device)), "vge_stats_finalize")
    return mean, std


COMPUTE = {"f32": 0, "f32x3": 1, "f16": 2}


class Encoder:
    """HumanActionScorer (model.py:102-193) as a libvge encoder handle owning repacked HBM weights.

    compute="f32x3" (default): split-precision 3xfp16 MFMA, f32-class results (~1e-7 from exact f32);
    compute="f32": exact f32 MFMA.  n_modalities 5 (vit, global, pose, beta, kp2d; feats rows of 2596) or 4 (the
    keypoint-less model, feats rows of 2356).  A checkpoint with d_model / time_heads other than 256 / 8 runs on the
    generic exact-f32 kernels (compute "f32" only; d_model 32..256 in steps of 32, head dim <= 64): its embeddings
    are d_model wide."""

    def __init__(self, state_dict: Dict[str, np.ndarray], time_layers: int = 4, time_heads: int = 8,
                 d_model: int = 256, device=None, compute: str = "f32x3", n_modalities: int = 5):
        lib = L.load()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        dims = L.Dims()
        dims.n_modalities = n_modalities
        for i in range(min(n_modalities, 5)):
            dims.dims_raw[i] = DIMS_RAW[i]
            dims.dims_diff[i] = DIMS_DIFF[i]
        dims.d_model, dims.time_layers, dims.time_heads, dims.clip_len = d_model, time_layers, time_heads, 32
        keep = []
        views = (L.TensorView * len(state_dict))()
        for i, (k, v) in enumerate(state_dict.items()):
            a = np.ascontiguousarray(np.asarray(v, np.float32))
            keep.append(a)
            views[i].name = k.encode()
            views[i].data = a.ctypes.data
            views[i].ndim = a.ndim
            for j, s in enumerate(a.shape[:4]):
                views[i].shape[j] = s
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(lib.vge_encoder_create(C.byref(dims), views, len(state_dict), COMPUTE[compute], C.byref(h)),
                    "vge_encoder_create")
        self.compute = compute
        self._h = h
        self._tail = None  # set_tail_stream()
        self._lib = lib
        self.capacity = 0
        self.n_modalities = n_modalities
        self.d_model = int(d_model)
        self.feat_dim = int(lib.vge_encoder_feat_dim(h))
        self.layout = "kp" if self.feat_dim == FEAT_DIM else "nokp"

    def reserve(self, max_windows: int) -> None:
        if max_windows > self.capacity:
            with torch.cuda.device(self.device):
                L.check(self._lib.vge_encoder_reserve(self._h, int(max_windows)), "vge_encoder_reserve")
            self.capacity = int(max_windows)

    def encode(self, feats: torch.Tensor, frame_embed: bool = False, tc: bool = True,
               seq_out: Optional[torch.Tensor] = None, tc_out: Optional[torch.Tensor] = None):
        """feats [B,32,feat_dim] -> (seq_embed [B,d], frame_embeds [B,33,d] | None, tc_window [B] | None), d = d_model.
        seq_out / tc_out: optional contiguous float32 destinations ([B,d] / [B]) written in place."""
        B, T, D = feats.shape
        if D != self.feat_dim:
            raise L.VgeError(f"feats last dim {D} != {self.feat_dim}")
        D_ = self.d_model
        for t, shape in ((seq_out, (B, D_)), (tc_out, (B,))):
            if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()
                                  or t.device != feats.device):
                raise L.VgeError(f"encode: output must be a contiguous float32 {shape} tensor on {feats.device}")
        self.reserve(B)
        seq = seq_out if seq_out is not None else torch.empty((B, D_), device=feats.device, dtype=torch.float32)
        fe = torch.empty((B, T + 1, D_), device=feats.device, dtype=torch.float32) if frame_embed else None
        tcw = (tc_out if tc_out is not None else torch.empty((B,), device=feats.device, dtype=torch.float32)) if tc else None
        L.check(self._lib.vge_encode(self._h, _ptr(feats), B, T, _ptr(seq), _ptr(fe), _ptr(tcw), _stream(feats.device)),
                "vge_encode")
        if self._tail is not None:
            # the outputs are written on the tail stream.  Those allocated here belong to the current stream in the
            # caching allocator's books: record the tail stream on them (a dropped fe / tcw is not reused before the
            # tail stream is done with it) and make the current stream wait for it, so they read as complete there.
            # Caller-provided seq_out / tc_out (and no frame embeddings) keep the overlap: the caller orders them.
            own = [t for t, given in ((seq, seq_out is not None), (fe, False), (tcw, tc_out is not None))
                   if t is not None and not given]
            for t in own:
                t.record_stream(self._tail)
            if own:
                torch.cuda.current_stream(feats.device).wait_stream(self._tail)
        return seq, fe, tcw

    def status(self) -> None:
        """Raise DeviceFaultError if a completed launch raised the encoder's device status word (vge_encoder_status;
        synchronise first to cover launches still in flight)."""
        L.check(self._lib.vge_encoder_status(self._h), "vge_encoder_status")

    def clear_status(self) -> None:
        L.check(self._lib.vge_encoder_clear_status(self._h), "vge_encoder_clear_status")

    def profile_mask(self, event_mask: int) -> None:
        """Stage-boundary events recorded by profiled encodes (bit k = before stage k; 0x3 = the conv stage only)."""
        L.check(self._lib.vge_encoder_profile_mask(self._h, event_mask), "vge_encoder_profile_mask")

    def wait_conv(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Make `stream` (default: the current stream) wait until the conv stage of the last encode() -- the last
        reader of its feats -- has finished (vge_encoder_wait_conv): the next batch can be featurised into the same
        buffer on another stream while this batch's fusion / transformer run."""
        st = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
        L.check(self._lib.vge_encoder_wait_conv(self._h, st), "vge_encoder_wait_conv")

    def set_tail_stream(self, stream: Optional[torch.cuda.Stream]) -> None:
        """Run the stages after the fusion (token GEMM, transformer, outputs / TC) of later encode() calls on `stream`
        (None: back on the encode stream) -- vge_encoder_set_tail_stream.  encode()'s outputs are then complete in
        `stream`'s order; the encode stream is free for the next batch's featurise and conv stage."""
        with torch.cuda.device(self.device):  # its events are created on the encoder's device
            L.check(self._lib.vge_encoder_set_tail_stream(self._h, stream.cuda_stream if stream is not None else None),
                    "vge_encoder_set_tail_stream")
        self._tail = stream

    STAGES = ("conv_encoders", "fusion_pool", "token_gemm", "transformer", "outputs_tc")

    def profile_begin(self, max_calls: int) -> None:
        L.check(self._lib.vge_encoder_profile_begin(self._h, int(max_calls)), "vge_encoder_profile_begin")

    def profile_read(self):
        """-> ({stage: summed ms}, n_calls) for the encode calls since profile_begin."""
        ms = (C.c_double * 5)()
        n = C.c_int(0)
        L.check(self._lib.vge_encoder_profile_read(self._h, ms, C.byref(n)), "vge_encoder_profile_read")
        return dict(zip(self.STAGES, list(ms))), int(n.value)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.vge_encoder_destroy(h)
            except Exception:
                pass
            self._h = None


def tc_windows(frame_embeds: torch.Tensor) -> torch.Tensor:
    lib = L.load()
    B, T1, d = frame_embeds.shape
    out = torch.empty((B,), device=frame_embeds.device, dtype=torch.float32)
    L.check(lib.vge_tc_windows(_ptr(frame_embeds), B, T1, d, _ptr(out), _stream(frame_embeds.device)), "vge_tc_windows")
    return out


def score_videos(seq: torch.Tensor, tc_window: torch.Tensor, video_first_win: torch.Tensor, video_class: torch.Tensor,
                 centroids: Optional[torch.Tensor], out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-video AC (float32) / TC (float64).  out: (ac [V] float32, tc [V] float64) to write instead of new device
    tensors -- device tensors, or pinned (page-locked) host tensors, which the kernel then writes directly over the
    bus (no copy kernels; the values are the host's once the stream is synchronised)."""
    lib = L.load()
    V = int(video_class.shape[0])
    d = int(seq.shape[1])
    if out is not None:
        ac, tc = out
        if (ac.dtype, tc.dtype) != (torch.float32, torch.float64) or ac.numel() < V or tc.numel() < V or \
                not ac.is_contiguous() or not tc.is_contiguous() or \
                any(not t.is_cuda and not t.is_pinned() for t in (ac, tc)):
            raise L.VgeError("score_videos: out must be contiguous (float32, float64) tensors of >= V elements, on the "
                             "device or in pinned host memory")
    else:
        ac = torch.empty((V,), device=seq.device, dtype=torch.float32)
        tc = torch.empty((V,), device=seq.device, dtype=torch.float64)
    if centroids is None:
        centroids = torch.zeros((1, d), device=seq.device, dtype=torch.float32)
    # (a pinned host tensor's address is also its device address: HIP maps page-locked host memory into the GPU's
    # virtual address space at the same address)
    op = lambda t: _ptr(t) if t.is_cuda else t.data_ptr()  # noqa: E731
    L.check(lib.vge_score_videos(_ptr(seq), _ptr(tc_window), _ptr(video_first_win), _ptr(video_class), _ptr(centroids),
                                 V, d, op(ac), op(tc), _stream(seq.device)), "vge_score_videos")
    return ac, tc


def centroid_accumulate(seq: torch.Tensor, class_id: torch.Tensor, sums: torch.Tensor, counts: torch.Tensor) -> None:
    lib = L.load()
    C_, d = sums.shape
    L.check(lib.vge_centroid_accumulate(_ptr(seq), _ptr(class_id), int(seq.shape[0]), C_, d, _ptr(sums), _ptr(counts),
                                        _stream(seq.device)), "vge_centroid_accumulate")


def centroid_finalize(sums: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    lib = L.load()
    C_, d = sums.shape
    out = torch.empty_like(sums)
    L.check(lib.vge_centroid_finalize(_ptr(sums), _ptr(counts), C_, d, _ptr(out), _stream(sums.device)),
            "vge_centroid_finalize")
    return out


# ----------------------------------------------------------------------------- held-out validation loss (vge.validate)

def time_gather(feats: torch.Tensor, src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b,t,:] = feats[b, src[b,t], :] (vge_time_gather): the shuffled / reversed / static windows of
    utils.py:65-95 from one int32 [B,32] index table.  The table's range is checked here (the C caller owns that
    contract): an entry outside [0, 32) is refused."""
    lib = L.load()
    B, T, D = feats.shape
    if feats.dtype != torch.float32 or src.dtype != torch.int32 or tuple(src.shape) != (B, T):
        raise L.VgeError(f"time_gather: feats must be float32 [B,T,D] and src int32 [{B},{T}]")
    if B and (int(src.min()) < 0 or int(src.max()) >= T):
        raise L.VgeError(f"time_gather: src entries must lie in [0, {T})")
    if out is None:
        out = torch.empty_like(feats)
    elif tuple(out.shape) != (B, T, D) or out.dtype != torch.float32 or out.device != feats.device:
        raise L.VgeError(f"time_gather: out must be a float32 [{B},{T},{D}] tensor on {feats.device}")
    L.check(lib.vge_time_gather(_ptr(feats), _ptr(src), B, T, D, _ptr(out), _stream(feats.device)), "vge_time_gather")
    return out


def tcl_loss(emb: torch.Tensor, labels: torch.Tensor, temperature: float = 0.1, k1: float = 5000.0, k2: float = 1.0,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """TCL (losses.py:6-34) of emb [B,d] with int32 labels [B] -> device float64 [1]; NaN when a label appears once
    in the batch, as the reference gives.  out: a float64 device tensor whose first element is written."""
    lib = L.load()
    B, d = emb.shape
    if emb.dtype != torch.float32 or labels.dtype != torch.int32 or labels.numel() != B:
        raise L.VgeError("tcl_loss: emb must be float32 [B,d] and labels int32 [B]")
    if out is None:
        out = torch.empty((1,), device=emb.device, dtype=torch.float64)
    wsb = int(lib.vge_tcl_workspace_bytes(B))
    ws = torch.empty(max(wsb, 8) // 8, dtype=torch.float64, device=emb.device)
    L.check(lib.vge_tcl_loss(_ptr(emb), _ptr(labels), B, d, float(temperature), float(k1), float(k2), _ptr(ws), wsb,
                             _ptr(out), _stream(emb.device)), "vge_tcl_loss")
    return out


def hardneg_loss(anchor: torch.Tensor, neg: torch.Tensor, temperature: float = 0.07,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SupConWithHardNegatives(anchor, anchor, neg) (losses.py:37-56) -> device float64 [1], unweighted."""
    lib = L.load()
    B, d = anchor.shape
    if anchor.dtype != torch.float32 or neg.dtype != torch.float32 or tuple(neg.shape) != (B, d):
        raise L.VgeError("hardneg_loss: anchor and neg must be float32 [B,d]")
    if out is None:
        out = torch.empty((1,), device=anchor.device, dtype=torch.float64)
    L.check(lib.vge_hardneg_loss(_ptr(anchor), _ptr(neg), B, d, float(temperature), _ptr(out),
                                 _stream(anchor.device)), "vge_hardneg_loss")
    return out


def _f32_rows(fn: str, name: str, t: torch.Tensor, shape=None) -> None:
    if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or \
            (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "[B,d]" if shape is None else f"[{shape[0]},{shape[1]}]"
        raise L.VgeError(f"{fn}: {name} must be a contiguous float32 {want} tensor, got {t.dtype} {tuple(t.shape)}")


def tcl_loss_grad(emb: torch.Tensor, labels: torch.Tensor, temperature: float = 0.1, k1: float = 5000.0,
                  k2: float = 1.0, out: Optional[torch.Tensor] = None, grad: Optional[torch.Tensor] = None):
    """tcl_loss and its gradient in one call (vge_tcl_loss_grad) -> (device float64 [1], float32 [B,d]).  The loss has
    tcl_loss's bits; where it is NaN (a label that appears once) the gradient is unspecified."""
    lib = L.load()
    _f32_rows("tcl_loss_grad", "emb", emb)
    B, d = emb.shape
    if labels.dtype != torch.int32 or labels.dim() != 1 or labels.numel() != B or labels.device != emb.device:
        raise L.VgeError(f"tcl_loss_grad: labels must be int32 [{B}] on {emb.device}")
    if out is None:
        out = torch.empty((1,), device=emb.device, dtype=torch.float64)
    if grad is None:
        grad = torch.empty_like(emb)
    else:
        _f32_rows("tcl_loss_grad", "grad", grad, (B, d))
    wsb = int(lib.vge_tcl_grad_workspace_bytes(B))
    ws = torch.empty(max(wsb, 8) // 8, dtype=torch.float64, device=emb.device)
    L.check(lib.vge_tcl_loss_grad(_ptr(emb), _ptr(labels), B, d, float(temperature), float(k1), float(k2), _ptr(ws),
                                  wsb, _ptr(out), _ptr(grad), _stream(emb.device)), "vge_tcl_loss_grad")
    return out, grad


def hardneg_loss_grad(anchor: torch.Tensor, neg: torch.Tensor, temperature: float = 0.07,
                      out: Optional[torch.Tensor] = None, grad_anchor: Optional[torch.Tensor] = None,
                      grad_neg: Optional[torch.Tensor] = None):
    """hardneg_loss and its gradients in one call (vge_hardneg_loss_grad) -> (device float64 [1], grad_anchor
    float32 [B,d], grad_neg float32 [B,d]); anchor is the positive too, and grad_anchor covers both of its uses."""
    lib = L.load()
    _f32_rows("hardneg_loss_grad", "anchor", anchor)
    B, d = anchor.shape
    _f32_rows("hardneg_loss_grad", "neg", neg, (B, d))
    if out is None:
        out = torch.empty((1,), device=anchor.device, dtype=torch.float64)
    if grad_anchor is None:
        grad_anchor = torch.empty_like(anchor)
    else:
        _f32_rows("hardneg_loss_grad", "grad_anchor", grad_anchor, (B, d))
    if grad_neg is None:
        grad_neg = torch.empty_like(anchor)
    else:
        _f32_rows("hardneg_loss_grad", "grad_neg", grad_neg, (B, d))
    L.check(lib.vge_hardneg_loss_grad(_ptr(anchor), _ptr(neg), B, d, float(temperature), _ptr(out), _ptr(grad_anchor),
                                      _ptr(grad_neg), _stream(anchor.device)), "vge_hardneg_loss_grad")
    return out, grad_anchor, grad_neg


def centroid_distance(emb: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
    """|| normalize(emb_i) - centroids[labels[i]] ||_2 (train.py:366-378) -> float32 [n]; NaN where the label is
    outside [0, C)."""
    lib = L.load()
    n, d = emb.shape
    C_ = int(centroids.shape[0])
    if emb.dtype != torch.float32 or labels.dtype != torch.int32 or labels.numel() != n or \
            centroids.dtype != torch.float32 or int(centroids.shape[1]) != d:
        raise L.VgeError("centroid_distance: emb float32 [n,d], labels int32 [n], centroids float32 [C,d]")
    out = torch.empty((n,), device=emb.device, dtype=torch.float32)
    L.check(lib.vge_centroid_distance(_ptr(emb), _ptr(labels), _ptr(centroids), n, C_, d, _ptr(out),
                                      _stream(emb.device)), "vge_centroid_distance")
    return out


def _convblock_args(fn: str, x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, mask: Optional[torch.Tensor],
                    gamma: torch.Tensor, like: Sequence[Tuple[str, torch.Tensor]] = ()) -> Tuple[int, int, int]:
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise L.VgeError(f"{fn}: x must be a contiguous float32 [B,T,C] tensor, got {x.dtype} {tuple(x.shape)}")
    B, T, C_ = x.shape
    for name, t, shape in [("w1", w1, (C_, C_, 5)), ("w2", w2, (C_, C_, 5)), ("gamma", gamma, (C_,))] + \
            [(n, t, (B, T, C_)) for n, t in (("mask", mask),) + tuple(like) if t is not None]:
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != x.device:
            raise L.VgeError(f"{fn}: {name} must be a contiguous float32 {list(shape)} tensor on {x.device}, got "
                             f"{t.dtype} {tuple(t.shape)}")
    return B, T, C_


def _convblock_vector(fn: str, name: str, t: torch.Tensor, n: int, device) -> None:
    if t.dtype != torch.float32 or tuple(t.shape) != (n,) or not t.is_contiguous() or t.device != device:
        raise L.VgeError(f"{fn}: {name} must be a contiguous float32 [{n}] tensor on {device}, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")


def _convblock_workspace(lib, B: int, T: int, C_: int, device) -> Tuple[torch.Tensor, int]:
    wsb = int(lib.vge_convblock_workspace_bytes(B, T, C_))
    return torch.empty(max(wsb, 16) // 4, dtype=torch.float32, device=device), wsb


def convblock_forward(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                      dilation: int, mask: Optional[torch.Tensor] = None, save: bool = True,
                      y: Optional[torch.Tensor] = None, saved=None):
    """One residual conv block (vge_convblock_forward, include/vge.h) on the current stream -> (y, saved), saved =
    (a, u, mean, rstd) for convblock_backward, or None with save=False (nothing is kept).  x [B,T,C] float32; w1, w2
    [C,C,5]; mask [B,T,C] the dropout multiplier or None; y / saved: the tensors to write, or None."""
    lib = L.load()
    a, u, mean, rstd = saved if saved is not None else (None, None, None, None)
    B, T, C_ = _convblock_args("convblock_forward", x, w1, w2, mask, gamma, (("y", y), ("a", a), ("u", u)))
    _convblock_vector("convblock_forward", "beta", beta, C_, x.device)
    if y is None:
        y = torch.empty_like(x)
    if save and saved is None:
        saved = (torch.empty_like(x), torch.empty_like(x), torch.empty(B, dtype=torch.float32, device=x.device),
                 torch.empty(B, dtype=torch.float32, device=x.device))
    a, u, mean, rstd = saved if save else (None, None, None, None)
    if save:
        _convblock_vector("convblock_forward", "mean", mean, B, x.device)
        _convblock_vector("convblock_forward", "rstd", rstd, B, x.device)
    wsb = int(lib.vge_convblock_forward_workspace_bytes(C_))      # the two weight images
    ws = torch.empty(max(wsb, 16) // 4, dtype=torch.float32, device=x.device)
    L.check(lib.vge_convblock_forward(_ptr(x), _ptr(w1), _ptr(w2), _ptr(mask), _ptr(gamma), _ptr(beta), B, T, C_,
                                      int(dilation), _ptr(a), _ptr(u), _ptr(mean), _ptr(rstd), _ptr(y), _ptr(ws), wsb,
                                      _stream(x.device)), "vge_convblock_forward")
    return y, (saved if save else None)


def convblock_backward(dy: torch.Tensor, x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, gamma: torch.Tensor,
                       dilation: int, saved, mask: Optional[torch.Tensor] = None, out=None):
    """The block's backward (vge_convblock_backward) on the current stream -> (dx, dw1, dw2, dgamma, dbeta).  saved:
    convblock_forward's (a, u, mean, rstd) of the same x, weights and mask; out: the five result tensors, or None."""
    lib = L.load()
    a, u, mean, rstd = saved
    B, T, C_ = _convblock_args("convblock_backward", x, w1, w2, mask, gamma, (("dy", dy), ("a", a), ("u", u)))
    _convblock_vector("convblock_backward", "mean", mean, B, x.device)
    _convblock_vector("convblock_backward", "rstd", rstd, B, x.device)
    if out is None:
        out = (torch.empty_like(x), torch.empty_like(w1), torch.empty_like(w2), torch.empty_like(gamma),
               torch.empty_like(gamma))
    dx, dw1, dw2, dgamma, dbeta = out
    _convblock_args("convblock_backward", dx, dw1, dw2, None, dgamma)
    if dx.shape != x.shape or dx.device != x.device:
        raise L.VgeError(f"convblock_backward: dx must be a float32 {list(x.shape)} tensor on {x.device}")
    _convblock_vector("convblock_backward", "dbeta", dbeta, C_, x.device)
    ws, wsb = _convblock_workspace(lib, B, T, C_, x.device)
    L.check(lib.vge_convblock_backward(_ptr(dy), _ptr(x), _ptr(w1), _ptr(w2), _ptr(mask), _ptr(gamma), _ptr(a), _ptr(u),
                                       _ptr(mean), _ptr(rstd), B, T, C_, int(dilation), _ptr(dx), _ptr(dw1), _ptr(dw2),
                                       _ptr(dgamma), _ptr(dbeta), _ptr(ws), wsb, _stream(x.device)),
            "vge_convblock_backward")
    return dx, dw1, dw2, dgamma, dbeta


# the twelve parameter tensors of one temporal layer, in the order of vge_timelayer_forward, with their shapes
TIMELAYER_PARAMS = ("in_proj_weight", "in_proj_bias", "out_proj_weight", "out_proj_bias", "linear1_weight",
                    "linear1_bias", "linear2_weight", "linear2_bias", "norm1_weight", "norm1_bias", "norm2_weight",
                    "norm2_bias")


def _timelayer_shapes(B: int, S: int, D: int, H: int, F_: int) -> Dict[str, Tuple[int, ...]]:
    return {"x": (B, S, D), "y": (B, S, D), "dy": (B, S, D), "dx": (B, S, D),
            "in_proj_weight": (3 * D, D), "in_proj_bias": (3 * D,), "out_proj_weight": (D, D), "out_proj_bias": (D,),
            "linear1_weight": (F_, D), "linear1_bias": (F_,), "linear2_weight": (D, F_), "linear2_bias": (D,),
            "norm1_weight": (D,), "norm1_bias": (D,), "norm2_weight": (D,), "norm2_bias": (D,),
            "m_attn": (B, H, S, S), "m1": (B, S, D), "m_ff": (B, S, F_), "m2": (B, S, D),
            "qkv": (B, S, 3 * D), "u1": (B, S, D), "f": (B, S, F_), "u2": (B, S, D), "stats": (4, B * S)}


TIMELAYER_SAVED = ("qkv", "u1", "f", "u2", "stats")
TIMELAYER_MASKS = ("m_attn", "m1", "m_ff", "m2")


def _timelayer_check(fn: str, x: torch.Tensor, params: Sequence[torch.Tensor], heads: int,
                     named: Sequence[Tuple[str, Optional[torch.Tensor]]]) -> Tuple[int, int, int, int, Dict]:
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise L.VgeError(f"{fn}: x must be a contiguous float32 [B,S,D] tensor, got {x.dtype} {tuple(x.shape)}")
    if len(params) != 12:
        raise L.VgeError(f"{fn}: params must be the twelve tensors {TIMELAYER_PARAMS}")
    B, S, D = x.shape
    F_ = int(params[4].shape[0]) if params[4].dim() == 2 else -1
    shapes = _timelayer_shapes(B, S, D, int(heads), F_)
    for name, t in list(zip(TIMELAYER_PARAMS, params)) + [(n, t) for n, t in named if t is not None]:
        key = name[2:] if name.startswith("d_") else name
        if t.dtype != torch.float32 or tuple(t.shape) != shapes[key] or not t.is_contiguous() or t.device != x.device:
            raise L.VgeError(f"{fn}: {name} must be a contiguous float32 {list(shapes[key])} tensor on {x.device}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
    return B, S, D, F_, shapes


def _timelayer_new(shapes, names, device):
    return tuple(torch.empty(shapes[n], dtype=torch.float32, device=device) for n in names)


def timelayer_forward(x: torch.Tensor, params: Sequence[torch.Tensor], heads: int, masks=None, save: bool = True,
                      y: Optional[torch.Tensor] = None, saved=None, workspace: Optional[torch.Tensor] = None):
    """One temporal layer (vge_timelayer_forward, include/vge.h) on the current stream -> (y, saved), saved = (qkv, u1,
    f, u2, stats) for timelayer_backward, or None with save=False (nothing but y is written).  x [B,S,D] float32;
    params: the twelve tensors of TIMELAYER_PARAMS; masks: (m_attn, m1, m_ff, m2), each a dropout multiplier or None,
    or None for no dropout; y / saved: the tensors to write, or None; workspace: a float32 tensor to use, or None."""
    lib = L.load()
    masks = tuple(masks) if masks is not None else (None,) * 4
    given = tuple(saved) if (save and saved is not None) else (None,) * 5
    B, S, D, F_, shapes = _timelayer_check("timelayer_forward", x, params, heads,
                                           list(zip(TIMELAYER_MASKS, masks)) + [("y", y)] +
                                           list(zip(TIMELAYER_SAVED, given)))
    if y is None:
        y = torch.empty_like(x)
    if save and saved is None:
        saved = _timelayer_new(shapes, TIMELAYER_SAVED, x.device)
    out = tuple(saved) if save else (None,) * 5
    wsb = int(lib.vge_timelayer_forward_workspace_bytes(B, S, D, int(heads), F_))
    if workspace is None:
        workspace = torch.empty(max(wsb, 16) // 4, dtype=torch.float32, device=x.device)
    else:
        wsb = workspace.numel() * 4
    L.check(lib.vge_timelayer_forward(_ptr(x), *[_ptr(p) for p in params], *[_ptr(m) for m in masks], B, S, D,
                                      int(heads), F_, *[_ptr(t) for t in out], _ptr(y), _ptr(workspace), wsb,
                                      _stream(x.device)), "vge_timelayer_forward")
    return y, (tuple(saved) if save else None)


def timelayer_backward(dy: torch.Tensor, x: torch.Tensor, params: Sequence[torch.Tensor], heads: int, saved,
                       masks=None, out=None, workspace: Optional[torch.Tensor] = None):
    """The layer's backward (vge_timelayer_backward) on the current stream -> (dx, then the twelve parameter gradients
    in TIMELAYER_PARAMS order).  saved: timelayer_forward's (qkv, u1, f, u2, stats) of the same x, params and masks;
    out: the thirteen result tensors, or None; workspace: a float32 tensor to use, or None."""
    lib = L.load()
    masks = tuple(masks) if masks is not None else (None,) * 4
    named = [("dy", dy)] + list(zip(TIMELAYER_MASKS, masks)) + list(zip(TIMELAYER_SAVED, saved))
    if out is not None:
        named += list(zip(("dx",) + tuple("d_" + n for n in TIMELAYER_PARAMS), out))
    B, S, D, F_, shapes = _timelayer_check("timelayer_backward", x, params, heads, named)
    if out is None:
        out = _timelayer_new(shapes, ("dx",) + TIMELAYER_PARAMS, x.device)
    wsb = int(lib.vge_timelayer_workspace_bytes(B, S, D, int(heads), F_))
    if workspace is None:
        workspace = torch.empty(max(wsb, 16) // 4, dtype=torch.float32, device=x.device)
    else:
        wsb = workspace.numel() * 4
    p = dict(zip(TIMELAYER_PARAMS, params))
    weights = [p[n] for n in ("in_proj_weight", "out_proj_weight", "linear1_weight", "linear2_weight", "norm1_weight",
                              "norm1_bias", "norm2_weight")]
    L.check(lib.vge_timelayer_backward(_ptr(dy), _ptr(x), *[_ptr(t) for t in weights], *[_ptr(m) for m in masks],
                                       *[_ptr(t) for t in saved], B, S, D, int(heads), F_, *[_ptr(t) for t in out],
                                       _ptr(workspace), wsb, _stream(x.device)), "vge_timelayer_backward")
    return tuple(out)


def _linear_check(fn: str, x: torch.Tensor, W: torch.Tensor,
                  named: Sequence[Tuple[str, Optional[torch.Tensor], Tuple[int, ...]]]) -> Tuple[int, int, int, int]:
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or (x.shape[1] > 1 and x.stride(1) != 1) or \
            (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        raise L.VgeError(f"{fn}: x must be a float32 [R,K] device tensor with unit column stride and a row stride >= K, "
                         f"got {x.dtype} {tuple(x.shape)} strides {tuple(x.stride())}")
    R, K = x.shape
    if W.dim() != 2 or int(W.shape[1]) != K:
        raise L.VgeError(f"{fn}: W must be [N,{K}], got {tuple(W.shape)}")
    N = int(W.shape[0])
    for name, t, shape in [("W", W, (N, K))] + [e for e in named if e[1] is not None]:
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != x.device:
            raise L.VgeError(f"{fn}: {name} must be a contiguous float32 {list(shape)} tensor on {x.device}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
    return R, K, N, (int(x.stride(0)) if R > 1 else max(K, int(x.stride(0))))


def linear_forward(x: torch.Tensor, W: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x W^T (vge_linear_forward, include/vge.h) on the current stream.  x float32 [R,K], read in place: a column
    slice of a wider tensor keeps its row stride; W [N,K]; y: the [R,N] tensor to write, or None."""
    lib = L.load()
    R, K, N, ldx = _linear_check("linear_forward", x, W, [("y", y, (x.shape[0], int(W.shape[0])))])
    if y is None:
        y = torch.empty((R, N), dtype=torch.float32, device=x.device)
    L.check(lib.vge_linear_forward(x.data_ptr(), ldx, _ptr(W), _ptr(y), R, K, N, _stream(x.device)), "vge_linear_forward")
    return y


def linear_backward(dy: torch.Tensor, x: torch.Tensor, W: torch.Tensor, need_dx: bool = True, out=None,
                    workspace: Optional[torch.Tensor] = None):
    """The linear map's backward (vge_linear_backward) on the current stream -> (dx [R,K] or None, dW [N,K]).  out:
    the two result tensors (dx None to skip it), or None; workspace: a float32 tensor to use, or None."""
    lib = L.load()
    N_ = int(W.shape[0]) if W.dim() == 2 else -1
    dx, dW = out if out is not None else (None, None)
    R, K, N, ldx = _linear_check("linear_backward", x, W, [("dy", dy, (x.shape[0], N_)), ("dx", dx, tuple(x.shape)),
                                                           ("dW", dW, tuple(W.shape))])
    if out is None:
        dx = torch.empty((R, K), dtype=torch.float32, device=x.device) if need_dx else None
        dW = torch.empty_like(W)
    wsb = int(lib.vge_linear_workspace_bytes(R, K, N))
    if workspace is None:
        workspace = torch.empty(max(wsb, 16) // 4, dtype=torch.float32, device=x.device)
    else:
        wsb = workspace.numel() * 4
    L.check(lib.vge_linear_backward(_ptr(dy), x.data_ptr(), ldx, _ptr(W), _ptr(dx), _ptr(dW), _ptr(workspace), wsb, R,
                                    K, N, _stream(x.device)), "vge_linear_backward")
    return dx, dW


# the eleven parameter tensors of the fusion, in the order of vge_fusion_forward
FUSION_PARAMS = ("latent", "q_ln_weight", "q_ln_bias", "kv_ln_weight", "kv_ln_bias", "Wq", "Wk", "Wv", "Wo",
                 "logit_temp", "logit_bias")
FUSION_SAVED = ("stats", "a", "p", "vp")


def _fusion_shapes(R: int, M: int, D: int) -> Dict[str, Tuple[int, ...]]:
    return {"s": (R, M, D), "ds": (R, M, D), "out": (R, D), "d_out": (R, D), "latent": (D,), "q_ln_weight": (D,),
            "q_ln_bias": (D,), "kv_ln_weight": (D,), "kv_ln_bias": (D,), "Wq": (D, D), "Wk": (D, D), "Wv": (D, D),
            "Wo": (D, D), "logit_temp": (M,), "logit_bias": (M,), "m_attn": (R, M), "stats": (4, R * M), "a": (R, M),
            "p": (R, D), "vp": (R, D)}


def _fusion_check(fn: str, s: torch.Tensor, params: Sequence[torch.Tensor],
                  named: Sequence[Tuple[str, Optional[torch.Tensor]]]) -> Tuple[int, int, int, Dict]:
    if s.dim() != 3 or s.dtype != torch.float32 or not s.is_contiguous():
        raise L.VgeError(f"{fn}: s must be a contiguous float32 [R,M,D] tensor, got {s.dtype} {tuple(s.shape)}")
    if len(params) != 11:
        raise L.VgeError(f"{fn}: params must be the eleven tensors {FUSION_PARAMS}")
    R, M, D = s.shape
    shapes = _fusion_shapes(R, M, D)
    for name, t in list(zip(FUSION_PARAMS, params)) + [(n, t) for n, t in named if t is not None]:
        key = name[2:] if name.startswith("d_") and name != "d_out" else name
        if t.dtype != torch.float32 or tuple(t.shape) != shapes[key] or not t.is_contiguous() or t.device != s.device:
            raise L.VgeError(f"{fn}: {name} must be a contiguous float32 {list(shapes[key])} tensor on {s.device}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
    return R, M, D, shapes


def fusion_forward(s: torch.Tensor, params: Sequence[torch.Tensor], m_attn: Optional[torch.Tensor] = None,
                   save: bool = True, out: Optional[torch.Tensor] = None, saved=None,
                   workspace: Optional[torch.Tensor] = None):
    """The modality fusion (vge_fusion_forward, include/vge.h) on the current stream -> (out [R,D], saved), saved =
    (stats, a, p, vp) for fusion_backward, or None with save=False (nothing but out is written).  s [R,M,D] float32: the
    per-modality sums before the affine-free LayerNorm; params: the eleven tensors of FUSION_PARAMS (latent as [D]);
    m_attn [R,M]: the dropout multiplier or None; out / saved: the tensors to write, or None."""
    lib = L.load()
    given = tuple(saved) if (save and saved is not None) else (None,) * 4
    R, M, D, shapes = _fusion_check("fusion_forward", s, params,
                                    [("m_attn", m_attn), ("out", out)] + list(zip(FUSION_SAVED, given)))
    if out is None:
        out = torch.empty(shapes["out"], dtype=torch.float32, device=s.device)
    if save and saved is None:
        saved = tuple(torch.empty(shapes[n], dtype=torch.float32, device=s.device) for n in FUSION_SAVED)
    keep = tuple(saved) if save else (None,) * 4
    wsb = int(lib.vge_fusion_forward_workspace_bytes(R, M, D))
    if workspace is None:
        workspace = torch.empty(max(wsb, 16) // 4, dtype=torch.float32, device=s.device)
    else:
        wsb = workspace.numel() * 4
    L.check(lib.vge_fusion_forward(_ptr(s), *[_ptr(p) for p in params], _ptr(m_attn), R, M, D, *[_ptr(t) for t in keep],
                                   _ptr(out), _ptr(workspace), wsb, _stream(s.device)), "vge_fusion_forward")
    return out, (tuple(saved) if save else None)


def fusion_backward(d_out: torch.Tensor, s: torch.Tensor, params: Sequence[torch.Tensor], saved,
                    m_attn: Optional[torch.Tensor] = None, out=None, workspace: Optional[torch.Tensor] = None):
    """The fusion's backward (vge_fusion_backward) on the current stream -> (ds, then the eleven parameter gradients in
    FUSION_PARAMS order).  saved: fusion_forward's (stats, a, p, vp) of the same s, params and m_attn; out: the twelve
    result tensors, or None; workspace: a float32 tensor to use, or None."""
    lib = L.load()
    named = [("d_out", d_out), ("m_attn", m_attn)] + list(zip(FUSION_SAVED, saved))
    if out is not None:
        named += list(zip(("ds",) + tuple("d_" + n for n in FUSION_PARAMS), out))
    R, M, D, shapes = _fusion_check("fusion_backward", s, params, named)
    if out is None:
        out = tuple(torch.empty(shapes[n], dtype=torch.float32, device=s.device) for n in ("ds",) + FUSION_PARAMS)
    wsb = int(lib.vge_fusion_workspace_bytes(R, M, D))
    if workspace is None:
        workspace = torch.empty(max(wsb, 16) // 4, dtype=torch.float32, device=s.device)
    else:
        wsb = workspace.numel() * 4
    L.check(lib.vge_fusion_backward(_ptr(d_out), _ptr(s), *[_ptr(p) for p in params], _ptr(m_attn),
                                    *[_ptr(t) for t in saved], R, M, D, *[_ptr(t) for t in out], _ptr(workspace), wsb,
                                    _stream(s.device)), "vge_fusion_backward")
    return tuple(out)
