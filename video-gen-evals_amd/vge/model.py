"""The scorer as a torch module, for autograd through the encoder during training (vge.train).

HumanActionScorer has the reference's constructor signature (model.py:102-110) and exactly its state_dict keys and
shapes, so a state dict moves both ways between it, the reference, and the hand-written forward (ops.Encoder /
vge.eval.load_model).  The architecture is the one oracle/encoder.py and DESIGN.md state:

  per modality   state encoder on the raw features (+ motion encoder on the differences where the modality has any):
                 stem (1x1 conv = matmul), 4 residual blocks of two k = 5 convolutions with dilation 1, 2, 4, 8
                 (GELU(erf), dropout after the first, GroupNorm(1)), a projection; then a LayerNorm without affine
  fusion         one learned query over the M modality tokens of a frame: LayerNorms, Wq / Wk / Wv, logits /
                 sqrt(d) / (softplus(logit_temp) + 1e-3) + logit_bias, softmax, dropout, Wo
  temporal       CLS + frames, sinusoidal positions, torch's own nn.TransformerEncoder (post-norm, ReLU), so its
                 keys match;  outputs L2-normalised

Everything is channels-last [B,T,C] and the convolutions are matmuls: a dilated k = 5 convolution is the five
shifted slices of the zero-padded sequence concatenated on the channel axis times the [5 C, C] reshaped weight.  No
convolution library is involved (no solver search at the first step), and every op runs on the current stream.  The
temporal stack's attention takes scaled_dot_product_attention's "math" route (two matmuls and a softmax), not torch's
fused attention kernels: those are the least exact float32 step of the backward.

This module's forward and backward run on torch's kernels (rocBLAS / hipBLASLt and native ones); the hand-written
encoder kernels keep no activations and have no backward.  The HIP of a training step is the loss (vge.losses) and,
with conv_backend="hip", the residual blocks of the movement encoders: each block is then one autograd node
(vge.convblock.ConvBlockFunction) on the forward and backward kernels of vge_convblock.hip, with the same parameters
under the same state-dict keys.  With time_backend="hip" each layer of the temporal stack is one autograd node as well
(vge.timelayer.TimeLayerFunction) on the kernels of vge_timelayer.hip, again on the nn.TransformerEncoder's own
parameters.  With linear_backend="hip" the stem and the projection of every movement encoder go through
vge.linear.LinearFunction on the kernels of vge_linear.hip -- the stem reads its columns of x in place, as a view with
a row stride --, and with fusion_backend="hip" the per-modality LayerNorm and the fusion are one node
(vge.fusion.FusionFunction, vge_fusion.hip) in the folded form: Wk meets the query, not the tokens, and Wv and Wo run
over the pooled rows.  The four switches are independent; their defaults, "torch", are the graph described above,
unchanged.  With all four on "hip" every GEMM and every sum across samples of a step's forward and backward runs in
the project's kernels; what stays on torch is elementwise or per row (the additions, positions, dropout masks,
F.normalize) and the concatenation of CLS.
"""
from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

from .convblock import convblock
from .fusion import fusion, fusion_params
from .linear import linear
from .timelayer import draw_masks, layer_params, timelayer

KERNEL_SIZE = 5
DILATIONS = (1, 2, 4, 8)
CONV_BACKENDS = ("torch", "hip")
TIME_BACKENDS = ("torch", "hip")
LINEAR_BACKENDS = ("torch", "hip")
FUSION_BACKENDS = ("torch", "hip")


def _check_conv_backend(conv_backend: str) -> str:
    if conv_backend not in CONV_BACKENDS:
        raise ValueError(f"conv_backend must be one of {CONV_BACKENDS}, got {conv_backend!r}")
    return conv_backend


def _check_time_backend(time_backend: str) -> str:
    if time_backend not in TIME_BACKENDS:
        raise ValueError(f"time_backend must be one of {TIME_BACKENDS}, got {time_backend!r}")
    return time_backend


def _check_linear_backend(linear_backend: str) -> str:
    if linear_backend not in LINEAR_BACKENDS:
        raise ValueError(f"linear_backend must be one of {LINEAR_BACKENDS}, got {linear_backend!r}")
    return linear_backend


def _check_fusion_backend(fusion_backend: str) -> str:
    if fusion_backend not in FUSION_BACKENDS:
        raise ValueError(f"fusion_backend must be one of {FUSION_BACKENDS}, got {fusion_backend!r}")
    return fusion_backend


def _uniform_fan_in(shape, fan_in: int) -> nn.Parameter:
    """torch's default init of Linear / Conv weights: U(-1/sqrt(fan_in), 1/sqrt(fan_in))."""
    b = 1.0 / math.sqrt(fan_in)
    return nn.Parameter(torch.empty(shape).uniform_(-b, b))


class _ConvWeight(nn.Module):
    """`weight` [C_out, C_in, k] of a bias-free Conv1d, applied to channels-last input as shifted matmuls."""

    def __init__(self, c_in: int, c_out: int, k: int, dilation: int = 1):
        super().__init__()
        self.k, self.dilation = k, dilation
        self.weight = _uniform_fan_in((c_out, c_in, k), c_in * k)

    def forward(self, x: torch.Tensor) -> torch.Tensor:            # [B,T,C_in] -> [B,T,C_out]
        if self.k == 1:
            return x @ self.weight[:, :, 0].t()
        T, dil = x.shape[1], self.dilation
        pad = dil * (self.k - 1) // 2
        xp = F.pad(x, (0, 0, pad, pad))
        taps = torch.cat([xp[:, j * dil:j * dil + T, :] for j in range(self.k)], dim=-1)      # [B,T,k C_in]
        w = self.weight.permute(2, 1, 0).reshape(self.k * self.weight.shape[1], self.weight.shape[0])
        return taps @ w


class _ChannelAffine(nn.Module):
    """GroupNorm(1, C) on channels-last input: one mean / variance per sample over (T, C), per-channel affine."""

    def __init__(self, channels: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(channels))
        self.bias = nn.Parameter(torch.zeros(channels))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return F.layer_norm(x, x.shape[1:], eps=self.eps) * self.weight + self.bias


class _Block(nn.Module):
    def __init__(self, channels: int, dilation: int, p: float, conv_backend: str = "torch"):
        super().__init__()
        self.conv_backend = _check_conv_backend(conv_backend)
        self.conv1 = _ConvWeight(channels, channels, KERNEL_SIZE, dilation)
        self.conv2 = _ConvWeight(channels, channels, KERNEL_SIZE, dilation)
        self.norm = _ChannelAffine(channels)
        self.drop = nn.Dropout(p)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.conv_backend == "hip":
            # the multiplier self.drop would apply, drawn where the torch backend draws it (after conv1)
            mask = F.dropout(torch.ones_like(x), self.drop.p, True) if self.training and self.drop.p > 0 else None
            return convblock(x, self.conv1.weight, self.conv2.weight, self.norm.weight, self.norm.bias,
                             self.conv1.dilation, mask)
        y = self.conv2(self.drop(F.gelu(self.conv1(x))))
        return self.norm(F.gelu(y + x))


class _Linear(nn.Module):
    """`weight` [out, in] of a bias-free Linear."""

    def __init__(self, d_in: int, d_out: int):
        super().__init__()
        self.weight = _uniform_fan_in((d_out, d_in), d_in)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x @ self.weight.t()


class _MovementEncoder(nn.Module):
    def __init__(self, d_in: int, d_out: int, p: float, conv_backend: str = "torch", linear_backend: str = "torch"):
        super().__init__()
        self.linear_backend = _check_linear_backend(linear_backend)
        self.stem = _ConvWeight(d_in, d_out, 1)
        self.blocks = nn.ModuleList([_Block(d_out, dil, p, conv_backend) for dil in DILATIONS])
        self.proj = _Linear(d_out, d_out)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        hip = self.linear_backend == "hip"
        # x is a column slice of the feature tensor: linear() reads it in place
        y = linear(x, self.stem.weight.view(self.stem.weight.shape[:2])) if hip else self.stem(x)
        for blk in self.blocks:
            y = blk(y)
        return linear(y, self.proj.weight) if hip else self.proj(y)


class _Fusion(nn.Module):
    def __init__(self, d_model: int, n_modalities: int, p: float):
        super().__init__()
        self.latent = nn.Parameter(torch.randn(1, 1, d_model))
        self.q_ln = nn.LayerNorm(d_model)
        self.kv_ln = nn.LayerNorm(d_model)
        self.Wq, self.Wk = _Linear(d_model, d_model), _Linear(d_model, d_model)
        self.Wv, self.Wo = _Linear(d_model, d_model), _Linear(d_model, d_model)
        self.logit_temp = nn.Parameter(torch.zeros(n_modalities))
        self.logit_bias = nn.Parameter(torch.zeros(n_modalities))
        self.dropout = nn.Dropout(p)

    def forward(self, tokens: torch.Tensor) -> torch.Tensor:        # [B,T,M,D] -> [B,T,D]
        D = tokens.shape[-1]
        kv = self.kv_ln(tokens)
        q = self.Wq(self.q_ln(self.latent)).view(D)                 # the one query, the same for every frame
        logits = (self.Wk(kv) @ q) / math.sqrt(D)                   # [B,T,M]
        logits = logits / (F.softplus(self.logit_temp) + 1e-3) + self.logit_bias
        attn = self.dropout(logits.softmax(dim=-1))
        return self.Wo((attn.unsqueeze(-1) * self.Wv(kv)).sum(dim=2))


class _Positions(nn.Module):
    def __init__(self, d_model: int, max_len: int = 5000):
        super().__init__()
        pos = torch.arange(max_len, dtype=torch.float32).unsqueeze(1)
        div = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) * (-math.log(10000.0) / d_model))
        pe = torch.zeros(max_len, d_model)
        pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * div), torch.cos(pos * div)
        self.register_buffer("pe", pe.unsqueeze(0))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x + self.pe[:, :x.shape[1]]


class HumanActionScorer(nn.Module):
    def __init__(self, dims_map_raw: Dict[str, int], dims_map_diff: Dict[str, int], d_model: int = 256,
                 latent_dim: int = 128, time_layers: int = 4, time_heads: int = 8, dropout: float = 0.1,
                 conv_backend: str = "torch", time_backend: str = "torch", linear_backend: str = "torch",
                 fusion_backend: str = "torch"):
        super().__init__()
        self.conv_backend = _check_conv_backend(conv_backend)
        self.time_backend = _check_time_backend(time_backend)
        self.linear_backend = _check_linear_backend(linear_backend)
        self.fusion_backend = _check_fusion_backend(fusion_backend)
        if not isinstance(dims_map_raw, dict) or not isinstance(dims_map_diff, dict):
            raise ValueError("dims_map_raw and dims_map_diff must be dicts of {modality: dim}")
        if set(dims_map_raw) != set(dims_map_diff):
            raise ValueError("dims_map_raw and dims_map_diff must have the same modalities")
        self.modalities = list(dims_map_raw)
        self.dims_raw = {m: int(dims_map_raw[m]) for m in self.modalities}
        self.dims_diff = {m: int(dims_map_diff[m]) for m in self.modalities}
        self.hyper_parameters = {"d_model": int(d_model), "latent_dim": int(latent_dim),
                                 "time_layers": int(time_layers), "time_heads": int(time_heads),
                                 "dropout": float(dropout)}
        self.state_enc = nn.ModuleDict({m: _MovementEncoder(self.dims_raw[m], d_model, dropout, conv_backend,
                                                            linear_backend)
                                        for m in self.modalities})
        with_diff = [m for m in self.modalities if self.dims_diff[m] > 0]
        self.motion_enc = nn.ModuleDict({m: _MovementEncoder(self.dims_diff[m], d_model, dropout, conv_backend,
                                                             linear_backend)
                                         for m in with_diff}) if with_diff else None
        self.fusion = _Fusion(d_model, len(self.modalities), dropout)
        self.cls = nn.Parameter(torch.randn(1, 1, d_model))
        self.pos_enc = _Positions(d_model)
        layer = nn.TransformerEncoderLayer(d_model, time_heads, 4 * d_model, dropout, batch_first=True)
        self.temporal = nn.TransformerEncoder(layer, num_layers=time_layers, enable_nested_tensor=False)

    def _temporal_hip(self, tokens: torch.Tensor) -> torch.Tensor:
        """self.temporal layer by layer through vge.timelayer, on each layer's own parameters.  In training mode the
        four dropout multipliers are drawn as torch's layer draws its masks (vge.timelayer.draw_masks)."""
        for layer in self.temporal.layers:
            H = layer.self_attn.num_heads
            masks = None
            if self.training:
                masks = draw_masks(tokens, H, layer.linear1.out_features, layer.self_attn.dropout, layer.dropout1.p,
                                   layer.dropout.p, layer.dropout2.p)
            tokens = timelayer(tokens, layer_params(layer), H, masks)
        return tokens

    def forward(self, x: torch.Tensor):
        """x [B,T,sum(raw) + sum(diff)] -> (seq_embed [B,d], frame_embeds [B,T+1,d], tokens [B,T+1,d])."""
        n_raw = sum(self.dims_raw.values())
        n_diff = sum(self.dims_diff.values())
        if x.dim() != 3 or x.shape[-1] != n_raw + n_diff:
            raise ValueError(f"HumanActionScorer: x must be [B,T,{n_raw + n_diff}], got {tuple(x.shape)}")
        raw = dict(zip(self.modalities, torch.split(x[..., :n_raw], list(self.dims_raw.values()), dim=-1)))
        diff = dict(zip(self.modalities, torch.split(x[..., n_raw:], list(self.dims_diff.values()), dim=-1)))
        per_mod = []
        for m in self.modalities:
            s = self.state_enc[m](raw[m])
            if self.dims_diff[m] > 0:
                s = s + self.motion_enc[m](diff[m])
            per_mod.append(s if self.fusion_backend == "hip" else F.layer_norm(s, s.shape[-1:]))
        if self.fusion_backend == "hip":
            # the node owns the affine-free LayerNorm; the multiplier self.fusion.dropout would apply to the attention
            # weights is drawn where the torch backend draws it
            p = self.fusion.dropout.p
            m_attn = F.dropout(torch.ones(x.shape[0], x.shape[1], len(per_mod), dtype=x.dtype, device=x.device), p,
                               True) if self.training and p > 0 else None
            frames = fusion(torch.stack(per_mod, dim=2), fusion_params(self.fusion), m_attn)
        else:
            frames = self.fusion(torch.stack(per_mod, dim=2))
        tokens = torch.cat([self.cls.expand(x.shape[0], -1, -1), frames], dim=1)
        if self.time_backend == "hip":
            tokens = self._temporal_hip(self.pos_enc(tokens))
            return F.normalize(tokens[:, 0, :]), F.normalize(tokens, dim=-1), tokens
        # attention as matmul + softmax + matmul (the "math" route of scaled_dot_product_attention): torch's fused
        # attention kernels are less exact in float32 -- with them two step-0 gradient norms of the golden checkpoint
        # sit 8.7 r from float64 on an MI355X, with this route the worst is 2.2 r
        with sdpa_kernel(SDPBackend.MATH):
            tokens = self.temporal(self.pos_enc(tokens))
        return F.normalize(tokens[:, 0, :]), F.normalize(tokens, dim=-1), tokens

    def numpy_state_dict(self) -> Dict[str, "object"]:
        """The state dict as float32 numpy arrays on the host: what ops.Encoder and load_model take."""
        return {k: v.detach().float().cpu().numpy() for k, v in self.state_dict().items()}
