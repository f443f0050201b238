"""One layer of the temporal stack (torch's nn.TransformerEncoderLayer: post-norm, ReLU, batch_first) as one autograd
node.

  timelayer_torch           the forward in torch ops on the layer's own twelve parameter tensors: the in-projection,
                            softmax(q k^T / sqrt(d)) per head, the out-projection, residual + LayerNorm, the ReLU
                            feed-forward, residual + LayerNorm; the four dropout multipliers applied by multiplication
  timelayer_backward_torch  the backward of include/vge.h written out in torch ops, in the inputs' dtype (float64 for
                            the tests' reference)
  TimeLayerFunction         once-differentiable.  On float32 device tensors of a shape the kernels take it calls
                            vge_timelayer_forward / vge_timelayer_backward (vge_timelayer.hip) and keeps qkv, u1, f, u2
                            and the LayerNorm statistics; everywhere else -- CPU tensors, other dtypes, refused shapes
                            such as a head dimension of 8 -- it runs the two torch restatements above, so a module
                            built with time_backend="hip" works anywhere.  Under torch.no_grad(), or when no input
                            requires grad, it saves nothing: the kernel is called with a NULL saved set
                            (ops.timelayer_forward(save=False)).

params is the tuple of ops.TIMELAYER_PARAMS: in_proj_weight [3D,D], in_proj_bias, out_proj weight [D,D] and bias,
linear1 weight [F,D] and bias, linear2 weight [D,F] and bias, norm1 weight and bias, norm2 weight and bias.  masks is
(m_attn [B,H,S,S], m1 [B,S,D], m_ff [B,S,F], m2 [B,S,D]), dropout multipliers (entries 0 or 1 / (1 - p)) drawn by the
caller; None, or a None entry, stands for all ones.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import ops

EPS = 1e-5
NO_MASKS = (None, None, None, None)


def layer_params(layer: torch.nn.TransformerEncoderLayer) -> Tuple[torch.Tensor, ...]:
    """The twelve parameter tensors of a torch layer in ops.TIMELAYER_PARAMS order."""
    a = layer.self_attn
    return (a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, layer.linear1.weight,
            layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, layer.norm1.weight, layer.norm1.bias,
            layer.norm2.weight, layer.norm2.bias)


def draw_masks(x: torch.Tensor, heads: int, ff: int, p_attn: float, p1: Optional[float] = None,
               p_ff: Optional[float] = None, p2: Optional[float] = None):
    """The four multipliers of a training-mode layer, each F.dropout(ones, p, True) or None where p = 0 (p1, p_ff, p2
    default to p_attn), drawn in the order torch's layer draws its own: the attention weights, dropout1, the
    feed-forward dropout, dropout2.  On the device, under one seed, they ARE torch's masks: torch's dropout1 acts on
    the attention's output, which with batch_first is the transposed view of a [S,B,D] tensor, and the dropout kernel
    draws by memory layout for such a view -- so m1 is drawn on the same view (drawn on a contiguous [B,S,D] it shares
    only the generator offset with torch's, and 0.83 of the entries at p = 0.1)."""
    B, S, D = x.shape
    p1, p_ff, p2 = (p_attn if p is None else p for p in (p1, p_ff, p2))

    def one(p, *shape, batch_second=False):
        if not p > 0:
            return None
        ones = torch.ones(shape, dtype=x.dtype, device=x.device)
        return F.dropout(ones.transpose(0, 1), p, True).contiguous() if batch_second else F.dropout(ones, p, True)
    return (one(p_attn, B, heads, S, S), one(p1, S, B, D, batch_second=True), one(p_ff, B, S, ff), one(p2, B, S, D))


def _heads(t: torch.Tensor, H: int) -> torch.Tensor:            # [B,S,D] -> [B,H,S,d]
    B, S, D = t.shape
    return t.view(B, S, H, D // H).transpose(1, 2)


def _merge(t: torch.Tensor) -> torch.Tensor:                    # [B,H,S,d] -> [B,S,D]
    B, H, S, d = t.shape
    return t.transpose(1, 2).reshape(B, S, H * d)


def _ln(u: torch.Tensor):
    mean = u.mean(dim=-1, keepdim=True)
    rstd = torch.rsqrt(u.var(dim=-1, unbiased=False, keepdim=True) + EPS)
    return (u - mean) * rstd, mean, rstd


def _attention(qkv: torch.Tensor, H: int, m_attn: Optional[torch.Tensor]):
    """-> (P, P m_attn, q, k, v), heads split: [B,H,S,S] and [B,H,S,d]."""
    q, k, v = (_heads(t, H) for t in qkv.chunk(3, dim=-1))
    P = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1]), dim=-1)
    return P, (P if m_attn is None else P * m_attn), q, k, v


def timelayer_torch(x, params: Sequence[torch.Tensor], heads: int, masks=None, return_saved: bool = False):
    """-> y [B,S,D], or (y, (qkv, u1, f, u2, stats)) with return_saved; stats [4, B S] = mean1, rstd1, mean2, rstd2."""
    Win, b_in, Wo, b_o, W1, c1, W2, c2, g1, be1, g2, be2 = params
    m_attn, m1, m_ff, m2 = masks if masks is not None else NO_MASKS
    qkv = x @ Win.t() + b_in
    _, Pm, _, _, v = _attention(qkv, heads, m_attn)
    z = _merge(Pm @ v) @ Wo.t() + b_o
    u1 = x + (z if m1 is None else z * m1)
    xh1, mean1, rstd1 = _ln(u1)
    x1 = xh1 * g1 + be1
    f = torch.relu(x1 @ W1.t() + c1)
    if m_ff is not None:
        f = f * m_ff
    g = f @ W2.t() + c2
    u2 = x1 + (g if m2 is None else g * m2)
    xh2, mean2, rstd2 = _ln(u2)
    y = xh2 * g2 + be2
    if not return_saved:
        return y
    stats = torch.stack([t.reshape(-1) for t in (mean1, rstd1, mean2, rstd2)])
    return y, (qkv, u1, f, u2, stats)


def _ln_backward(dy, u, mean, rstd, gamma):
    """-> (du, dgamma, dbeta): q = dy gamma, du = rstd (q - mean(q) - u^ mean(q u^))."""
    D = u.shape[-1]
    xh = (u - mean.view(*u.shape[:-1], 1)) * rstd.view(*u.shape[:-1], 1)
    q = dy * gamma
    du = rstd.view(*u.shape[:-1], 1) * (q - q.mean(dim=-1, keepdim=True) - xh * (q * xh).mean(dim=-1, keepdim=True))
    return du, (dy * xh).reshape(-1, D).sum(0), dy.reshape(-1, D).sum(0)


def timelayer_backward_torch(dy, x, params: Sequence[torch.Tensor], heads: int, saved, masks=None):
    """-> (dx, then the twelve parameter gradients in ops.TIMELAYER_PARAMS order) from saved = (qkv, u1, f, u2,
    stats): the formulas of include/vge.h."""
    Win, _, Wo, _, W1, _, W2, _, g1, be1, g2, _ = params
    m_attn, m1, m_ff, m2 = masks if masks is not None else NO_MASKS
    qkv, u1, f, u2, stats = saved
    D = x.shape[-1]
    rows = lambda t: t.reshape(-1, t.shape[-1])                                      # noqa: E731
    mean1, rstd1, mean2, rstd2 = (s.view(x.shape[:-1]) for s in stats)
    du2, dg2, dbe2 = _ln_backward(dy, u2, mean2, rstd2, g2)
    x1 = (u1 - mean1.unsqueeze(-1)) * rstd1.unsqueeze(-1) * g1 + be1
    dg = du2 if m2 is None else du2 * m2
    dW2, dc2 = rows(dg).t() @ rows(f), rows(dg).sum(0)
    da = (dg @ W2) * (f > 0).to(dy.dtype)
    if m_ff is not None:
        da = da * m_ff
    dW1, dc1 = rows(da).t() @ rows(x1), rows(da).sum(0)
    dx1 = du2 + da @ W1
    du1, dg1, dbe1 = _ln_backward(dx1, u1, mean1, rstd1, g1)
    dz = du1 if m1 is None else du1 * m1
    P, Pm, q, k, v = _attention(qkv, heads, m_attn)
    o = _merge(Pm @ v)
    dWo, dbo = rows(dz).t() @ rows(o), rows(dz).sum(0)
    do = _heads(dz @ Wo, heads)
    dv = Pm.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    if m_attn is not None:
        dP = dP * m_attn
    dS = P * (dP - (dP * P).sum(dim=-1, keepdim=True))
    scale = 1.0 / math.sqrt(D // heads)
    dqkv = torch.cat([_merge(dS @ k) * scale, _merge(dS.transpose(-1, -2) @ q) * scale, _merge(dv)], dim=-1)
    dWin, dbin = rows(dqkv).t() @ rows(x), rows(dqkv).sum(0)
    dx = du1 + dqkv @ Win
    return dx, dWin, dbin, dWo, dbo, dW1, dc1, dW2, dc2, dg1, dbe1, dg2, dbe2


def kernels_take(x: torch.Tensor, params: Sequence[torch.Tensor], heads: int, masks=NO_MASKS) -> bool:
    """Whether vge_timelayer_forward / _backward run this call: float32 device tensors of an accepted shape."""
    if not x.is_cuda or x.dim() != 3 or any(t is not None and (t.dtype != torch.float32 or t.device != x.device)
                                            for t in (x,) + tuple(params) + tuple(masks)):
        return False
    B, S, D = x.shape
    H, ff = int(heads), int(params[4].shape[0])
    if not (B >= 1 and 1 <= S <= 65 and 32 <= D <= 256 and D % 32 == 0 and H >= 1 and D % H == 0 and ff == 4 * D):
        return False
    d = D // H
    return d % 16 == 0 and d <= 64 and B * S * ff < 2 ** 31 and B * H * S * S < 2 ** 31


class TimeLayerFunction(torch.autograd.Function):
    """y = layer(x; the twelve parameters) with `heads` heads and the four dropout multipliers (each a tensor or None)."""

    @staticmethod
    def forward(ctx, x, heads, keep, m_attn, m1, m_ff, m2, *params):
        # keep: whether a backward can follow.  The caller decides it (timelayer below): inside forward() grad mode is
        # always off, and ctx.needs_input_grad stays True for a parameter under torch.no_grad().
        masks = (m_attn, m1, m_ff, m2)
        ctx.heads = int(heads)
        ctx.hip = kernels_take(x, params, ctx.heads, masks)
        if ctx.hip:
            x = x.contiguous()
            params = tuple(p.contiguous() for p in params)
            masks = tuple(None if m is None else m.contiguous() for m in masks)
            y, saved = ops.timelayer_forward(x, params, ctx.heads, masks, save=keep)
        elif keep:
            y, saved = timelayer_torch(x, params, ctx.heads, masks, return_saved=True)
        else:
            y, saved = timelayer_torch(x, params, ctx.heads, masks), None
        ctx.mask_given = tuple(m is not None for m in masks)
        if keep:
            ctx.save_for_backward(x, *params, *saved, *(m for m in masks if m is not None))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        t = ctx.saved_tensors
        x, params, saved = t[0], t[1:13], t[13:18]
        rest = iter(t[18:])
        masks = tuple(next(rest) if given else None for given in ctx.mask_given)
        if ctx.hip:
            grads = ops.timelayer_backward(dy.contiguous(), x, params, ctx.heads, saved, masks)
        else:
            grads = timelayer_backward_torch(dy, x, params, ctx.heads, saved, masks)
        return (grads[0], None, None, None, None, None, None, *grads[1:])


def timelayer(x: torch.Tensor, params: Sequence[torch.Tensor], heads: int, masks=None) -> torch.Tensor:
    """The layer through TimeLayerFunction; the saved set is kept only if grad mode is on and an input requires grad."""
    masks = tuple(masks) if masks is not None else NO_MASKS
    keep = torch.is_grad_enabled() and any(t.requires_grad for t in (x,) + tuple(params))
    return TimeLayerFunction.apply(x, int(heads), keep, *masks, *params)
