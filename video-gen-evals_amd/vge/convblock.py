"""One residual block of a movement encoder (vge.model._Block, the reference's TemporalConvBlock) as one autograd node.

  convblock_torch           the forward in torch ops, the arithmetic of _Block: two dilated k = 5 convolutions as
                            shifted matmuls, GELU(erf), the dropout multiplier, the residual, GroupNorm(1)
  convblock_backward_torch  the backward of include/vge.h written out in torch ops, in the inputs' dtype (float64 for
                            the tests' reference)
  ConvBlockFunction         once-differentiable.  On float32 device tensors of a shape the kernels take it calls
                            vge_convblock_forward / vge_convblock_backward (vge_convblock.hip) and keeps a, u, mean and
                            rstd; everywhere else -- CPU tensors, other dtypes, other shapes -- it runs the two torch
                            restatements above, so a module built with conv_backend="hip" works anywhere.  Under
                            torch.no_grad(), or when no input requires grad, it saves nothing: the kernel is
                            called with a NULL saved set (ops.convblock_forward(save=False)).

The dropout multiplier `mask` [B,T,C] (entries 0 or 1 / (1 - p)) is drawn by the caller; None stands for all ones.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from . import ops

KERNEL_SIZE = 5
EPS = 1e-5
DILATIONS = (1, 2, 4, 8)


def _conv(v: torch.Tensor, w: torch.Tensor, dilation: int) -> torch.Tensor:
    """conv(v; w)[b,t,o] = sum_j sum_i v[b, t + (j - 2) dilation, i] w[o,i,j]: _ConvWeight.forward's arithmetic."""
    T, pad = v.shape[1], dilation * (KERNEL_SIZE - 1) // 2
    vp = F.pad(v, (0, 0, pad, pad))
    taps = torch.cat([vp[:, j * dilation:j * dilation + T, :] for j in range(KERNEL_SIZE)], dim=-1)
    return taps @ w.permute(2, 1, 0).reshape(KERNEL_SIZE * w.shape[1], w.shape[0])


def _conv_data_grad(d: torch.Tensor, w: torch.Tensor, dilation: int) -> torch.Tensor:
    """sum_j sum_o d[b, s - (j - 2) dilation, o] w[o,i,j]: the same convolution, taps flipped, each tap transposed."""
    return _conv(d, w.flip(2).transpose(0, 1), dilation)


def _conv_weight_grad(d: torch.Tensor, v: torch.Tensor, dilation: int) -> torch.Tensor:
    """dw[o,i,j] = sum_{b,t} d[b,t,o] v[b, t + (j - 2) dilation, i]."""
    T, pad = v.shape[1], dilation * (KERNEL_SIZE - 1) // 2
    vp = F.pad(v, (0, 0, pad, pad))
    return torch.stack([torch.einsum("bto,bti->oi", d, vp[:, j * dilation:j * dilation + T, :])
                        for j in range(KERNEL_SIZE)], dim=-1)


def _gelu_grad(z: torch.Tensor) -> torch.Tensor:
    """Phi(z) + z phi(z)."""
    return 0.5 * (1.0 + torch.erf(z * math.sqrt(0.5))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def convblock_torch(x, w1, w2, gamma, beta, dilation: int, mask: Optional[torch.Tensor] = None,
                    return_saved: bool = False):
    """-> y [B,T,C], or (y, (a, u, mean, rstd)) with return_saved."""
    a = _conv(x, w1, dilation)
    h = F.gelu(a)
    if mask is not None:
        h = h * mask
    u = _conv(h, w2, dilation) + x
    g = F.gelu(u)
    y = F.layer_norm(g, g.shape[1:], eps=EPS) * gamma + beta
    if not return_saved:
        return y
    mean = g.mean(dim=(1, 2))
    rstd = torch.rsqrt(g.var(dim=(1, 2), unbiased=False) + EPS)
    return y, (a, u, mean, rstd)


def convblock_backward_torch(dy, x, w1, w2, gamma, dilation: int, saved, mask: Optional[torch.Tensor] = None):
    """-> (dx, dw1, dw2, dgamma, dbeta) from saved = (a, u, mean, rstd): the formulas of include/vge.h."""
    a, u, mean, rstd = saved
    mean, rstd = mean.view(-1, 1, 1), rstd.view(-1, 1, 1)
    ghat = (F.gelu(u) - mean) * rstd
    dbeta = dy.sum(dim=(0, 1))
    dgamma = (dy * ghat).sum(dim=(0, 1))
    q = dy * gamma
    dg = rstd * (q - q.mean(dim=(1, 2), keepdim=True) - ghat * (q * ghat).mean(dim=(1, 2), keepdim=True))
    du = dg * _gelu_grad(u)
    h = F.gelu(a)
    if mask is not None:
        h = h * mask
    dw2 = _conv_weight_grad(du, h, dilation)
    da = _conv_data_grad(du, w2, dilation) * _gelu_grad(a)
    if mask is not None:
        da = da * mask
    dw1 = _conv_weight_grad(da, x, dilation)
    dx = du + _conv_data_grad(da, w1, dilation)
    return dx, dw1, dw2, dgamma, dbeta


def kernels_take(x: torch.Tensor, *others: Optional[torch.Tensor], dilation: int) -> bool:
    """Whether vge_convblock_forward / _backward run this call: float32 device tensors of an accepted shape."""
    if not x.is_cuda or x.dim() != 3 or any(t is not None and (t.dtype != torch.float32 or t.device != x.device)
                                            for t in (x,) + others):
        return False
    B, T, C = x.shape
    return B >= 1 and 1 <= T <= 64 and 32 <= C <= 256 and C % 32 == 0 and B * T * C < 2 ** 31 and dilation in DILATIONS


class ConvBlockFunction(torch.autograd.Function):
    """y = block(x; w1, w2, gamma, beta) with dilation and the dropout multiplier `mask` (or None)."""

    @staticmethod
    def forward(ctx, x, w1, w2, gamma, beta, dilation, mask, keep):
        # keep: whether a backward can follow.  The caller decides it (convblock below): inside forward() grad mode is
        # always off, and ctx.needs_input_grad stays True for a parameter under torch.no_grad().
        ctx.dilation = int(dilation)
        ctx.hip = kernels_take(x, w1, w2, gamma, beta, mask, dilation=ctx.dilation)
        if ctx.hip:
            x, w1, w2 = x.contiguous(), w1.contiguous(), w2.contiguous()
            gamma, beta = gamma.contiguous(), beta.contiguous()
            mask = None if mask is None else mask.contiguous()
            y, saved = ops.convblock_forward(x, w1, w2, gamma, beta, ctx.dilation, mask, save=keep)
        elif keep:
            y, saved = convblock_torch(x, w1, w2, gamma, beta, ctx.dilation, mask, return_saved=True)
        else:
            y, saved = convblock_torch(x, w1, w2, gamma, beta, ctx.dilation, mask), None
        ctx.has_mask = mask is not None
        if keep:
            ctx.save_for_backward(x, w1, w2, gamma, *saved, *((mask,) if mask is not None else ()))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w1, w2, gamma, a, u, mean, rstd = ctx.saved_tensors[:8]
        mask = ctx.saved_tensors[8] if ctx.has_mask else None
        if ctx.hip:
            grads = ops.convblock_backward(dy.contiguous(), x, w1, w2, gamma, ctx.dilation, (a, u, mean, rstd), mask)
        else:
            grads = convblock_backward_torch(dy, x, w1, w2, gamma, ctx.dilation, (a, u, mean, rstd), mask)
        return (*grads, None, None, None)


def convblock(x, w1, w2, gamma, beta, dilation: int, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The block through ConvBlockFunction; the saved set is kept only if grad mode is on and an input requires grad."""
    keep = torch.is_grad_enabled() and any(t.requires_grad for t in (x, w1, w2, gamma, beta))
    return ConvBlockFunction.apply(x, w1, w2, gamma, beta, dilation, mask, keep)
