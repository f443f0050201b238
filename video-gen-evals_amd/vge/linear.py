"""A bias-free linear map -- the movement encoders' stems (1 x 1 convolutions) and projections -- as one autograd node.

  linear_torch           y = x W^T in torch ops
  linear_backward_torch  the backward of include/vge.h in torch ops, in the inputs' dtype (float64 for the tests'
                         reference): dx = dy W, dW = dy^T x
  LinearFunction         once-differentiable.  On float32 device tensors of a shape the kernels take it calls
                         vge_linear_forward / vge_linear_backward (vge_linear.hip); everywhere else -- CPU tensors, other
                         dtypes, refused shapes such as N = 48 -- it runs the two torch restatements above, so a module
                         built with linear_backend="hip" works anywhere.  Under torch.no_grad(), or when no input
                         requires grad, it saves nothing.  dx is computed only where x requires grad: a stem's input
                         is data.

x is [..., K] with unit stride along K; a column slice of a wider contiguous tensor (a stem's input is columns of the
feature tensor [B,T,2596]) is handed to the kernel as it is, base pointer plus row stride, not copied.  W is [N,K].
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops


def linear_torch(x: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    return x @ W.t()


def linear_backward_torch(dy: torch.Tensor, x: torch.Tensor, W: torch.Tensor, need_dx: bool = True):
    """-> (dx or None, dW): the formulas of include/vge.h."""
    dW = dy.reshape(-1, dy.shape[-1]).t() @ x.reshape(-1, x.shape[-1])
    return (dy @ W if need_dx else None), dW


def _rows(x: torch.Tensor) -> Optional[torch.Tensor]:
    """x [..., K] as a [R,K] view with one row stride, or None where the leading dimensions do not collapse."""
    K = x.shape[-1]
    if x.dim() < 2 or (K > 1 and x.stride(-1) != 1):
        return None
    R = x.numel() // max(K, 1)
    lead = [(n, st) for n, st in zip(x.shape[:-1], x.stride()[:-1]) if n > 1]
    if not lead:
        return x.as_strided((R, K), (K, 1))
    ldx = lead[-1][1]
    span = ldx
    for n, st in reversed(lead):
        if st != span:
            return None
        span = st * n
    return x.as_strided((R, K), (ldx, 1)) if ldx >= K else None


def kernels_take(x: torch.Tensor, W: torch.Tensor) -> bool:
    """Whether vge_linear_forward / _backward run this call: float32 device tensors of an accepted shape."""
    if not x.is_cuda or x.dim() < 2 or W.dim() != 2 or any(t.dtype != torch.float32 or t.device != x.device
                                                             for t in (x, W)):
        return False
    N, K = W.shape
    if x.shape[-1] != K or not (1 <= K <= 4096 and 32 <= N <= 256 and N % 32 == 0) or x.numel() < 1:
        return False
    rows = _rows(x)
    return rows is not None and rows.shape[0] * max(N, int(rows.stride(0))) < 2 ** 31


class LinearFunction(torch.autograd.Function):
    """y = x W^T."""

    @staticmethod
    def forward(ctx, x, W, keep):
        # keep: whether a backward can follow; the caller decides it (linear below), as vge.timelayer does
        ctx.hip = kernels_take(x, W)
        if ctx.hip:
            W = W.contiguous()
            y = ops.linear_forward(_rows(x), W).view(*x.shape[:-1], W.shape[0])
        else:
            y = linear_torch(x, W)
        if keep:
            ctx.save_for_backward(x, W)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[0]
        if ctx.hip:
            dx, dW = ops.linear_backward(dy.contiguous().view(-1, W.shape[0]), _rows(x), W, need_dx)
            dx = dx.view(x.shape) if need_dx else None
        else:
            dx, dW = linear_backward_torch(dy, x, W, need_dx)
        return dx, dW, None


def linear(x: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """The map through LinearFunction; x and W are kept only if grad mode is on and one of them requires grad."""
    keep = torch.is_grad_enabled() and (x.requires_grad or W.requires_grad)
    return LinearFunction.apply(x, W, keep)
