"""The two training losses of the reference (losses.py:6-56) with gradients from libvge.

  TCL                      losses.py:6-34, defaults temperature 0.1, k1 5000, k2 1
  SupConWithHardNegatives  losses.py:37-56, default temperature 0.07

backend="hip" (the default): forward is a torch.autograd.Function that calls vge_tcl_loss_grad /
vge_hardneg_loss_grad once -- loss and gradient in f64 inside, the gradient rounded to float32 at the store -- and
keeps the gradient; backward multiplies it by the incoming scalar on the device.  Nothing synchronises with the host.
The loss comes back as a float64 scalar (the kernels' own precision).  The HIP route of SupConWithHardNegatives is
the call the training step makes, `positive is anchor` (train.py:519-521); a general positive, CPU tensors and
backend="torch" go through the same losses written in torch ops (autograd differentiates those), which is also the
A/B partner of tools/bench_train.py.

A label that appears once in the batch makes TCL NaN on both routes (0/0, as in the reference); the HIP gradient is
then unspecified and the training step is skipped (vge.train).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops

BACKENDS = ("hip", "torch")


def tcl_torch(emb: torch.Tensor, labels: torch.Tensor, temperature: float = 0.1, k1: float = 5000.0,
              k2: float = 1.0) -> torch.Tensor:
    """mean_i (1/|P(i)|) sum_{j in P(i)} [log den_j - s_ij / temperature] with den_j as in include/vge.h: the
    reference's value (its -log(e_ij / den_j) with the quotient taken apart), in emb's dtype."""
    s = emb @ emb.T
    e = torch.exp(s / temperature)
    same = labels.view(-1, 1) == labels.view(1, -1)
    pos = same & ~torch.eye(s.shape[0], dtype=torch.bool, device=s.device)
    posf, negf = pos.to(s.dtype), (~same).to(s.dtype)
    den = (e * posf).sum(1) + k1 * (torch.exp(-s) * posf).sum(1) + k2 * (e * negf).sum(1)
    terms = (torch.log(den).view(1, -1) - s / temperature) * posf
    return (terms.sum(1) / posf.sum(1)).mean()


def hardneg_torch(anchor: torch.Tensor, positive: torch.Tensor, hard_negative: torch.Tensor,
                  temperature: float = 0.07) -> torch.Tensor:
    """Cross entropy of the logits (<a,p>, <a,h>) / temperature against class 0, mean over the batch: softplus of the
    margin <a, h - p> / temperature.  The margin is formed from the difference of the vectors, not of the two
    logits, so float32 does not cancel two numbers near 1 / temperature."""
    margin = (anchor * (hard_negative - positive)).sum(-1) / temperature
    return torch.nn.functional.softplus(margin).mean()


class _TclFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, labels, temperature, k1, k2):
        loss, grad = ops.tcl_loss_grad(emb.detach(), labels, temperature, k1, k2)
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g.to(grad.dtype), None, None, None, None


class _HardnegFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, neg, temperature):
        loss, ga, gn = ops.hardneg_loss_grad(anchor.detach(), neg.detach(), temperature)
        ctx.save_for_backward(ga, gn)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        ga, gn = ctx.saved_tensors
        g = g.to(ga.dtype)
        return ga * g, gn * g, None


def _check_backend(backend: str) -> str:
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
    return backend


class TCL(nn.Module):
    def __init__(self, temperature: float = 0.1, k1: float = 5000.0, k2: float = 1.0, backend: str = "hip"):
        super().__init__()
        self.temperature, self.k1, self.k2 = float(temperature), float(k1), float(k2)
        self.backend = _check_backend(backend)

    def forward(self, projections: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        if projections.dim() != 2 or targets.dim() != 1 or targets.shape[0] != projections.shape[0]:
            raise ValueError(f"TCL: projections must be [B,d] and targets [B], got {tuple(projections.shape)} and "
                             f"{tuple(targets.shape)}")
        if self.backend == "hip" and projections.is_cuda:
            if projections.dtype != torch.float32:
                raise ValueError(f"TCL: projections must be float32 on the hip backend, got {projections.dtype}")
            return _TclFunction.apply(projections.contiguous(), targets.to(projections.device, torch.int32),
                                      self.temperature, self.k1, self.k2)
        return tcl_torch(projections, targets.to(projections.device), self.temperature, self.k1, self.k2)


class SupConWithHardNegatives(nn.Module):
    def __init__(self, temperature: float = 0.07, backend: str = "hip"):
        super().__init__()
        self.temperature = float(temperature)
        self.backend = _check_backend(backend)

    def forward(self, anchor: torch.Tensor, positive: torch.Tensor, hard_negative: torch.Tensor) -> torch.Tensor:
        if anchor.dim() != 2 or positive.shape != anchor.shape or hard_negative.shape != anchor.shape:
            raise ValueError(f"SupConWithHardNegatives: anchor, positive and hard_negative must share one [B,d] "
                             f"shape, got {tuple(anchor.shape)}, {tuple(positive.shape)}, "
                             f"{tuple(hard_negative.shape)}")
        if self.backend == "hip" and anchor.is_cuda and positive is anchor:
            if anchor.dtype != torch.float32 or hard_negative.dtype != torch.float32:
                raise ValueError(f"SupConWithHardNegatives: anchor and hard_negative must be float32 on the hip "
                                 f"backend, got {anchor.dtype} and {hard_negative.dtype}")
            return _HardnegFunction.apply(anchor.contiguous(), hard_negative.contiguous(), self.temperature)
        return hardneg_torch(anchor, positive, hard_negative, self.temperature)
