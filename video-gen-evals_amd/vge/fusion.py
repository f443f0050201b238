"""The modality fusion (vge.model._Fusion with the affine-free LayerNorm in front of it) as one autograd node.

  fusion_torch           the forward of include/vge.h in torch ops, in the folded form: the logit of modality m is
                         <kv_m, u> with u = Wk^T Wq (LN(latent) g_q + b_q), one vector for every row, and Wv and Wo
                         act on the pooled row p = sum_m ad_m kv_m, not on the M tokens
  fusion_backward_torch  the backward of include/vge.h written out in torch ops, in the inputs' dtype (float64 for the
                         tests' reference)
  FusionFunction         once-differentiable.  On float32 device tensors of a shape the kernels take it calls
                         vge_fusion_forward / vge_fusion_backward (vge_fusion.hip) and keeps the LayerNorm statistics,
                         the attention weights a, p and Wv p; everywhere else -- CPU tensors, other dtypes, refused
                         shapes such as M = 9 -- it runs the two torch restatements above, so a module built with
                         fusion_backend="hip" works anywhere.  Under torch.no_grad(), or when no input requires grad,
                         it saves nothing: the kernel is called with a NULL saved set.

s is [..., M, D]: the stacked per-modality sums before the affine-free LayerNorm; the result is [..., D].  params is
the tuple of ops.FUSION_PARAMS: latent (any shape of D elements), q_ln weight and bias, kv_ln weight and bias, Wq, Wk,
Wv, Wo [D,D], logit_temp and logit_bias [M].  m_attn [..., M] is the dropout multiplier of the attention weights
(entries 0 or 1 / (1 - p)) drawn by the caller; None stands for all ones.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import ops

EPS = 1e-5


def fusion_params(module) -> Tuple[torch.Tensor, ...]:
    """The eleven parameter tensors of a _Fusion module in ops.FUSION_PARAMS order."""
    return (module.latent, module.q_ln.weight, module.q_ln.bias, module.kv_ln.weight, module.kv_ln.bias,
            module.Wq.weight, module.Wk.weight, module.Wv.weight, module.Wo.weight, module.logit_temp,
            module.logit_bias)


def _ln(v: torch.Tensor):
    mean = v.mean(dim=-1, keepdim=True)
    rstd = torch.rsqrt(v.var(dim=-1, unbiased=False, keepdim=True) + EPS)
    return (v - mean) * rstd, mean, rstd


def _ln_backward(q: torch.Tensor, vh: torch.Tensor, rstd: torch.Tensor) -> torch.Tensor:
    """dv = rstd (q - mean(q) - v^ mean(q v^))."""
    return rstd * (q - q.mean(dim=-1, keepdim=True) - vh * (q * vh).mean(dim=-1, keepdim=True))


def _query(params: Sequence[torch.Tensor]):
    """-> (LN^(latent), rstd, ql, qv, u): the row-independent part."""
    latent, g_q, b_q, _, _, Wq, Wk = params[:7]
    hl, _, rstd = _ln(latent.reshape(-1))
    ql = hl * g_q + b_q
    qv = Wq @ ql
    return hl, rstd, ql, qv, Wk.t() @ qv


def _scale(temp: torch.Tensor, D: int) -> torch.Tensor:
    return 1.0 / math.sqrt(D) / (F.softplus(temp) + 1e-3)


def fusion_torch(s, params: Sequence[torch.Tensor], m_attn: Optional[torch.Tensor] = None, return_saved: bool = False):
    """-> out [..., D], or (out, (stats, a, p, vp)) with return_saved; stats [4, R M] = mean0, rstd0, mean1, rstd1."""
    g_kv, b_kv = params[3], params[4]
    Wv, Wo, temp, bias = params[7:]
    D = s.shape[-1]
    t, mean0, rstd0 = _ln(s)
    h, mean1, rstd1 = _ln(t)
    kv = h * g_kv + b_kv
    u = _query(params)[4]
    a = torch.softmax((kv @ u) * _scale(temp, D) + bias, dim=-1)
    ad = a if m_attn is None else a * m_attn
    p = (ad.unsqueeze(-1) * kv).sum(dim=-2)
    vp = p @ Wv.t()
    out = vp @ Wo.t()
    if not return_saved:
        return out
    stats = torch.stack([x.reshape(-1) for x in (mean0, rstd0, mean1, rstd1)])
    return out, (stats, a.reshape(-1, a.shape[-1]), p.reshape(-1, D), vp.reshape(-1, D))


def fusion_backward_torch(d_out, s, params: Sequence[torch.Tensor], saved, m_attn: Optional[torch.Tensor] = None):
    """-> (ds, then the eleven parameter gradients in ops.FUSION_PARAMS order) from saved = (stats, a, p, vp): the
    formulas of include/vge.h."""
    latent, g_q, b_q, g_kv, b_kv, Wq, Wk, Wv, Wo, temp, bias = params
    stats, a, p, vp = saved
    M, D = s.shape[-2:]
    rows = lambda x: x.reshape(-1, x.shape[-1])                                      # noqa: E731
    mean0, rstd0, mean1, rstd1 = (x.view(*s.shape[:-1], 1) for x in stats)
    a = a.view(s.shape[:-1])
    t = (s - mean0) * rstd0
    h = (t - mean1) * rstd1
    kv = h * g_kv + b_kv
    hl, rstd_l, ql, qv, u = _query(params)
    c = _scale(temp, D)
    dWo = rows(d_out).t() @ vp
    dvp = d_out @ Wo
    dWv = rows(dvp).t() @ p
    dp = dvp @ Wv
    da = (kv * dp.unsqueeze(-2)).sum(dim=-1)
    ad = a
    if m_attn is not None:
        da, ad = da * m_attn, a * m_attn
    dl = a * (da - (a * da).sum(dim=-1, keepdim=True))
    dbias = rows(dl).sum(0)
    dc = rows(dl * (kv @ u)).sum(0)
    dtemp = -dc * c * torch.sigmoid(temp) / (F.softplus(temp) + 1e-3)
    w2 = (dl * c).unsqueeze(-1)
    dkv = ad.unsqueeze(-1) * dp.unsqueeze(-2) + w2 * u
    du = rows(w2 * kv).sum(0)
    dg_kv, db_kv = rows(dkv * h).sum(0), rows(dkv).sum(0)
    ds = _ln_backward(_ln_backward(dkv * g_kv, h, rstd1), t, rstd0)
    dWk = torch.outer(qv, du)
    dqv = Wk @ du
    dWq = torch.outer(dqv, ql)
    dql = Wq.t() @ dqv
    dlatent = _ln_backward(dql * g_q, hl, rstd_l).reshape(latent.shape)
    return ds, dlatent, dql * hl, dql, dg_kv, db_kv, dWq, dWk, dWv, dWo, dtemp, dbias


def kernels_take(s: torch.Tensor, params: Sequence[torch.Tensor], m_attn: Optional[torch.Tensor] = None) -> bool:
    """Whether vge_fusion_forward / _backward run this call: float32 device tensors of an accepted shape."""
    if not s.is_cuda or s.dim() < 2 or any(t is not None and (t.dtype != torch.float32 or t.device != s.device)
                                           for t in (s, m_attn) + tuple(params)):
        return False
    M, D = s.shape[-2:]
    return 1 <= M <= 8 and 32 <= D <= 256 and D % 32 == 0 and 1 <= s.numel() < 2 ** 31


class FusionFunction(torch.autograd.Function):
    """out = fusion(s; the eleven parameters) with the dropout multiplier m_attn (a tensor or None)."""

    @staticmethod
    def forward(ctx, s, keep, m_attn, *params):
        # keep: whether a backward can follow; the caller decides it (fusion below), as vge.timelayer does
        ctx.hip = kernels_take(s, params, m_attn)
        ctx.latent_shape = params[0].shape
        if ctx.hip:
            M, D = s.shape[-2:]
            s = s.contiguous()
            params = (params[0].reshape(D),) + tuple(p.contiguous() for p in params[1:])
            m_attn = None if m_attn is None else m_attn.contiguous()
            out, saved = ops.fusion_forward(s.view(-1, M, D), params, None if m_attn is None else m_attn.view(-1, M),
                                            save=keep)
            out = out.view(*s.shape[:-2], D)
        elif keep:
            out, saved = fusion_torch(s, params, m_attn, return_saved=True)
        else:
            out, saved = fusion_torch(s, params, m_attn), None
        ctx.masked = m_attn is not None
        if keep:
            ctx.save_for_backward(s, *params, *saved, *((m_attn,) if ctx.masked else ()))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        t = ctx.saved_tensors
        s, params, saved = t[0], t[1:12], t[12:16]
        m_attn = t[16] if ctx.masked else None
        if ctx.hip:
            M, D = s.shape[-2:]
            grads = ops.fusion_backward(d_out.contiguous().view(-1, D), s.view(-1, M, D), params, saved,
                                        None if m_attn is None else m_attn.view(-1, M))
            grads = (grads[0].view(s.shape), grads[1].view(ctx.latent_shape)) + grads[2:]
        else:
            grads = fusion_backward_torch(d_out, s, params, saved, m_attn)
        return (grads[0], None, None, *grads[1:])


def fusion(s: torch.Tensor, params: Sequence[torch.Tensor], m_attn: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The fusion through FusionFunction; the saved set is kept only if grad mode is on and an input requires grad."""
    keep = torch.is_grad_enabled() and any(t.requires_grad for t in (s,) + tuple(params))
    return FusionFunction.apply(s, keep, m_attn, *params)
