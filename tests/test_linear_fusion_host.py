"""The linear and fusion nodes off the GPU: vge.linear's and vge.fusion's torch restatements against float64 autograd
of the module's own graph (the unfolded _Fusion behind F.layer_norm, and x @ W^T), the module with
linear_backend="hip" / fusion_backend="hip" on CPU tensors (where the functions run those restatements), and the
argument checks of the C entries, which all run before the first HIP call."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_ref as TR

FUSION_CASES = [(1, 1, 32), (5, 4, 64), (7, 5, 256)]
ENTRIES = ("vge_linear_workspace_bytes", "vge_linear_forward", "vge_linear_backward", "vge_fusion_workspace_bytes",
           "vge_fusion_forward_workspace_bytes", "vge_fusion_forward", "vge_fusion_backward")
BOUND = 1e-9        # of the tensor's largest magnitude: formula errors are O(1), float64 rounding over K <= 256 ~1e-13


def _fusion_module(M, D, seed):
    """A float64 _Fusion with every parameter moved off its initial value (logit_temp and logit_bias start at 0)."""
    from vge.model import _Fusion
    torch.manual_seed(seed)
    mod = _Fusion(D, M, 0.3).double().eval()
    with torch.no_grad():
        for p in mod.parameters():
            p.add_(0.3 * torch.randn_like(p))
    return mod


def _unfolded(mod, s, m_attn):
    """The module's graph, F.layer_norm in front, its dropout replaced by the given multiplier."""
    import math
    D = s.shape[-1]
    kv = mod.kv_ln(F.layer_norm(s, (D,)))
    q = mod.Wq(mod.q_ln(mod.latent)).view(D)
    logits = (mod.Wk(kv) @ q) / math.sqrt(D)
    logits = logits / (F.softplus(mod.logit_temp) + 1e-3) + mod.logit_bias
    attn = logits.softmax(dim=-1)
    if m_attn is not None:
        attn = attn * m_attn
    return mod.Wo((attn.unsqueeze(-1) * mod.Wv(kv)).sum(dim=-2))


def _close(name, got, want):
    scale = float(want.detach().abs().max())
    assert got.shape == want.shape, name
    err = float((got - want).detach().abs().max())
    assert err <= BOUND * max(scale, 1e-300), (name, err, scale)


def _mask(R, M, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(R, M, generator=g) >= 0.3).double() / 0.7


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", FUSION_CASES, ids=lambda c: "R%d_M%d_D%d" % c)
def test_fusion_restatements_equal_autograd_through_the_module(shape, masked):
    """float64: fusion_torch (folded) is the module's unfolded graph, fusion_backward_torch gives its autograd
    gradients of s and all eleven parameters, and FusionFunction on CPU tensors returns the same."""
    from vge import fusion as FU
    R, M, D = shape
    mod = _fusion_module(M, D, 100 * D + R)
    params = FU.fusion_params(mod)
    g = torch.Generator().manual_seed(D + R)
    s = (torch.randn(R, M, D, generator=g, dtype=torch.float64) * 1.7 + 0.4).requires_grad_(True)
    dy = torch.randn(R, D, generator=g, dtype=torch.float64)
    m_attn = _mask(R, M, 3 * D + R) if masked else None
    want = _unfolded(mod, s, m_attn)
    g_want = torch.autograd.grad(want, (s,) + params, dy)
    out, saved = FU.fusion_torch(s, params, m_attn, return_saved=True)
    _close("out", out, want)
    got = FU.fusion_backward_torch(dy, s.detach(), [p.detach() for p in params], [t.detach() for t in saved], m_attn)
    assert len(got) == 12
    for name, a, b in zip(("s",) + FU.ops.FUSION_PARAMS, got, g_want):
        _close(name, a, b)
    leaves = [s.detach().clone().requires_grad_(True)] + [p.detach().clone().requires_grad_(True) for p in params]
    out2 = FU.fusion(leaves[0], leaves[1:], m_attn)
    assert torch.equal(out2, out)
    out2.backward(dy)
    for name, t, b in zip(("s",) + FU.ops.FUSION_PARAMS, leaves, g_want):
        _close(name, t.grad, b)


@pytest.mark.parametrize("K", [3, 207, 1024])
def test_linear_restatements_equal_autograd(K):
    from vge import linear as LN
    g = torch.Generator().manual_seed(K)
    wide = torch.randn(2, 5, K + 40, generator=g, dtype=torch.float64)
    x = wide[..., 17:17 + K].requires_grad_(True)                  # a column slice, as a stem's input is
    W = torch.randn(64, K, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(2, 5, 64, generator=g, dtype=torch.float64)
    want = x @ W.t()
    gx, gW = torch.autograd.grad(want, (x, W), dy)
    _close("y", LN.linear_torch(x, W), want)
    dx, dW = LN.linear_backward_torch(dy, x.detach(), W.detach())
    _close("dx", dx, gx)
    _close("dW", dW, gW)
    assert LN.linear_backward_torch(dy, x.detach(), W.detach(), need_dx=False)[0] is None
    xl, Wl = x.detach().clone().requires_grad_(True), W.detach().clone().requires_grad_(True)
    y = LN.linear(xl, Wl)
    y.backward(dy)
    _close("function y", y, want)
    _close("function dx", xl.grad, gx)
    _close("function dW", Wl.grad, gW)
    rows = LN._rows(wide[..., 17:17 + K])
    assert rows.shape == (10, K) and rows.stride() == (K + 40, 1) and rows.data_ptr() == wide[..., 17:].data_ptr()
    assert LN._rows(wide.transpose(0, 1)[..., :K]) is None         # leading dimensions that do not collapse


def test_one_modality_has_exactly_zero_logit_gradients():
    """M = 1: the softmax is exactly 1 and dl = a (da - a da) is exactly 0, so the gradients of logit_temp, logit_bias,
    Wk, Wq, latent and q_ln are exactly 0."""
    from vge import fusion as FU
    mod = _fusion_module(1, 32, 5)
    leaves = [p.detach().clone().requires_grad_(True) for p in FU.fusion_params(mod)]
    g = torch.Generator().manual_seed(9)
    s = torch.randn(6, 1, 32, generator=g, dtype=torch.float64).requires_grad_(True)
    FU.fusion(s, leaves).backward(torch.randn(6, 32, generator=g, dtype=torch.float64))
    grads = dict(zip(FU.ops.FUSION_PARAMS, (t.grad for t in leaves)))
    for n in ("logit_temp", "logit_bias", "Wk", "Wq", "latent", "q_ln_weight", "q_ln_bias"):
        assert bool((grads[n] == 0).all()), n
    assert bool((grads["Wv"] != 0).any()) and bool((s.grad != 0).any())


def test_an_all_zero_mask_row_gives_a_zero_output_row():
    from vge import fusion as FU
    mod = _fusion_module(4, 64, 6)
    g = torch.Generator().manual_seed(10)
    s = torch.randn(5, 4, 64, generator=g, dtype=torch.float64)
    m = _mask(5, 4, 11)
    m[2] = 0.0
    out = FU.fusion_torch(s, FU.fusion_params(mod), m)
    assert bool((out[2] == 0).all()) and bool((out[1] != 0).any())


def test_functions_save_nothing_without_a_backward_to_follow(monkeypatch):
    from vge import fusion as FU, linear as LN
    mod = _fusion_module(4, 32, 1).float()
    params = FU.fusion_params(mod)
    s = torch.randn(3, 4, 32)
    asked = []
    real = FU.fusion_torch

    def spy(*a, return_saved=False, **k):
        asked.append(return_saved)
        return real(*a, return_saved=return_saved, **k)
    monkeypatch.setattr(FU, "fusion_torch", spy)
    with torch.no_grad():
        y0 = FU.fusion(s, params)
    y1 = FU.fusion(s, [p.detach() for p in params])
    y2 = FU.fusion(s, params)
    assert asked == [False, False, True]
    assert y0.grad_fn is None and y1.grad_fn is None and len(y2.grad_fn.saved_tensors) == 1 + 11 + 4
    assert torch.equal(y0, y2) and torch.equal(y1, y2)
    assert not FU.kernels_take(s, params)                           # CPU tensors
    W = torch.randn(32, 9, requires_grad=True)
    x = torch.randn(4, 9)
    with torch.no_grad():
        z0 = LN.linear(x, W)
    z1, z2 = LN.linear(x, W.detach()), LN.linear(x, W)
    assert z0.grad_fn is None and z1.grad_fn is None and len(z2.grad_fn.saved_tensors) == 2
    assert not LN.kernels_take(x, W)


def _two_modules(layout, dtype):
    from tests.golden.dataset_spec import SMALL_HP
    from vge import synth
    from vge.model import HumanActionScorer
    ref, sd = TR.module(layout, 0.0)
    mods = list(synth.DIMS_RAW)[:4 if layout == "nokp" else 5]
    hp = dict(SMALL_HP) if layout == "small" else {}
    hip = HumanActionScorer({k: synth.DIMS_RAW[k] for k in mods}, {k: synth.DIMS_DIFF[k] for k in mods},
                            dropout=0.0, linear_backend="hip", fusion_backend="hip", **hp)
    return TR.load(ref, sd).to(dtype), TR.load(hip, sd).to(dtype), sd


def test_hip_backends_module_on_the_cpu_in_float64():
    """The default module's state-dict keys and shapes; in float64 the three outputs and every parameter gradient equal
    the default module's within 1e-9 of the tensor's largest magnitude."""
    ref, hip, sd = _two_modules("small", torch.float64)
    assert (hip.linear_backend, hip.fusion_backend, hip.conv_backend, hip.time_backend) == ("hip", "hip", "torch", "torch")
    assert (ref.linear_backend, ref.fusion_backend) == ("torch", "torch")
    assert sorted(hip.state_dict()) == sorted(ref.state_dict()) == sorted(sd)
    assert {k: tuple(v.shape) for k, v in hip.state_dict().items()} == {k: tuple(np.shape(v)) for k, v in sd.items()}
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(3, 32, sum(ref.dims_raw.values()) + sum(ref.dims_diff.values()), generator=g,
                        dtype=torch.float64)
    w = [torch.randn(s, generator=g, dtype=torch.float64) for s in ((3, 64), (3, 33, 64), (3, 33, 64))]
    outs, grads = [], []
    for m in (ref, hip):
        m.train()
        o = m(feats)
        sum((a * b).sum() for a, b in zip(o, w)).backward()
        outs.append([t.detach() for t in o])
        grads.append({n: p.grad.clone() for n, p in m.named_parameters()})
    for i, (a, b) in enumerate(zip(outs[1], outs[0])):
        _close(f"output {i}", a, b)
    assert sorted(grads[0]) == sorted(grads[1])
    for n in grads[0]:
        _close(n, grads[1][n], grads[0][n])


def test_backends_are_independent_and_unknown_ones_are_refused():
    import inspect
    from vge import train as T
    from vge.model import FUSION_BACKENDS, LINEAR_BACKENDS, HumanActionScorer
    assert LINEAR_BACKENDS == FUSION_BACKENDS == ("torch", "hip")
    x = torch.randn(2, 32, 4)
    for lb in LINEAR_BACKENDS:
        for fb in FUSION_BACKENDS:
            m = HumanActionScorer({"a": 4}, {"a": 0}, d_model=32, time_layers=1, time_heads=2, linear_backend=lb,
                                  fusion_backend=fb, conv_backend="hip")
            assert (m.linear_backend, m.fusion_backend, m.conv_backend, m.time_backend) == (lb, fb, "hip", "torch")
            m(x)[0].sum().backward()                            # training mode, dropout 0.1, on the CPU fallbacks
            assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    for kw in ("linear_backend", "fusion_backend"):
        with pytest.raises(ValueError, match=kw):
            HumanActionScorer({"a": 4}, {"a": 0}, d_model=32, time_layers=1, time_heads=2, **{kw: "cuda"})
        assert inspect.signature(T.train).parameters[kw].default == "torch"
        with pytest.raises(SystemExit):
            T.main(["meshes", "--save-dir", "x", "--" + kw.replace("_", "-"), "cuda"])


# ----------------------------------------------------------------------------- the C entries, no GPU

VGE_ERR_ARG, VGE_ERR_WORKSPACE, VGE_ERR_UNSUPPORTED = 1, 6, 7
F_IN = ("s", "latent", "g_q", "b_q", "g_kv", "b_kv", "Wq", "Wk", "Wv", "Wo", "temp", "bias", "m_attn")
F_SAVED = ("stats", "a", "p", "vp")
F_GRADS = ("ds", "d_latent", "d_g_q", "d_b_q", "d_g_kv", "d_b_kv", "d_Wq", "d_Wk", "d_Wv", "d_Wo", "d_temp", "d_bias")
L_ALL = ("x", "W", "y", "dy", "dx", "dW", "ws")


def _fake(names, big=1 << 24):
    """Distinct, aligned, non-overlapping addresses for every buffer (never dereferenced: the checks come first)."""
    return {k: (1 << 36) + i * big for i, k in enumerate(names)}


def _ffwd(so, bufs, R, M, D, wsb, **over):
    q = dict(bufs, **over)
    return so.vge_fusion_forward(*[q[k] for k in F_IN], R, M, D, *[q[k] for k in F_SAVED], q["out"], q["ws"], wsb, None)


def _fbwd(so, bufs, R, M, D, wsb, **over):
    q = dict(bufs, **over)
    return so.vge_fusion_backward(q["d_out"], *[q[k] for k in F_IN], *[q[k] for k in F_SAVED], R, M, D,
                                  *[q[k] for k in F_GRADS], q["ws"], wsb, None)


@pytest.mark.parametrize("shape", [(4, 5, 48), (4, 5, 288), (4, 9, 64), (4, 0, 64), (0, 5, 64), (4, 5, 16),
                                   (1 << 21, 8, 256)], ids=lambda s: "R%d_M%d_D%d" % s)
def test_fusion_entries_refuse_unsupported_shapes(shape):
    from vge import lib as L
    so = L.load()
    p = _fake(F_IN + F_SAVED + F_GRADS + ("out", "d_out", "ws"))
    for call in (_ffwd, _fbwd):
        assert call(so, p, *shape, 1 << 40) == VGE_ERR_UNSUPPORTED
        assert b"vge_fusion" in so.vge_last_error()
    assert int(so.vge_fusion_workspace_bytes(*shape)) == 0
    assert int(so.vge_fusion_forward_workspace_bytes(*shape)) == 0


def test_fusion_entries_refuse_null_aliasing_and_a_short_workspace():
    from vge import lib as L
    so = L.load()
    a = (40, 5, 64)
    p = _fake(F_IN + F_SAVED + F_GRADS + ("out", "d_out", "ws"))
    wsb, fwd_wsb = int(so.vge_fusion_workspace_bytes(*a)), int(so.vge_fusion_forward_workspace_bytes(*a))
    assert 0 < fwd_wsb <= wsb < 1 << 24
    assert _ffwd(so, p, *a, wsb, out=None) == VGE_ERR_ARG and b"null out" in so.vge_last_error()
    assert _ffwd(so, p, *a, wsb, s=None) == VGE_ERR_ARG
    assert _ffwd(so, p, *a, wsb, vp=None) == VGE_ERR_ARG                  # the saved set: all four or none
    assert _fbwd(so, p, *a, wsb, stats=None) == VGE_ERR_ARG
    assert _fbwd(so, p, *a, wsb, d_Wk=None) == VGE_ERR_ARG and b"null d_Wk" in so.vge_last_error()
    assert _ffwd(so, p, *a, wsb, out=p["s"]) == VGE_ERR_ARG and b"alias" in so.vge_last_error()
    assert _ffwd(so, p, *a, wsb, p=p["vp"]) == VGE_ERR_ARG
    assert _ffwd(so, p, *a, wsb, ws=p["out"] + 16) == VGE_ERR_ARG
    assert _fbwd(so, p, *a, wsb, ds=p["d_out"]) == VGE_ERR_ARG and b"alias" in so.vge_last_error()
    assert _fbwd(so, p, *a, wsb, d_temp=p["d_bias"]) == VGE_ERR_ARG
    assert _ffwd(so, p, *a, wsb, s=p["s"] + 4) == VGE_ERR_ARG and b"aligned" in so.vge_last_error()
    assert _ffwd(so, p, *a, fwd_wsb - 1) == VGE_ERR_WORKSPACE
    assert b"vge_fusion_forward_workspace_bytes" in so.vge_last_error()
    assert _fbwd(so, p, *a, wsb - 1) == VGE_ERR_WORKSPACE and b"vge_fusion_workspace_bytes" in so.vge_last_error()


def _lfwd(so, bufs, R, K, N, ldx, **over):
    q = dict(bufs, **over)
    return so.vge_linear_forward(q["x"], ldx, q["W"], q["y"], R, K, N, None)


def _lbwd(so, bufs, R, K, N, ldx, wsb, **over):
    q = dict(bufs, **over)
    return so.vge_linear_backward(q["dy"], q["x"], ldx, q["W"], q["dx"], q["dW"], q["ws"], wsb, R, K, N, None)


def test_linear_entries_refuse_bad_arguments():
    from vge import lib as L
    so = L.load()
    p = _fake(L_ALL)
    for R, K, N, ldx in ((4, 0, 64, 8), (4, 4097, 64, 4097), (4, 8, 48, 8), (4, 8, 16, 8), (4, 8, 288, 8), (0, 8, 64, 8),
                         (1 << 20, 8, 64, 2596)):
        assert _lfwd(so, p, R, K, N, ldx) == VGE_ERR_UNSUPPORTED and b"vge_linear_forward" in so.vge_last_error()
        assert _lbwd(so, p, R, K, N, ldx, 1 << 40) == VGE_ERR_UNSUPPORTED
        if ldx * R < 2 ** 31:                                    # the query does not see ldx
            assert int(so.vge_linear_workspace_bytes(R, K, N)) == 0
    a = (40, 207, 64, 2596)
    wsb = int(so.vge_linear_workspace_bytes(40, 207, 64))
    assert 0 < wsb < 1 << 24
    assert _lfwd(so, p, 40, 207, 64, 206) == VGE_ERR_ARG and _lbwd(so, p, 40, 207, 64, 206, wsb) == VGE_ERR_ARG
    assert _lfwd(so, p, *a, y=None) == VGE_ERR_ARG and b"null y" in so.vge_last_error()
    assert _lbwd(so, p, *a, wsb, dW=None) == VGE_ERR_ARG and b"null dW" in so.vge_last_error()
    assert _lfwd(so, p, *a, y=p["x"]) == VGE_ERR_ARG and b"alias" in so.vge_last_error()
    assert _lbwd(so, p, *a, wsb, dx=p["dy"]) == VGE_ERR_ARG and b"alias" in so.vge_last_error()
    assert _lfwd(so, p, *a, x=p["x"] + 2) == VGE_ERR_ARG and b"4-byte aligned" in so.vge_last_error()
    assert _lfwd(so, p, *a, W=p["W"] + 4) == VGE_ERR_ARG and b"16-byte aligned" in so.vge_last_error()
    assert _lbwd(so, p, *a, wsb - 1) == VGE_ERR_WORKSPACE and b"vge_linear_workspace_bytes" in so.vge_last_error()


def test_header_declares_and_library_exports_the_entries():
    from vge import lib as L
    so = L.load()
    header = (Path(__file__).resolve().parents[1] / "include" / "vge.h").read_text()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(so, name) and name in L.EXPORTS
        if name.endswith("workspace_bytes"):
            assert getattr(so, name).restype is C.c_size_t
    assert 0 < so.vge_fusion_workspace_bytes(33, 5, 256) < so.vge_fusion_workspace_bytes(7680, 5, 256)
    assert 0 < so.vge_linear_workspace_bytes(7680, 3, 256) < so.vge_linear_workspace_bytes(7680, 1024, 256)
