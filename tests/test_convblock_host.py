"""The conv block off the GPU: vge.convblock's torch restatements against float64 autograd of vge.model._Block, the
module with conv_backend="hip" on CPU tensors (where ConvBlockFunction runs those restatements), and the argument
checks of vge_convblock_forward / vge_convblock_backward, which all run before the first HIP call."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import train_ref as TR

CASES = [(2, 7, 32, 1), (1, 1, 32, 8), (3, 9, 64, 8), (2, 33, 96, 4)]
NAMES = ("dx", "dw1", "dw2", "dgamma", "dbeta")


def _inputs(B, T, Cn, masked, zero_sample, dtype=torch.float64):
    g = torch.Generator().manual_seed(1000 * B + 10 * T + Cn)
    x = torch.randn(B, T, Cn, generator=g, dtype=dtype)
    if zero_sample:
        x[B - 1] = 0.0        # conv of zeros is zero, gelu(0) = 0: the sample's variance is 0 and rstd = 1 / sqrt(eps)
    w1, w2 = (torch.randn(Cn, Cn, 5, generator=g, dtype=dtype) / (5 * Cn) ** 0.5 for _ in range(2))
    gamma = 1.0 + 0.3 * torch.randn(Cn, generator=g, dtype=dtype)
    beta = 0.2 * torch.randn(Cn, generator=g, dtype=dtype)
    mask = (torch.rand(B, T, Cn, generator=g) >= 0.3).to(dtype) / 0.7 if masked else None
    dy = torch.randn(B, T, Cn, generator=g, dtype=dtype)
    return x, w1, w2, gamma, beta, mask, dy


def _block(Cn, dil, w1, w2, gamma, beta):
    from vge.model import _Block
    blk = _Block(Cn, dil, 0.0).to(w1.dtype)
    with torch.no_grad():
        blk.conv1.weight.copy_(w1)
        blk.conv2.weight.copy_(w2)
        blk.norm.weight.copy_(gamma)
        blk.norm.bias.copy_(beta)
    return blk


def _block_autograd(blk, x, mask, dy):
    """y and the five gradients of _Block by autograd; the mask enters as _Block's dropout does (after GELU)."""
    import torch.nn.functional as F
    xr = x.clone().requires_grad_(True)
    h = F.gelu(blk.conv1(xr))
    if mask is not None:
        h = h * mask
    y = blk.norm(F.gelu(blk.conv2(h) + xr))
    grads = torch.autograd.grad(y, (xr, blk.conv1.weight, blk.conv2.weight, blk.norm.weight, blk.norm.bias), dy)
    return y.detach(), grads


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("zero_sample", [False, True], ids=["", "zero_sample"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_T%d_C%d_d%d" % c)
def test_backward_restatement_equals_float64_autograd(case, masked, zero_sample):
    from vge import convblock as CB
    B, T, Cn, dil = case
    x, w1, w2, gamma, beta, mask, dy = _inputs(B, T, Cn, masked, zero_sample)
    blk = _block(Cn, dil, w1, w2, gamma, beta)
    y_ref, g_ref = _block_autograd(blk, x, mask, dy)
    y, saved = CB.convblock_torch(x, w1, w2, gamma, beta, dil, mask, return_saved=True)
    assert _rel(y, y_ref) <= 1e-10
    if zero_sample:
        assert float(saved[3][B - 1]) == pytest.approx(1e-5 ** -0.5, rel=1e-12)
    got = CB.convblock_backward_torch(dy, x, w1, w2, gamma, dil, saved, mask)
    for name, a, b in zip(NAMES, got, g_ref):
        assert a.shape == b.shape, name
        assert _rel(a, b) <= 1e-10, (name, _rel(a, b))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_T%d_C%d_d%d" % c)
def test_forward_restatement_equals_the_block(case):
    from vge import convblock as CB
    B, T, Cn, dil = case
    for dtype in (torch.float32, torch.float64):
        x, w1, w2, gamma, beta, _, dy = _inputs(B, T, Cn, False, False, dtype)
        blk = _block(Cn, dil, w1, w2, gamma, beta)
        assert torch.equal(CB.convblock_torch(x, w1, w2, gamma, beta, dil), blk(x))
        # the autograd function on CPU tensors: the same forward, the restated backward
        xr = x.clone().requires_grad_(True)
        y = CB.convblock(xr, w1, w2, gamma, beta, dil)
        assert torch.equal(y, blk(x))
        with torch.no_grad():
            assert torch.equal(CB.convblock(xr, w1, w2, gamma, beta, dil), y)


def test_function_saves_nothing_without_a_backward_to_follow(monkeypatch):
    """Under torch.no_grad() with parameters that require grad, and with grad mode on but no input requiring grad, the
    function does not ask for the saved set and keeps no tensor; with a backward to follow it does."""
    from vge import convblock as CB
    x, w1, w2, gamma, beta, mask, _ = _inputs(2, 7, 32, True, False, torch.float32)
    params = [t.clone().requires_grad_(True) for t in (w1, w2, gamma, beta)]
    asked = []
    real = CB.convblock_torch

    def spy(*a, return_saved=False, **k):
        asked.append(return_saved)
        return real(*a, return_saved=return_saved, **k)
    monkeypatch.setattr(CB, "convblock_torch", spy)
    with torch.no_grad():
        y0 = CB.convblock(x, *params, 1, mask)
    y1 = CB.convblock(x, w1, w2, gamma, beta, 1, mask)
    y2 = CB.convblock(x, *params, 1, mask)
    assert asked == [False, False, True]
    assert y0.grad_fn is None and y1.grad_fn is None and len(y2.grad_fn.saved_tensors) == 9
    assert torch.equal(y0, y2) and torch.equal(y1, y2)


def _two_modules(layout, dropout=0.0, dtype=torch.float32):
    from vge.model import HumanActionScorer
    from tests.golden.dataset_spec import SMALL_HP
    from vge import synth
    ref, sd = TR.module(layout, dropout)
    mods = list(synth.DIMS_RAW)[:4 if layout == "nokp" else 5]
    hp = dict(SMALL_HP) if layout == "small" else {}
    hip = HumanActionScorer({k: synth.DIMS_RAW[k] for k in mods}, {k: synth.DIMS_DIFF[k] for k in mods},
                            dropout=dropout, conv_backend="hip", **hp)
    return TR.load(ref, sd).to(dtype), TR.load(hip, sd).to(dtype), sd


@pytest.mark.parametrize("layout", ["kp", "small"])
def test_hip_backend_module_on_the_cpu(layout):
    ref, hip, sd = _two_modules(layout)
    assert hip.conv_backend == "hip" and ref.conv_backend == "torch"
    assert sorted(hip.state_dict()) == sorted(sd)
    assert {k: tuple(v.shape) for k, v in hip.state_dict().items()} == {k: tuple(np.shape(v)) for k, v in sd.items()}
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(3, 32, sum(ref.dims_raw.values()) + sum(ref.dims_diff.values()), generator=g)
    ref.eval(), hip.eval()
    with torch.no_grad():
        assert torch.equal(hip(feats)[0], ref(feats)[0])


def test_hip_backend_module_float64_gradients_on_the_cpu():
    ref, hip, _ = _two_modules("small", dtype=torch.float64)
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(3, 32, sum(ref.dims_raw.values()) + sum(ref.dims_diff.values()), generator=g,
                        dtype=torch.float64)
    w = torch.randn(3, ref.hyper_parameters["d_model"], generator=g, dtype=torch.float64)
    grads = []
    for m in (ref, hip):
        m.train()
        (m(feats)[0] * w).sum().backward()
        grads.append({n: p.grad.clone() for n, p in m.named_parameters()})
    assert sorted(grads[0]) == sorted(grads[1])
    for n in grads[0]:
        assert _rel(grads[1][n], grads[0][n]) <= 1e-9, n


def test_unknown_conv_backend_is_refused():
    from vge.model import HumanActionScorer, _Block
    with pytest.raises(ValueError, match="conv_backend"):
        HumanActionScorer({"a": 4}, {"a": 0}, d_model=32, time_layers=1, time_heads=2, conv_backend="cuda")
    with pytest.raises(ValueError, match="conv_backend"):
        _Block(32, 1, 0.0, conv_backend="cuda")


# ----------------------------------------------------------------------------- the C entries, no GPU

VGE_ERR_ARG, VGE_ERR_WORKSPACE, VGE_ERR_UNSUPPORTED = 1, 6, 7


def _fake(so, B, T, Cn):
    """Distinct, aligned, non-overlapping addresses for every buffer (never dereferenced: the checks come first)."""
    act, wb = max(B * T * Cn * 4, 16), 5 * 256 * 256 * 4
    ws_bytes = int(so.vge_convblock_workspace_bytes(B, T, Cn))
    sizes = {"x": act, "w1": wb, "w2": wb, "mask": act, "gamma": 1024, "beta": 1024, "a": act, "u": act, "mean": 4096,
             "rstd": 4096, "y": act, "dy": act, "dx": act, "dw1": wb, "dw2": wb, "dgamma": 1024, "dbeta": 1024,
             "ws": max(ws_bytes, 16)}
    p, at = {}, 1 << 32
    for k, n in sizes.items():
        p[k] = at
        at += (n + 4095) // 4096 * 4096
    return p, ws_bytes


def _fwd(so, p, B, T, Cn, dil, wsb, **over):
    q = dict(p, **over)
    return so.vge_convblock_forward(q["x"], q["w1"], q["w2"], q["mask"], q["gamma"], q["beta"], B, T, Cn, dil, q["a"],
                                    q["u"], q["mean"], q["rstd"], q["y"], q["ws"], wsb, None)


def _bwd(so, p, B, T, Cn, dil, wsb, **over):
    q = dict(p, **over)
    return so.vge_convblock_backward(q["dy"], q["x"], q["w1"], q["w2"], q["mask"], q["gamma"], q["a"], q["u"],
                                     q["mean"], q["rstd"], B, T, Cn, dil, q["dx"], q["dw1"], q["dw2"], q["dgamma"],
                                     q["dbeta"], q["ws"], wsb, None)


@pytest.mark.parametrize("shape", [(2, 8, 48, 1), (2, 8, 288, 1), (2, 0, 64, 1), (2, 65, 64, 1), (0, 8, 64, 1),
                                   (2, 8, 64, 3)], ids=lambda s: "B%d_T%d_C%d_d%d" % s)
def test_entries_refuse_unsupported_shapes(shape):
    from vge import lib as L
    so = L.load()
    B, T, Cn, dil = shape
    p, _ = _fake(so, max(B, 1), max(T, 1), 64)
    for call in (_fwd, _bwd):
        assert call(so, p, B, T, Cn, dil, 1 << 40) == VGE_ERR_UNSUPPORTED
        assert b"vge_convblock" in so.vge_last_error()
    if dil == 1:
        assert int(so.vge_convblock_workspace_bytes(B, T, Cn)) == 0


def test_entries_refuse_null_aliasing_and_a_short_workspace():
    from vge import lib as L
    so = L.load()
    B, T, Cn, dil = 3, 9, 64, 2
    p, wsb = _fake(so, B, T, Cn)
    assert wsb > 0
    assert _fwd(so, p, B, T, Cn, dil, wsb, y=None) == VGE_ERR_ARG and b"null y" in so.vge_last_error()
    assert _bwd(so, p, B, T, Cn, dil, wsb, dw2=None) == VGE_ERR_ARG and b"null dw2" in so.vge_last_error()
    assert _fwd(so, p, B, T, Cn, dil, wsb, x=None) == VGE_ERR_ARG
    assert _fwd(so, p, B, T, Cn, dil, wsb, u=None) == VGE_ERR_ARG          # the saved set: all four or none
    assert _fwd(so, p, B, T, Cn, dil, wsb, y=p["x"]) == VGE_ERR_ARG and b"alias" in so.vge_last_error()
    assert _fwd(so, p, B, T, Cn, dil, wsb, a=p["u"]) == VGE_ERR_ARG
    assert _fwd(so, p, B, T, Cn, dil, wsb, ws=p["y"] + 16) == VGE_ERR_ARG
    assert _bwd(so, p, B, T, Cn, dil, wsb, dx=p["dy"]) == VGE_ERR_ARG and b"alias" in so.vge_last_error()
    assert _bwd(so, p, B, T, Cn, dil, wsb, dgamma=p["dbeta"]) == VGE_ERR_ARG
    assert _fwd(so, p, B, T, Cn, dil, wsb, x=p["x"] + 4) == VGE_ERR_ARG and b"aligned" in so.vge_last_error()
    fwd_wsb = int(so.vge_convblock_forward_workspace_bytes(Cn))         # the forward needs its two weight images only
    assert fwd_wsb == 2 * 5 * Cn * Cn * 4 and fwd_wsb < wsb
    assert _fwd(so, p, B, T, Cn, dil, fwd_wsb - 1) == VGE_ERR_WORKSPACE
    assert b"vge_convblock_forward_workspace_bytes" in so.vge_last_error()
    assert _bwd(so, p, B, T, Cn, dil, wsb - 1) == VGE_ERR_WORKSPACE
    assert b"vge_convblock_workspace_bytes" in so.vge_last_error()


def test_library_has_the_three_symbols():
    from vge import lib as L
    so = L.load()
    for name in ("vge_convblock_forward", "vge_convblock_backward", "vge_convblock_workspace_bytes",
                 "vge_convblock_forward_workspace_bytes"):
        assert hasattr(so, name) and name in L.EXPORTS
    assert so.vge_convblock_workspace_bytes.restype is C.c_size_t
    # the workspace grows with the batch and does not depend on the dilation
    assert 0 < so.vge_convblock_workspace_bytes(1, 32, 256) < so.vge_convblock_workspace_bytes(240, 32, 256)
