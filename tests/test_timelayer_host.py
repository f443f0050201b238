"""The temporal layer off the GPU: vge.timelayer's torch restatements against float64 autograd of torch's own
nn.TransformerEncoderLayer, the module with time_backend="hip" on CPU tensors (where TimeLayerFunction runs those
restatements), and the argument checks of vge_timelayer_forward / vge_timelayer_backward, which all run before the first
HIP call."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from torch.nn.attention import SDPBackend, sdpa_kernel

from tests import train_ref as TR

DH = [(32, 2), (64, 4), (96, 2), (256, 8)]
SS = [1, 5, 33]
ENTRIES = ("vge_timelayer_workspace_bytes", "vge_timelayer_forward_workspace_bytes", "vge_timelayer_forward",
           "vge_timelayer_backward")


def _layer(D, H, seed):
    """A float64 eval-mode torch layer with every parameter moved off its initial value (biases are 0, norms 1)."""
    torch.manual_seed(seed)
    layer = torch.nn.TransformerEncoderLayer(D, H, 4 * D, 0.0, batch_first=True).double().eval()
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(0.1 * torch.randn_like(p))
    return layer


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("dh", DH, ids=lambda c: "D%d_H%d" % c)
def test_forward_and_autograd_equal_the_torch_layer(dh, S):
    """float64, dropout 0: timelayer_torch on the layer's parameters is the layer (1e-10), and its autograd gradients
    of all 13 tensors are the layer's (1e-10 relative)."""
    from vge import timelayer as TL
    D, H = dh
    layer = _layer(D, H, 100 * D + S)
    params = TL.layer_params(layer)
    g = torch.Generator().manual_seed(D + S)
    x = torch.randn(2, S, D, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(2, S, D, generator=g, dtype=torch.float64)
    with sdpa_kernel(SDPBackend.MATH):
        want = layer(x)
    got = TL.timelayer_torch(x, params, H)
    assert float((got - want).abs().max()) <= 1e-10
    g_want = torch.autograd.grad(want, (x,) + params, dy)
    g_got = torch.autograd.grad(got, (x,) + params, dy)
    for name, a, b in zip(("x",) + TL.ops.TIMELAYER_PARAMS, g_got, g_want):
        assert a.shape == b.shape and _rel(a, b) <= 1e-10, (name, _rel(a, b))


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("dh", DH, ids=lambda c: "D%d_H%d" % c)
def test_backward_restatement_equals_autograd(dh, S, masked):
    """timelayer_backward_torch (the header's formulas) against autograd of timelayer_torch, with all four masks at
    p = 0.3 and with none; TimeLayerFunction on CPU tensors returns the same."""
    from vge import timelayer as TL
    D, H = dh
    layer = _layer(D, H, 7 * D + S)
    params = tuple(p.detach() for p in TL.layer_params(layer))
    g = torch.Generator().manual_seed(3 * D + S)
    x = torch.randn(3, S, D, generator=g, dtype=torch.float64)
    dy = torch.randn(3, S, D, generator=g, dtype=torch.float64)
    masks = None
    if masked:
        masks = tuple((torch.rand(s, generator=g) >= 0.3).double() / 0.7
                      for s in ((3, H, S, S), (3, S, D), (3, S, 4 * D), (3, S, D)))
    leaves = [x.clone().requires_grad_(True)] + [p.clone().requires_grad_(True) for p in params]
    y, saved = TL.timelayer_torch(leaves[0], leaves[1:], H, masks, return_saved=True)
    want = torch.autograd.grad(y, leaves, dy)
    got = TL.timelayer_backward_torch(dy, x, params, H, [s.detach() for s in saved], masks)
    assert len(got) == 13
    for name, a, b in zip(("x",) + TL.ops.TIMELAYER_PARAMS, got, want):
        assert a.shape == b.shape and _rel(a, b) <= 1e-10, (name, _rel(a, b))
    leaves2 = [t.detach().clone().requires_grad_(True) for t in leaves]
    y2 = TL.timelayer(leaves2[0], leaves2[1:], H, masks)
    assert torch.equal(y2, y)
    y2.backward(dy)
    for name, t, b in zip(("x",) + TL.ops.TIMELAYER_PARAMS, leaves2, want):
        assert _rel(t.grad, b) <= 1e-10, name


def test_function_saves_nothing_without_a_backward_to_follow(monkeypatch):
    from vge import timelayer as TL
    layer = _layer(32, 2, 1).float()
    params = TL.layer_params(layer)
    x = torch.randn(2, 5, 32)
    asked = []
    real = TL.timelayer_torch

    def spy(*a, return_saved=False, **k):
        asked.append(return_saved)
        return real(*a, return_saved=return_saved, **k)
    monkeypatch.setattr(TL, "timelayer_torch", spy)
    with torch.no_grad():
        y0 = TL.timelayer(x, params, 2)
    y1 = TL.timelayer(x, [p.detach() for p in params], 2)
    y2 = TL.timelayer(x, params, 2)
    assert asked == [False, False, True]
    assert y0.grad_fn is None and y1.grad_fn is None and len(y2.grad_fn.saved_tensors) == 1 + 12 + 5
    assert torch.equal(y0, y2) and torch.equal(y1, y2)


def test_kernels_take_only_what_the_entries_accept():
    from vge import timelayer as TL
    layer = _layer(32, 2, 1).float()
    assert not TL.kernels_take(torch.randn(2, 5, 32), TL.layer_params(layer), 2)        # CPU tensors


def _two_modules(layout, dtype=torch.float32):
    from tests.golden.dataset_spec import SMALL_HP
    from vge import synth
    from vge.model import HumanActionScorer
    ref, sd = TR.module(layout, 0.0)
    mods = list(synth.DIMS_RAW)[:4 if layout == "nokp" else 5]
    hp = dict(SMALL_HP) if layout == "small" else {}
    hip = HumanActionScorer({k: synth.DIMS_RAW[k] for k in mods}, {k: synth.DIMS_DIFF[k] for k in mods},
                            dropout=0.0, time_backend="hip", **hp)
    return TR.load(ref, sd).to(dtype), TR.load(hip, sd).to(dtype), sd


@pytest.mark.parametrize("layout", ["kp", "small"])
def test_hip_backend_module_on_the_cpu(layout):
    """The same state-dict keys and shapes under both backends; on the CPU "hip" falls back to the torch restatement:
    eval-mode outputs within 1e-6 in float32, from one state dict loaded both ways."""
    ref, hip, sd = _two_modules(layout)
    assert hip.time_backend == "hip" and ref.time_backend == "torch" and hip.conv_backend == "torch"
    assert sorted(hip.state_dict()) == sorted(ref.state_dict()) == sorted(sd)
    assert {k: tuple(v.shape) for k, v in hip.state_dict().items()} == {k: tuple(np.shape(v)) for k, v in sd.items()}
    ref.load_state_dict(hip.state_dict())                      # a checkpoint moves between the backends
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(3, 32, sum(ref.dims_raw.values()) + sum(ref.dims_diff.values()), generator=g)
    ref.eval(), hip.eval()
    with torch.no_grad():
        got, want = hip(feats), ref(feats)
        for a, b in zip(got[:2], want[:2]):                    # the two L2-normalised embeddings: absolute
            assert float((a - b).abs().max()) <= 1e-6
        # the unnormalised tokens reach |4.3|, where 1e-6 is two float32 ulps: relative to their largest magnitude
        assert _rel(got[2], want[2]) <= 1e-6


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


def test_all_four_backend_combinations_construct_and_unknown_ones_are_refused():
    from vge.model import CONV_BACKENDS, TIME_BACKENDS, HumanActionScorer
    assert TIME_BACKENDS == ("torch", "hip")
    x = torch.randn(2, 32, 4)
    for cb in CONV_BACKENDS:
        for tb in TIME_BACKENDS:
            m = HumanActionScorer({"a": 4}, {"a": 0}, d_model=32, time_layers=1, time_heads=2, conv_backend=cb,
                                  time_backend=tb)
            assert (m.conv_backend, m.time_backend) == (cb, tb)
            m(x)[0].sum().backward()                            # training mode, dropout 0.1, on the CPU fallbacks
            assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.temporal.parameters())
    with pytest.raises(ValueError, match="time_backend"):
        HumanActionScorer({"a": 4}, {"a": 0}, d_model=32, time_layers=1, time_heads=2, time_backend="cuda")


def test_train_takes_the_backend_on_the_command_line():
    import inspect
    from vge import train as T
    assert inspect.signature(T.train).parameters["time_backend"].default == "torch"
    with pytest.raises(SystemExit):
        T.main(["meshes", "--save-dir", "x", "--time-backend", "cuda"])


# ----------------------------------------------------------------------------- the C entries, no GPU

VGE_ERR_ARG, VGE_ERR_WORKSPACE, VGE_ERR_UNSUPPORTED = 1, 6, 7
FWD = ("x", "in_w", "in_b", "out_w", "out_b", "w1", "c1", "w2", "c2", "g1", "be1", "g2", "be2", "m_attn", "m1", "m_ff",
       "m2", "qkv", "u1", "f", "u2", "stats", "y", "ws")
BWD_IN = ("dy", "x", "in_w", "out_w", "w1", "w2", "g1", "be1", "g2", "m_attn", "m1", "m_ff", "m2", "qkv", "u1", "f", "u2",
          "stats")
BWD_OUT = ("dx", "d_in_w", "d_in_b", "d_out_w", "d_out_b", "d_w1", "d_c1", "d_w2", "d_c2", "d_g1", "d_be1", "d_g2",
           "d_be2", "ws")


def _fake(so, B, S, D, H):
    """Distinct, aligned, non-overlapping addresses for every buffer (never dereferenced: the checks come first)."""
    big = 4 * max(B, 1) * 65 * 1024 * 4 + max(B, 1) * 16 * 65 * 65 * 4
    ws_bytes = int(so.vge_timelayer_workspace_bytes(B, S, D, H, 4 * D))
    p, at = {}, 1 << 36
    for k in dict.fromkeys(FWD + BWD_IN + BWD_OUT):
        p[k] = at
        at += ((max(ws_bytes, 16) if k == "ws" else big) + 4095) // 4096 * 4096
    return p, ws_bytes


def _fwd(so, p, B, S, D, H, F_, wsb, **over):
    q = dict(p, **over)
    return so.vge_timelayer_forward(*[q[k] for k in FWD[:17]], B, S, D, H, F_, *[q[k] for k in FWD[17:]], wsb, None)


def _bwd(so, p, B, S, D, H, F_, wsb, **over):
    q = dict(p, **over)
    return so.vge_timelayer_backward(*[q[k] for k in BWD_IN], B, S, D, H, F_, *[q[k] for k in BWD_OUT], wsb, None)


@pytest.mark.parametrize("shape", [(2, 66, 64, 4, 256), (2, 0, 64, 4, 256), (2, 8, 48, 3, 192), (2, 8, 288, 8, 1152),
                                   (2, 8, 32, 4, 128), (2, 8, 64, 4, 128), (0, 8, 64, 4, 256), (2, 8, 64, 3, 256),
                                   (2, 8, 256, 2, 1024)], ids=lambda s: "B%d_S%d_D%d_H%d_F%d" % s)
def test_entries_refuse_unsupported_shapes(shape):
    from vge import lib as L
    so = L.load()
    B, S, D, H, F_ = shape
    p, _ = _fake(so, 2, 8, 64, 4)
    for call in (_fwd, _bwd):
        assert call(so, p, B, S, D, H, F_, 1 << 40) == VGE_ERR_UNSUPPORTED
        assert b"vge_timelayer" in so.vge_last_error()
    assert int(so.vge_timelayer_workspace_bytes(B, S, D, H, F_)) == 0
    assert int(so.vge_timelayer_forward_workspace_bytes(B, S, D, H, F_)) == 0


def test_entries_refuse_null_aliasing_and_a_short_workspace():
    from vge import lib as L
    so = L.load()
    B, S, D, H = 3, 9, 64, 4
    F_ = 4 * D
    p, wsb = _fake(so, B, S, D, H)
    a = (B, S, D, H, F_)
    fwd_wsb = int(so.vge_timelayer_forward_workspace_bytes(*a))
    assert 0 < fwd_wsb <= wsb
    assert _fwd(so, p, *a, wsb, y=None) == VGE_ERR_ARG and b"null y" in so.vge_last_error()
    assert _bwd(so, p, *a, wsb, d_w2=None) == VGE_ERR_ARG and b"null d_linear2_weight" in so.vge_last_error()
    assert _fwd(so, p, *a, wsb, x=None) == VGE_ERR_ARG
    assert _fwd(so, p, *a, wsb, u2=None) == VGE_ERR_ARG                  # the saved set: all five or none
    assert _bwd(so, p, *a, wsb, stats=None) == VGE_ERR_ARG
    assert _fwd(so, p, *a, wsb, y=p["x"]) == VGE_ERR_ARG and b"alias" in so.vge_last_error()
    assert _fwd(so, p, *a, wsb, qkv=p["f"]) == VGE_ERR_ARG
    assert _fwd(so, p, *a, wsb, ws=p["y"] + 16) == VGE_ERR_ARG
    assert _bwd(so, p, *a, wsb, dx=p["dy"]) == VGE_ERR_ARG and b"alias" in so.vge_last_error()
    assert _bwd(so, p, *a, wsb, d_g1=p["d_be1"]) == VGE_ERR_ARG
    assert _fwd(so, p, *a, wsb, x=p["x"] + 4) == VGE_ERR_ARG and b"aligned" in so.vge_last_error()
    assert _fwd(so, p, *a, wsb, m_ff=p["m_ff"] + 8) == VGE_ERR_ARG
    assert _fwd(so, p, *a, fwd_wsb - 1) == VGE_ERR_WORKSPACE
    assert b"vge_timelayer_forward_workspace_bytes" in so.vge_last_error()
    assert _bwd(so, p, *a, wsb - 1) == VGE_ERR_WORKSPACE
    assert b"vge_timelayer_workspace_bytes" in so.vge_last_error()


def test_header_declares_and_library_exports_the_four_entries():
    from vge import lib as L
    so = L.load()
    header = (Path(__file__).resolve().parents[1] / "include" / "vge.h").read_text()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(so, name) and name in L.EXPORTS
    assert so.vge_timelayer_workspace_bytes.restype is C.c_size_t
    assert so.vge_timelayer_forward_workspace_bytes.restype is C.c_size_t
    # the workspace grows with the batch; head dimension 8 is refused, 16 is taken
    assert 0 < so.vge_timelayer_workspace_bytes(1, 33, 256, 8, 1024) < so.vge_timelayer_workspace_bytes(240, 33, 256, 8, 1024)
    assert so.vge_timelayer_workspace_bytes(2, 33, 32, 4, 128) == 0 < so.vge_timelayer_workspace_bytes(2, 33, 32, 2, 128)
