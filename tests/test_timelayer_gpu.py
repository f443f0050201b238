"""The temporal layer's forward and backward kernels (vge_timelayer.hip) on the GPU, through vge.ops, vge.timelayer and
the module with time_backend="hip".

Reference and bar.  The reference is float64 autograd of vge.timelayer.timelayer_torch on the CPU, on the same inputs
and masks.  Per tensor -- y and each of the 13 gradients -- max|gpu - f64| <= 8 r, r being the distance of the float32
CPU autograd from the float64 one, floored at one float32 ulp of the tensor's largest float64 magnitude (DESIGN.md 5e,
tests/test_convblock_gpu.py::_check).  Every test prints its ratios.

Measured on an MI355X, largest max|gpu - f64| / r per tensor (bar 8) over the seven shapes with and without masks, the
two all-zero masks, x scaled by 10, the logit 60 above the others and the autograd function:
  y 1.11  dx 1.92  in_proj_weight 1.94  in_proj_bias 1.87  out_proj_weight 1.22  out_proj_bias 1.03
  linear1_weight 0.75  linear1_bias 0.99  linear2_weight 1.07  linear2_bias 1.72
  norm1_weight 1.16  norm1_bias 1.20  norm2_weight 1.14  norm2_bias 0.48
(the largest at B = 1, S = 1, D = 32, where r is a few ulps).  The module-level tests carry their own figures; all of
them are in DESIGN.md 5e."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import train_ref as TR
from tests import validate_ref as R
from tests.test_convblock_gpu import _ReplayedDropout, tgold, train_setup  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = -12345.0
PARAMS = ("in_proj_weight", "in_proj_bias", "out_proj_weight", "out_proj_bias", "linear1_weight", "linear1_bias",
          "linear2_weight", "linear2_bias", "norm1_weight", "norm1_bias", "norm2_weight", "norm2_bias")
NAMES = ("y", "dx") + tuple("d_" + n for n in PARAMS)
SAVED = ("qkv", "u1", "f", "u2", "stats")

# (B, S, D, H)
CASES = [(1, 1, 32, 2),        # one token: the softmax is exactly 1, dq and dk exactly 0; head dimension 16
         (2, 5, 64, 4),        # the small golden checkpoint's shape
         (5, 16, 256, 16),     # 16 heads
         (3, 17, 96, 2),       # head dimension 48; D not a power of two; rows not a multiple of any tile
         (2, 33, 256, 8),      # the training shape
         (2, 65, 192, 3),      # the largest S (two keys per lane in the softmax), head dimension 64
         (17, 33, 256, 8)]     # 561 rows: the weight gradient's 8th chunk holds one row
VARIANTS = ("nomask", "mask")


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _shapes(B, S, D, H):
    from vge import ops
    return ops._timelayer_shapes(B, S, D, H, 4 * D)


@functools.lru_cache(maxsize=None)
def _case(shape, variant):
    """Inputs (float32 torch, CPU) and the CPU references of one case, computed once: {name: (f64, f32)}."""
    from vge import timelayer as TL
    B, S, D, H = shape
    sh = _shapes(B, S, D, H)
    g = torch.Generator().manual_seed(7919 * B + 31 * S + D + H)
    x = torch.randn(B, S, D, generator=g)
    params = []
    for n in PARAMS:
        if n.endswith("_weight") and len(sh[n]) == 2:
            params.append(torch.randn(sh[n], generator=g) / sh[n][1] ** 0.5)
        elif n.startswith("norm") and n.endswith("weight"):
            params.append(1.0 + 0.3 * torch.randn(sh[n], generator=g))
        else:
            params.append(0.2 * torch.randn(sh[n], generator=g))
    dy = torch.randn(B, S, D, generator=g)
    masks = [None] * 4
    if variant in ("mask", "zero_attn", "zero_ff", "x10", "logit60"):
        masks = [(torch.rand(sh[n], generator=g) >= 0.3).float() / 0.7 for n in ("m_attn", "m1", "m_ff", "m2")]
    if variant == "zero_attn":
        masks[0] = torch.zeros(sh["m_attn"])
    if variant == "zero_ff":
        masks[2] = torch.zeros(sh["m_ff"])
    if variant == "x10":
        x = x * 10.0
    if variant == "logit60":
        # every query's logit against key 0 is 60 above the others: k_0 = c q-direction is not available per query, so
        # the in-projection is set up directly: q = 1 on every head column (bias), k_j = 0 except k_0 = 60 sqrt(d) / d
        d = D // H
        params[0] = params[0].clone()
        params[1] = params[1].clone()
        params[0][:2 * D] = 0.0
        params[1][:D] = 1.0
        params[1][D:2 * D] = 0.0
        x = x.clone()
        x[:, 0, 0] = 1.0
        x[:, 1:, 0] = 0.0
        params[0][D:2 * D, 0] = 60.0 * math.sqrt(d) / d          # k_0 = that constant on every column, k_j = 0
    ref = {}
    for dtype in (torch.float64, torch.float32):
        leaves = [x.to(dtype).clone().requires_grad_(True)] + [p.to(dtype).clone().requires_grad_(True) for p in params]
        mk = [None if m is None else m.to(dtype) for m in masks]
        y = TL.timelayer_torch(leaves[0], leaves[1:], H, mk)
        grads = torch.autograd.grad(y, leaves, dy.to(dtype))
        ref[dtype] = [t.detach().numpy() for t in (y,) + grads]
    inputs = dict(x=x, params=tuple(params), dy=dy, masks=tuple(masks))
    return inputs, {n: (a, b) for n, a, b in zip(NAMES, ref[torch.float64], ref[torch.float32])}


def _dev(inputs):
    mv = lambda t: None if t is None else t.to(DEV)                                   # noqa: E731
    return dict(x=mv(inputs["x"]), dy=mv(inputs["dy"]), params=tuple(mv(p) for p in inputs["params"]),
                masks=tuple(mv(m) for m in inputs["masks"]))


def _guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _run(inputs, H):
    """Forward + backward through vge.ops into guard-banded outputs -> {name: device tensor} (with the saved set)."""
    from vge import ops
    d = _dev(inputs)
    B, S, D = d["x"].shape
    sh = _shapes(B, S, D, H)
    bufs, out = {}, {}
    for k in NAMES + SAVED:
        bufs[k], out[k] = _guarded(sh[k[2:] if k.startswith("d_") else k])
    saved = tuple(out[k] for k in SAVED)
    ops.timelayer_forward(d["x"], d["params"], H, d["masks"], y=out["y"], saved=saved)
    ops.timelayer_backward(d["dy"], d["x"], d["params"], H, saved, d["masks"], out=tuple(out[k] for k in NAMES[1:]))
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()), f"guard band of {k}"
    return out


def _check(tag, out, ref):
    worst = {}
    for n in NAMES:
        f64, f32 = ref[n]
        got = out[n].detach().cpu().numpy()
        r = max(float(np.abs(f32.astype(np.float64) - f64).max()), _ulp32(np.abs(f64).max()))
        err = float(np.abs(got.astype(np.float64) - f64).max())
        worst[n] = err / r
        print(f"{tag} {n}: max|gpu-f64| {err:.3e} r {r:.3e} ratio {err / r:.4f}")
    for n in NAMES:
        assert np.isfinite(out[n].detach().cpu().numpy()).all(), (tag, n)
        assert worst[n] <= 8.0, (tag, n, worst[n])
    return worst


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "B%d_S%d_D%d_H%d" % s)
def test_layer_against_float64_autograd(shape, variant):
    """y and the 13 gradients within 8 r of float64 autograd of timelayer_torch; guard bands around every output and
    saved tensor intact; a second call gives the same bits."""
    inputs, ref = _case(shape, variant)
    out = _run(inputs, shape[3])
    _check("B%d_S%d_D%d_H%d %s" % (*shape, variant), out, ref)
    again = _run(inputs, shape[3])
    for k in out:
        assert _same_bits(out[k], again[k]), k


def test_one_token_has_no_query_or_key_gradient():
    """S = 1: the softmax is exactly 1, so dq and dk -- rows 0 .. 2D-1 of d in_proj_weight and d in_proj_bias -- are
    exactly 0."""
    inputs, _ = _case((1, 1, 32, 2), "mask")
    if float(inputs["masks"][0].min()) == 0.0:      # a dropped single weight would zero dv as well; keep it
        inputs = dict(inputs, masks=(torch.full_like(inputs["masks"][0], 1 / 0.7),) + inputs["masks"][1:])
    out = _run(inputs, 2)
    assert bool((out["d_in_proj_weight"][:64] == 0).all()) and bool((out["d_in_proj_bias"][:64] == 0).all())
    assert bool((out["d_in_proj_bias"][64:] != 0).any())


def test_zero_attention_mask_cuts_the_attention_off():
    """An all-zero m_attn: o = 0, so z = b_o bit for bit (u1 = x + b_o m1), d in_proj_weight and d in_proj_bias are
    exactly 0, and dx does not change when the in-projection changes."""
    shape = (2, 5, 64, 4)
    inputs, ref = _case(shape, "zero_attn")
    out = _run(inputs, 4)
    _check("zero_attn", out, ref)
    d = _dev(inputs)
    assert _same_bits(out["u1"], d["x"] + d["params"][3] * d["masks"][1])
    assert bool((out["d_in_proj_weight"] == 0).all()) and bool((out["d_in_proj_bias"] == 0).all())
    p = list(inputs["params"])
    p[0], p[1] = p[0] * 3.0 + 1.0, p[1] - 2.0
    assert _same_bits(_run(dict(inputs, params=tuple(p)), 4)["dx"], out["dx"])


def test_zero_feed_forward_mask_cuts_the_first_linear_off():
    """An all-zero m_ff: f = 0, so g = c2 bit for bit (u2 keeps its bits when linear2.weight is replaced by zeros, where
    g is c2 by construction), d linear1.weight and d linear1.bias are exactly 0, and dx does not change when linear1
    changes."""
    shape = (2, 5, 64, 4)
    inputs, ref = _case(shape, "zero_ff")
    out = _run(inputs, 4)
    _check("zero_ff", out, ref)
    assert bool((out["f"] == 0).all())
    zero_w2 = list(inputs["params"])
    zero_w2[6] = torch.zeros_like(zero_w2[6])
    assert _same_bits(_run(dict(inputs, params=tuple(zero_w2)), 4)["u2"], out["u2"])
    assert bool((out["d_linear1_weight"] == 0).all()) and bool((out["d_linear1_bias"] == 0).all())
    p = list(inputs["params"])
    p[4], p[5] = p[4] * 3.0 + 1.0, p[5] - 2.0
    assert _same_bits(_run(dict(inputs, params=tuple(p)), 4)["dx"], out["dx"])


@pytest.mark.parametrize("variant", ("x10", "logit60"))
def test_saturated_softmax_rows(variant):
    """x scaled by 10, and one key's logit 60 above the others in every row (p = 1 there, exp(-60) elsewhere):
    everything finite and within the bar."""
    shape = (3, 17, 96, 2)
    inputs, ref = _case(shape, variant)
    if variant == "logit60":
        from vge import timelayer as TL
        qkv = inputs["x"].double() @ inputs["params"][0].double().t() + inputs["params"][1].double()
        P = TL._attention(qkv, 2, None)[0]
        assert float(P[..., 0].min()) >= 1.0 - 1e-12 and float(P[..., 1:].max()) < 1e-25
    _check(variant, _run(inputs, shape[3]), ref)


def test_nan_stays_in_its_sample():
    from vge import ops
    inputs, _ = _case((3, 17, 96, 2), "mask")
    d = _dev(inputs)
    y, saved = ops.timelayer_forward(d["x"], d["params"], 2, d["masks"])
    grads = ops.timelayer_backward(d["dy"], d["x"], d["params"], 2, saved, d["masks"])
    xn = d["x"].clone()
    xn[1, 4, 7] = float("nan")
    yn, saved_n = ops.timelayer_forward(xn, d["params"], 2, d["masks"])
    grads_n = ops.timelayer_backward(d["dy"], xn, d["params"], 2, saved_n, d["masks"])
    torch.cuda.synchronize()
    assert bool(torch.isnan(yn[1]).all()) and bool(torch.isnan(grads_n[0][1]).all())
    for b in (0, 2):
        assert _same_bits(yn[b], y[b]) and _same_bits(grads_n[0][b], grads[0][b])
    # every parameter gradient but norm2.bias's, which is the column sum of dy alone
    assert all(bool(torch.isnan(g).any()) for g in grads_n[1:12]) and bool(torch.isfinite(grads_n[12]).all())


def test_refusals_launch_nothing():
    from vge import ops
    from vge.lib import UnsupportedModelError, VgeError

    def args(B, S, D, H, F_=None):
        sh = ops._timelayer_shapes(B, S, D, H, 4 * D if F_ is None else F_)
        return torch.zeros(B, S, D, device=DEV), tuple(torch.zeros(sh[n], device=DEV) for n in PARAMS)
    sentinel = torch.full((2, 8, 48), SENTINEL, device=DEV)
    with pytest.raises(UnsupportedModelError):
        x, p = args(2, 8, 48, 3)
        ops.timelayer_forward(x, p, 3, y=sentinel)
    for B, S, D, H, F_ in ((2, 66, 64, 4, None), (2, 8, 288, 8, None), (2, 8, 32, 4, None), (2, 8, 64, 4, 128)):
        with pytest.raises(UnsupportedModelError):
            x, p = args(B, S, D, H, F_)
            ops.timelayer_forward(x, p, H)
    x, p = args(2, 8, 64, 4)
    y64 = torch.full((2, 8, 64), SENTINEL, device=DEV)
    with pytest.raises(VgeError, match="workspace"):
        ops.timelayer_forward(x, p, 4, y=y64, workspace=torch.empty(1024, device=DEV))
    with pytest.raises(VgeError, match="alias"):
        ops.timelayer_forward(x, p, 4, y=x)
    _, saved = ops.timelayer_forward(x, p, 4)
    out = tuple(torch.full_like(t, SENTINEL) for t in (x,) + p)
    with pytest.raises(VgeError, match="workspace"):
        ops.timelayer_backward(x, x, p, 4, saved, out=out, workspace=torch.empty(1024, device=DEV))
    with pytest.raises(VgeError, match="alias"):
        ops.timelayer_backward(x, x, p, 4, saved, out=(x,) + out[1:])
    torch.cuda.synchronize()
    assert bool((sentinel == SENTINEL).all()) and bool((y64 == SENTINEL).all())
    assert all(bool((t == SENTINEL).all()) for t in out)


def test_autograd_function_under_a_non_unit_upstream_gradient(monkeypatch):
    """vge.timelayer.timelayer on device tensors: gradients of (y * dy).sum() * 0.37 against the float64 reference
    scaled the same way; under no_grad, and when nothing requires grad, the kernel is asked for no saved set; with only
    x requiring grad, dx is still within the bar."""
    from vge import timelayer as TL
    shape = (3, 17, 96, 2)
    inputs, ref = _case(shape, "mask")
    d = _dev(inputs)
    leaves = [d["x"].clone().requires_grad_(True)] + [p.clone().requires_grad_(True) for p in d["params"]]
    y = TL.timelayer(leaves[0], leaves[1:], 2, d["masks"])
    assert y.grad_fn is not None and len(y.grad_fn.saved_tensors) == 1 + 12 + 5 + 4
    ((y * d["dy"]).sum() * 0.37).backward()
    out = {"y": y.detach()}
    out.update({n: t.grad for n, t in zip(NAMES[1:], leaves)})
    scaled = {n: ((a, b) if n == "y" else (a * 0.37, b * np.float32(0.37))) for n, (a, b) in ref.items()}
    _check("function", out, scaled)
    calls = []
    real = TL.ops.timelayer_forward

    def spy(*a, save=True, **k):
        calls.append(save)
        return real(*a, save=save, **k)
    monkeypatch.setattr(TL.ops, "timelayer_forward", spy)
    with torch.no_grad():
        y2 = TL.timelayer(leaves[0], leaves[1:], 2, d["masks"])
    y3 = TL.timelayer(leaves[0].detach(), [t.detach() for t in leaves[1:]], 2, d["masks"])
    xg = d["x"].clone().requires_grad_(True)
    y4 = TL.timelayer(xg, d["params"], 2, d["masks"])
    assert calls == [False, False, True]
    assert y2.grad_fn is None and y3.grad_fn is None
    assert _same_bits(y2, y.detach()) and _same_bits(y3, y.detach())
    ((y4 * d["dy"]).sum() * 0.37).backward()
    f64, f32 = scaled["dx"]
    r = max(float(np.abs(f32.astype(np.float64) - f64).max()), _ulp32(np.abs(f64).max()))
    ratio = float(np.abs(xg.grad.cpu().numpy().astype(np.float64) - f64).max()) / r
    print(f"only x requires grad: dx ratio {ratio:.4f}")
    assert ratio <= 8.0


def test_forward_without_the_saved_set():
    """ops.timelayer_forward(save=False) -- the kernel's NULL saved set -- inside guard bands: y has the bits of the
    saving run."""
    from vge import ops
    for shape, variant in (((3, 17, 96, 2), "mask"), ((2, 33, 256, 8), "nomask")):
        inputs, _ = _case(shape, variant)
        d = _dev(inputs)
        want, saved = ops.timelayer_forward(d["x"], d["params"], shape[3], d["masks"])
        buf, y = _guarded(shape[:3])
        got, none = ops.timelayer_forward(d["x"], d["params"], shape[3], d["masks"], save=False, y=y)
        torch.cuda.synchronize()
        assert none is None and saved is not None and got.data_ptr() == y.data_ptr()
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
        assert _same_bits(got, want)


# ----------------------------------------------------------------------------- the module

def _module(conv_backend, time_backend):
    """train_ref.module with the backends set: the same checkpoint, modalities and hyper-parameters."""
    def build(layout, dropout=0.0):
        from tests.golden.dataset_spec import SMALL_HP, golden_state_dict
        from vge import synth
        from vge.model import HumanActionScorer
        sd = golden_state_dict(layout)
        mods = list(synth.DIMS_RAW)[:4 if layout == "nokp" else 5]
        hp = dict(SMALL_HP) if layout == "small" else {}
        m = HumanActionScorer({k: synth.DIMS_RAW[k] for k in mods}, {k: synth.DIMS_DIFF[k] for k in mods},
                              dropout=dropout, conv_backend=conv_backend, time_backend=time_backend, **hp)
        return m, sd
    return build


def test_four_steps_reproduce_the_reference_on_the_hip_layers(tgold, train_setup, monkeypatch):
    """Fixture (c)'s four recorded steps of the d_model 256 checkpoint with time_backend="hip" (conv blocks on torch),
    under the fixture's own factor (8).  Measured on an MI355X, largest |gpu - f64| / r: components 1.27, small tensors
    1.04, gradient norms 4.32 (motion_enc.pose.blocks.3.norm.bias)."""
    _, feats_of, labels = train_setup
    monkeypatch.setattr(TR, "module", _module("torch", "hip"))
    comps, grads, m = TR.run_steps(tgold, "kp", feats_of, labels, DEV, "hip")
    assert m.time_backend == "hip" and m.conv_backend == "torch"
    TR.check_steps(tgold, "kp", comps, grads, "gpu hip layers")


def test_four_steps_of_the_small_checkpoint_on_the_hip_layers(tgold, train_setup, monkeypatch):
    """The d_model 64 checkpoint (head dimension 16) under the fixture's factor 16.  Measured on an MI355X: components
    3.21, small tensors 1.54, gradient norms 13.8 (temporal.layers.0.norm2.bias)."""
    _, feats_of, labels = train_setup
    monkeypatch.setattr(TR, "module", _module("torch", "hip"))
    comps, grads, _ = TR.run_steps(tgold, "small", feats_of, labels, DEV, "hip")
    TR.check_steps(tgold, "small", comps, grads, "gpu hip layers")


@pytest.mark.parametrize("ckpt", ("kp", "small"))
def test_four_steps_with_both_backends_on_hip_stay_finite(ckpt, tgold, train_setup, monkeypatch):
    """conv_backend="hip" and time_backend="hip" together: the ratios are printed (DESIGN.md 5e records them) and every
    step's loss must be finite.  Measured on an MI355X: d_model 256 components 0.80, gradient norms 4.04; d_model 64
    components 2.75, gradient norms 10.6."""
    _, feats_of, labels = train_setup
    monkeypatch.setattr(TR, "module", _module("hip", "hip"))
    comps, grads, _ = TR.run_steps(tgold, ckpt, feats_of, labels, DEV, "hip")
    p = f"steps_{ckpt}_"
    names = [str(n) for n in tgold[p + "names"]]
    rk = np.abs(comps - tgold[p + "comp_f64"]) / tgold[p + "r_k"]
    norms = np.array([np.linalg.norm(grads[n].ravel()) for n in names])
    rn = np.abs(norms - tgold[p + "norm_f64"]) / tgold[p + "r_norm"]
    print(f"gpu hip blocks + hip layers {ckpt}: components {rk.max():.3f}, gradient norms {rn.max():.3f} "
          f"({names[int(rn.argmax())]}); factor of the fixture {int(tgold[p + 'factor'][0])}")
    assert np.isfinite(comps).all() and all(np.isfinite(g).all() for g in grads.values())


def _dropout_step_norms(time_backend, device, dtype, feats, table, labels, monkeypatch, attn_dropout):
    """Per-tensor gradient norms of one loss_components backward of the d_model 256 checkpoint in training mode with
    dropout 0.1 on replayed masks (conv blocks on torch)."""
    from vge import train as T
    from vge.losses import TCL, SupConWithHardNegatives
    m, sd = _module("torch", time_backend)("kp", dropout=0.1)
    TR.load(m, sd).to(device=device, dtype=dtype).train()
    if not attn_dropout:
        for layer in m.temporal.layers:
            layer.self_attn.dropout = 0.0
    f = feats.to(device=device, dtype=dtype)
    monkeypatch.setattr(torch.nn.functional, "dropout", _ReplayedDropout(4242))
    comps = T.loss_components(m, TCL(), SupConWithHardNegatives(), f, T.window_variants(f, table), labels.to(device))
    (comps[0] + comps[1] + comps[2] + comps[3]).backward()
    monkeypatch.undo()
    return {n: float(p.grad.double().norm()) for n, p in m.named_parameters()}


def test_hip_layers_under_replayed_dropout(tgold, train_setup, monkeypatch):
    """Dropout 0.1, replayed masks.  (a) attention dropout off everywhere (torch's cannot be replayed): the hip layers'
    worst per-tensor gradient-norm ratio against the float64 CPU run, r from the float32 CPU run of the same
    computation, is at most the larger of 8 and the torch layers' worst ratio measured here.  (b) attention dropout on:
    the hip layers on the device against the float64 CPU run of the "hip" module (the torch restatement, same masks):
    the ratio is printed, the gradients must be finite.  Measured on an MI355X: (a) torch layers 9.44 r, hip layers
    7.49 r; (b) 10.0 r (state_enc.global.blocks.1.conv1.weight)."""
    _, feats_of, labels = train_setup
    b = torch.from_numpy(tgold["steps_kp_batches"][0].astype(np.int64))
    feats = feats_of(b).cpu()
    table = torch.from_numpy(tgold["steps_kp_tables"][0].astype(np.int32))
    args = (feats, table, labels[b], monkeypatch)
    f64 = _dropout_step_norms("torch", "cpu", torch.float64, *args, False)
    f32 = _dropout_step_norms("torch", "cpu", torch.float32, *args, False)
    tor = _dropout_step_norms("torch", DEV, torch.float32, *args, False)
    hip = _dropout_step_norms("hip", DEV, torch.float32, *args, False)
    r = {n: max(abs(f32[n] - f64[n]), _ulp32(f64[n])) for n in f64}
    vs64 = {k: max(abs(v[n] - f64[n]) / r[n] for n in f64) for k, v in (("torch", tor), ("hip", hip))}
    print(f"(a) dropout 0.1 without attention dropout, against the float64 norms: torch layers {vs64['torch']:.3f} r, "
          f"hip layers {vs64['hip']:.3f} r")
    assert vs64["hip"] <= max(8.0, vs64["torch"])
    g64 = _dropout_step_norms("hip", "cpu", torch.float64, *args, True)
    g32 = _dropout_step_norms("hip", "cpu", torch.float32, *args, True)
    ghip = _dropout_step_norms("hip", DEV, torch.float32, *args, True)
    rb = {n: max(abs(g32[n] - g64[n]), _ulp32(g64[n])) for n in g64}
    ratio = {n: abs(ghip[n] - g64[n]) / rb[n] for n in g64}
    worst = max(ratio, key=ratio.get)
    print(f"(b) dropout 0.1 with attention dropout: hip layers {ratio[worst]:.3f} r ({worst})")
    assert all(math.isfinite(v) for v in ghip.values())


def test_hip_layer_draws_the_torch_layers_masks():
    """One seed, dropout 0.1, training mode, one layer on the device: all four multipliers of vge.timelayer.draw_masks
    are the masks torch's own layer draws on the math route -- the attention weights' too -- so the outputs differ by
    float32 rounding only (another mask would move them by O(1); measured 7.2e-7 with and without attention dropout).
    m1 coincides because it is drawn on the [S,B,D]-strided view torch's dropout1 sees; drawn on a contiguous [B,S,D]
    tensor it agrees with torch's on 0.83 of the entries and the outputs are 0.29 apart, which is pinned too."""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    from vge import timelayer as TL
    torch.manual_seed(1)
    layer = torch.nn.TransformerEncoderLayer(64, 4, 256, 0.1, batch_first=True).to(DEV).train()
    x = torch.randn(5, 33, 64, device=DEV)

    def both(attn_p, contiguous_m1=False):
        layer.self_attn.dropout = attn_p
        torch.manual_seed(7)
        with sdpa_kernel(SDPBackend.MATH):
            yt = layer(x).detach()
        torch.manual_seed(7)
        masks = TL.draw_masks(x, 4, 256, attn_p, 0.1, 0.1, 0.1)
        assert (masks[0] is None) == (attn_p == 0.0) and tuple(masks[1].shape) == (5, 33, 64)
        if contiguous_m1:
            torch.manual_seed(7)
            if attn_p > 0:
                torch.nn.functional.dropout(torch.ones(5, 4, 33, 33, device=DEV), attn_p, True)
            masks = (masks[0], torch.nn.functional.dropout(torch.ones(5, 33, 64, device=DEV), 0.1, True)) + masks[2:]
        return float((TL.timelayer(x, TL.layer_params(layer), 4, masks).detach() - yt).abs().max())
    off, on, other = both(0.0), both(0.1), both(0.1, contiguous_m1=True)
    print(f"dropout 0.1, one seed: max|y_hip - y_torch| without attention dropout {off:.3e}, with it {on:.3e}; with m1 "
          f"drawn on a contiguous tensor {other:.3e}")
    assert off <= 1e-4 and on <= 1e-4
    assert other > 1e-2


def test_train_one_epoch_on_the_hip_layers(golden_dataset, tmp_path):
    from vge import eval as E, train as T, validate as V
    paths, _ = golden_dataset
    (rec,) = T.train(paths["real"], paths["real_kp"], str(tmp_path / "run"), epochs=1, P=4, K=3,
                     eval_batch=R.FLOW_SMALL_BATCH, device=DEV, time_backend="hip")
    print({k: rec[k] for k in ("train_loss", "steps", "eval_loss", "conv_backend", "time_backend", "validated_by")})
    assert rec["time_backend"] == "hip" and rec["conv_backend"] == "torch"
    assert rec["steps"] > 0 and math.isfinite(rec["train_loss"]) and rec["checkpoint"] is not None
    dp = V.build_data_path(paths["real"], paths["real_kp"], device=DEV)
    assert isinstance(E.load_model(rec["checkpoint"], dp.dims_raw, dp.dims_diff, device=DEV), E.ops.Encoder)
    again = V.rank_checkpoints(paths["real"], paths["real_kp"], [rec["checkpoint"]], batch=R.FLOW_SMALL_BATCH,
                               device=DEV)[0]
    assert again["loss"] == rec["eval_loss"] and again["n_batches"] == rec["n_batches"]
