"""The bias-free linear node (vge_linear.hip) and the fusion node (vge_fusion.hip) on the GPU, through vge.ops,
vge.linear, vge.fusion and the module with linear_backend="hip" / fusion_backend="hip".

Reference and bar.  The reference is float64 autograd of the torch restatements (vge.linear.linear_torch,
vge.fusion.fusion_torch) on the CPU, on the same inputs and mask.  Per tensor max|gpu - f64| <= 8 r, r being the
distance of the float32 CPU autograd from the float64 one, floored at one float32 ulp of the tensor's largest float64
magnitude: the bar and the r of tests/test_timelayer_gpu.py.  Every test prints its ratios.

Measured on an MI355X, largest max|gpu - f64| / r per tensor (bar 8).  Fusion, over the six shapes with and without the
mask, the bias 60 above the others, the constant row and the autograd function:
  out 1.03  ds 1.04  latent 1.05  q_ln_weight 0.54  q_ln_bias 0.88  kv_ln_weight 2.16  kv_ln_bias 1.15
  Wq 0.73  Wk 1.00  Wv 0.64  Wo 0.82  logit_temp 0.82  logit_bias 0.57
Linear, over the six shapes and the autograd function:  y 0.85  dW 0.81  dx 0.77.
The module-level tests carry their own figures; all of them are in DESIGN.md 5e."""
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
FPARAMS = ("latent", "q_ln_weight", "q_ln_bias", "kv_ln_weight", "kv_ln_bias", "Wq", "Wk", "Wv", "Wo", "logit_temp",
           "logit_bias")
FNAMES = ("out", "ds") + tuple("d_" + n for n in FPARAMS)
FSAVED = ("stats", "a", "p", "vp")

# (R, M, D)
FUSION_CASES = [(1, 1, 32), (5, 4, 64), (33, 5, 96), (64, 5, 256),
                (561, 5, 256),      # the last chunk of the weight gradients and of the row sums holds one row
                (3, 8, 192)]
# (R, K, N, ldx, column, dx)
LINEAR_CASES = [(1, 3, 32, 3, 0, False), (5, 9, 64, 9, 0, True),
                (33, 207, 256, 2596, 1033, False),      # read in place, unaligned, K tail
                (70, 1024, 256, 2596, 0, False),        # aligned slice: vector loads
                (561, 120, 96, 120, 0, False), (65, 256, 256, 256, 0, True)]


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(bufs):
    for k, b in bufs.items():
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()), f"guard band of {k}"


def _check(tag, names, out, ref, finite=True):
    worst = {}
    for n in names:
        f64, f32 = ref[n]
        got = out[n].detach().cpu().numpy()
        r = max(float(np.abs(f32.astype(np.float64) - f64).max()), _ulp32(np.abs(f64).max()))
        err = float(np.abs(got.astype(np.float64) - f64).max())
        worst[n] = err / r
        print(f"{tag} {n}: max|gpu-f64| {err:.3e} r {r:.3e} ratio {err / r:.4f}")
    for n in names:
        assert np.isfinite(out[n].detach().cpu().numpy()).all(), (tag, n)
        assert worst[n] <= 8.0, (tag, n, worst[n])
    return worst


# ----------------------------------------------------------------------------- the fusion node

def _fshapes(R_, M, D):
    from vge import ops
    return ops._fusion_shapes(R_, M, D)


@functools.lru_cache(maxsize=None)
def _fcase(shape, variant):
    """Inputs (float32 torch, CPU) and the CPU references of one case, computed once: {name: (f64, f32)}."""
    from vge import fusion as FU
    R_, M, D = shape
    sh = _fshapes(R_, M, D)
    g = torch.Generator().manual_seed(7919 * R_ + 31 * M + D)
    s = torch.randn(R_, M, D, generator=g) * (1.0 + torch.rand(R_, M, 1, generator=g)) + 0.3
    params = []
    for n in FPARAMS:
        if n.startswith("W"):
            params.append(torch.randn(sh[n], generator=g) / D ** 0.5)
        elif n.endswith("ln_weight"):
            params.append(1.0 + 0.3 * torch.randn(sh[n], generator=g))
        elif n == "latent":
            params.append(torch.randn(sh[n], generator=g))
        else:
            params.append(0.2 * torch.randn(sh[n], generator=g))
    dy = torch.randn(R_, D, generator=g)
    m_attn = None
    if variant in ("mask", "bias60", "const"):
        m_attn = (torch.rand(R_, M, generator=g) >= 0.3).float() / 0.7
    if variant == "bias60":
        params[10] = params[10].clone()
        params[10][M // 2] += 60.0
    if variant == "const":
        s = s.clone()
        s[R_ // 2] = 1.75                          # every modality of one row: zero variance
    ref = {}
    for dtype in (torch.float64, torch.float32):
        leaves = [s.to(dtype).clone().requires_grad_(True)] + [p.to(dtype).clone().requires_grad_(True) for p in params]
        out = FU.fusion_torch(leaves[0], leaves[1:], None if m_attn is None else m_attn.to(dtype))
        grads = torch.autograd.grad(out, leaves, dy.to(dtype))
        ref[dtype] = [t.detach().numpy() for t in (out,) + grads]
    inputs = dict(s=s, params=tuple(params), dy=dy, m_attn=m_attn)
    return inputs, {n: (a, b) for n, a, b in zip(FNAMES, ref[torch.float64], ref[torch.float32])}


def _fdev(inputs):
    mv = lambda t: None if t is None else t.to(DEV)                                   # noqa: E731
    return dict(s=mv(inputs["s"]), dy=mv(inputs["dy"]), params=tuple(mv(p) for p in inputs["params"]),
                m_attn=mv(inputs["m_attn"]))


def _frun(inputs):
    """Forward + backward through vge.ops into guard-banded outputs -> {name: device tensor} (with the saved set)."""
    from vge import ops
    d = _fdev(inputs)
    sh = _fshapes(*d["s"].shape)
    bufs, out = {}, {}
    for k in FNAMES + FSAVED:
        bufs[k], out[k] = _guarded(sh[k[2:] if k.startswith("d_") else k])
    saved = tuple(out[k] for k in FSAVED)
    ops.fusion_forward(d["s"], d["params"], d["m_attn"], out=out["out"], saved=saved)
    ops.fusion_backward(d["dy"], d["s"], d["params"], saved, d["m_attn"], out=tuple(out[k] for k in FNAMES[1:]))
    torch.cuda.synchronize()
    _guards_intact(bufs)
    return out


@pytest.mark.parametrize("variant", ("nomask", "mask"))
@pytest.mark.parametrize("shape", FUSION_CASES, ids=lambda s: "R%d_M%d_D%d" % s)
def test_fusion_against_float64_autograd(shape, variant):
    """out and the 12 gradients within 8 r of float64 autograd of fusion_torch; guard bands around every output and
    saved tensor intact; a second call gives the same bits."""
    inputs, ref = _fcase(shape, variant)
    out = _frun(inputs)
    _check("fusion R%d_M%d_D%d %s" % (*shape, variant), FNAMES, out, ref)
    again = _frun(inputs)
    for k in out:
        assert _same_bits(out[k], again[k]), k


def test_one_modality_has_no_logit_gradient():
    """M = 1: the softmax is exactly 1, so the gradients of logit_temp, logit_bias, Wk, Wq, latent and q_ln are exactly
    0, as in the host test."""
    inputs, _ = _fcase((1, 1, 32), "nomask")
    out = _frun(inputs)
    for n in ("logit_temp", "logit_bias", "Wk", "Wq", "latent", "q_ln_weight", "q_ln_bias"):
        assert bool((out["d_" + n] == 0).all()), n
    assert bool((out["d_Wv"] != 0).any()) and bool((out["ds"] != 0).any())


def test_an_all_zero_mask_row_gives_a_zero_output_row():
    inputs, ref = _fcase((33, 5, 96), "mask")
    m = inputs["m_attn"].clone()
    m[7] = 0.0
    out = _frun(dict(inputs, m_attn=m))
    assert bool((out["out"][7].view(torch.int32) == 0).all()) and bool((out["p"][7] == 0).all())
    assert bool((out["out"][6] != 0).any())


@pytest.mark.parametrize("variant", ("bias60", "const"))
def test_saturated_and_constant_rows(variant):
    """One modality's logit_bias 60 above the others (a = 1 there, exp(-60) elsewhere), and a row of s that is constant
    (zero variance in the first LayerNorm): everything finite and within the bar."""
    inputs, ref = _fcase((33, 5, 96), variant)
    _check(variant, FNAMES, _frun(inputs), ref)


def test_nan_stays_in_its_row():
    from vge import ops
    inputs, _ = _fcase((33, 5, 96), "mask")
    d = _fdev(inputs)
    out, saved = ops.fusion_forward(d["s"], d["params"], d["m_attn"])
    grads = ops.fusion_backward(d["dy"], d["s"], d["params"], saved, d["m_attn"])
    sn = d["s"].clone()
    sn[11, 2, 5] = float("nan")
    out_n, saved_n = ops.fusion_forward(sn, d["params"], d["m_attn"])
    grads_n = ops.fusion_backward(d["dy"], sn, d["params"], saved_n, d["m_attn"])
    torch.cuda.synchronize()
    assert bool(torch.isnan(out_n[11]).all()) and bool(torch.isnan(grads_n[0][11]).all())
    keep = [r for r in range(33) if r != 11]
    assert _same_bits(out_n[keep], out[keep]) and _same_bits(grads_n[0][keep], grads[0][keep])


def test_fusion_forward_without_the_saved_set():
    from vge import ops
    inputs, _ = _fcase((64, 5, 256), "mask")
    d = _fdev(inputs)
    want, saved = ops.fusion_forward(d["s"], d["params"], d["m_attn"])
    buf, o = _guarded((64, 256))
    got, none = ops.fusion_forward(d["s"], d["params"], d["m_attn"], save=False, out=o)
    torch.cuda.synchronize()
    assert none is None and saved is not None and got.data_ptr() == o.data_ptr()
    _guards_intact({"out": buf})
    assert _same_bits(got, want)


def test_fusion_refusals_launch_nothing():
    from vge import ops
    from vge.lib import UnsupportedModelError, VgeError

    def args(R_, M, D):
        sh = _fshapes(R_, M, D)
        return torch.zeros(R_, M, D, device=DEV), tuple(torch.zeros(sh[n], device=DEV) for n in FPARAMS)
    sentinels = []
    for R_, M, D in ((4, 5, 48), (4, 5, 288), (4, 9, 64)):
        s, p = args(R_, M, D)
        sentinels.append(torch.full((R_, D), SENTINEL, device=DEV))
        with pytest.raises(UnsupportedModelError):
            ops.fusion_forward(s, p, out=sentinels[-1])
    s, p = args(4, 5, 64)
    o = torch.full((4, 64), SENTINEL, device=DEV)
    with pytest.raises(VgeError, match="workspace"):
        ops.fusion_forward(s, p, out=o, workspace=torch.empty(16, device=DEV))
    with pytest.raises(VgeError, match="alias"):
        ops.fusion_forward(s, p, out=s.view(-1)[:4 * 64].view(4, 64))
    _, saved = ops.fusion_forward(s, p)
    outs = (torch.full_like(s, SENTINEL),) + tuple(torch.full_like(t, SENTINEL) for t in p)
    dy = torch.zeros(4, 64, device=DEV)
    with pytest.raises(VgeError, match="workspace"):
        ops.fusion_backward(dy, s, p, saved, out=outs, workspace=torch.empty(16, device=DEV))
    with pytest.raises(VgeError, match="alias"):
        ops.fusion_backward(dy, s, p, saved, out=(s,) + outs[1:])
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all()) and all(bool((t == SENTINEL).all()) for t in tuple(sentinels) + outs)


def test_fusion_autograd_function(monkeypatch):
    """vge.fusion.fusion on device tensors under a 0.37 upstream gradient; under no_grad, and when nothing requires
    grad, the kernel is asked for no saved set; with only s requiring grad, ds is still within the bar."""
    from vge import fusion as FU
    inputs, ref = _fcase((33, 5, 96), "mask")
    d = _fdev(inputs)
    leaves = [d["s"].clone().requires_grad_(True)] + [p.clone().requires_grad_(True) for p in d["params"]]
    y = FU.fusion(leaves[0], leaves[1:], d["m_attn"])
    assert y.grad_fn is not None and len(y.grad_fn.saved_tensors) == 1 + 11 + 4 + 1
    ((y * d["dy"]).sum() * 0.37).backward()
    out = {"out": y.detach()}
    out.update({n: t.grad for n, t in zip(FNAMES[1:], leaves)})
    scaled = {n: ((a, b) if n == "out" else (a * 0.37, b * np.float32(0.37))) for n, (a, b) in ref.items()}
    _check("fusion function", FNAMES, out, scaled)
    calls = []
    real = FU.ops.fusion_forward

    def spy(*a, save=True, **k):
        calls.append(save)
        return real(*a, save=save, **k)
    monkeypatch.setattr(FU.ops, "fusion_forward", spy)
    with torch.no_grad():
        y2 = FU.fusion(leaves[0], leaves[1:], d["m_attn"])
    y3 = FU.fusion(leaves[0].detach(), [t.detach() for t in leaves[1:]], d["m_attn"])
    sg = d["s"].clone().requires_grad_(True)
    y4 = FU.fusion(sg, d["params"], d["m_attn"])
    assert calls == [False, False, True]
    assert y2.grad_fn is None and y3.grad_fn is None
    assert _same_bits(y2, y.detach()) and _same_bits(y3, y.detach())
    ((y4 * d["dy"]).sum() * 0.37).backward()
    _check("fusion, only s requires grad", ("ds",), {"ds": sg.grad}, scaled)


# ----------------------------------------------------------------------------- the linear node

@functools.lru_cache(maxsize=None)
def _lcase(case):
    from vge import linear as LN
    R_, K, N, ldx, col, _ = case
    g = torch.Generator().manual_seed(104729 * R_ + 7 * K + N)
    wide = torch.randn(R_, ldx, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    dy = torch.randn(R_, N, generator=g)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        x = wide[:, col:col + K].to(dtype).clone().requires_grad_(True)
        w = W.to(dtype).clone().requires_grad_(True)
        y = LN.linear_torch(x, w)
        ref[dtype] = [t.detach().numpy() for t in (y,) + torch.autograd.grad(y, (x, w), dy.to(dtype))]
    return dict(wide=wide, W=W, dy=dy), {n: (a, b) for n, a, b in zip(("y", "dx", "dW"), ref[torch.float64],
                                                                      ref[torch.float32])}


def _lrun(case, inputs):
    from vge import ops
    R_, K, N, ldx, col, need_dx = case
    wide, W, dy = (inputs[k].to(DEV) for k in ("wide", "W", "dy"))
    x = wide[:, col:col + K]
    assert x.data_ptr() == wide.data_ptr() + 4 * col
    names = ("y", "dW") + (("dx",) if need_dx else ())
    bufs, out = {}, {}
    for k, shape in (("y", (R_, N)), ("dW", (N, K)), ("dx", (R_, K))):
        if k in names:
            bufs[k], out[k] = _guarded(shape)
    ops.linear_forward(x, W, y=out["y"])
    ops.linear_backward(dy, x, W, need_dx, out=(out.get("dx"), out["dW"]))
    torch.cuda.synchronize()
    _guards_intact(bufs)
    return names, out


@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: "R%d_K%d_N%d_ld%d_c%d_dx%d" % c)
def test_linear_against_float64_autograd(case):
    """y, dW (and dx where asked for) within 8 r of float64 autograd; x read in place from the wider tensor; guard
    bands intact; a second call gives the same bits."""
    inputs, ref = _lcase(case)
    names, out = _lrun(case, inputs)
    _check("linear R%d_K%d_N%d_ld%d_c%d_dx%d" % case, names, out, ref)
    _, again = _lrun(case, inputs)
    for k in out:
        assert _same_bits(out[k], again[k]), k


def test_linear_refusals_launch_nothing():
    from vge import lib as L, ops
    from vge.lib import UnsupportedModelError, VgeError
    so = L.load()
    y = torch.full((4, 64), SENTINEL, device=DEV)
    W = torch.zeros(64, 8, device=DEV)
    x = torch.zeros(4, 8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert so.vge_linear_forward(x.data_ptr(), 8, W.data_ptr(), y.data_ptr(), 4, 0, 64, stream) == 7      # K = 0
    assert so.vge_linear_forward(x.data_ptr(), 4097, W.data_ptr(), y.data_ptr(), 4, 4097, 64, stream) == 7
    assert so.vge_linear_forward(x.data_ptr(), 4, W.data_ptr(), y.data_ptr(), 4, 8, 64, stream) == 1      # ldx < K
    with pytest.raises(UnsupportedModelError):
        ops.linear_forward(x, torch.zeros(48, 8, device=DEV), y=torch.full((4, 48), SENTINEL, device=DEV))
    dW, dx = torch.full_like(W, SENTINEL), torch.full_like(x, SENTINEL)
    dy = torch.zeros(4, 64, device=DEV)
    with pytest.raises(VgeError, match="workspace"):
        ops.linear_backward(dy, x, W, out=(dx, dW), workspace=torch.empty(16, device=DEV))
    with pytest.raises(VgeError, match="alias"):
        ops.linear_backward(dy, x, W, out=(dx, W))
    with pytest.raises(VgeError, match="alias"):
        ops.linear_forward(W.view(-1)[:4 * 64].view(4, 64)[:, :8], W, y=W.view(-1)[:4 * 64].view(4, 64))
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((dW == SENTINEL).all()) and bool((dx == SENTINEL).all())


def test_linear_autograd_function():
    """vge.linear.linear on a [B,T,K] column slice of a [B,T,2596] tensor under a 0.37 upstream gradient; under no_grad
    nothing is saved; dx only where x requires grad."""
    from vge import linear as LN
    case = (33, 207, 256, 2596, 1033, False)
    inputs, ref = _lcase(case)
    wide = inputs["wide"].to(DEV).view(3, 11, 2596)
    x = wide[..., 1033:1033 + 207]
    W = inputs["W"].to(DEV).requires_grad_(True)
    dy = inputs["dy"].to(DEV).view(3, 11, 256)
    assert LN.kernels_take(x, W) and LN._rows(x).data_ptr() == x.data_ptr()
    y = LN.linear(x, W)
    ((y * dy).sum() * 0.37).backward()
    scaled = {n: ((a, b) if n == "y" else (a * 0.37, b * np.float32(0.37))) for n, (a, b) in ref.items()}
    _check("linear function", ("y", "dW"), {"y": y.detach().view(33, 256), "dW": W.grad}, scaled)
    with torch.no_grad():
        y2 = LN.linear(x, W)
    assert y2.grad_fn is None and _same_bits(y2, y.detach())
    xg = x.detach().clone().requires_grad_(True)                  # contiguous [3,11,207]
    y3 = LN.linear(xg, W.detach())
    ((y3 * dy).sum() * 0.37).backward()
    _check("linear, only x requires grad", ("dx",), {"dx": xg.grad.view(33, 207)}, scaled)


# ----------------------------------------------------------------------------- the module

def _module(conv_backend, time_backend, linear_backend="hip", fusion_backend="hip"):
    """train_ref.module with the backends set: the same checkpoint, modalities and hyper-parameters."""
    def build(layout, dropout=0.0):
        from tests.golden.dataset_spec import SMALL_HP, golden_state_dict
        from vge import synth
        from vge.model import HumanActionScorer
        sd = golden_state_dict(layout)
        mods = list(synth.DIMS_RAW)[:4 if layout == "nokp" else 5]
        hp = dict(SMALL_HP) if layout == "small" else {}
        m = HumanActionScorer({k: synth.DIMS_RAW[k] for k in mods}, {k: synth.DIMS_DIFF[k] for k in mods},
                              dropout=dropout, conv_backend=conv_backend, time_backend=time_backend,
                              linear_backend=linear_backend, fusion_backend=fusion_backend, **hp)
        return m, sd
    return build


def test_four_steps_reproduce_the_reference_on_the_hip_linear_and_fusion(tgold, train_setup, monkeypatch):
    """Fixture (c)'s four recorded steps of the d_model 256 checkpoint with linear_backend="hip" and
    fusion_backend="hip" (conv blocks and temporal layers on torch), under the fixture's own factor (8).  Measured on
    an MI355X, largest |gpu - f64| / r: components 1.38, small tensors 0.96, gradient norms 2.53
    (temporal.layers.1.norm2.bias)."""
    _, feats_of, labels = train_setup
    monkeypatch.setattr(TR, "module", _module("torch", "torch"))
    comps, grads, m = TR.run_steps(tgold, "kp", feats_of, labels, DEV, "hip")
    assert (m.linear_backend, m.fusion_backend, m.conv_backend, m.time_backend) == ("hip", "hip", "torch", "torch")
    TR.check_steps(tgold, "kp", comps, grads, "gpu hip linear + fusion")


def test_four_steps_of_the_small_checkpoint_on_the_hip_linear_and_fusion(tgold, train_setup, monkeypatch):
    """The d_model 64 checkpoint under the fixture's factor 16.  Measured on an MI355X: components 13.1 (the fourth
    step; 2.1 at most before it), small tensors 1.28, gradient norms 12.1 (temporal.layers.0.norm2.bias)."""
    _, feats_of, labels = train_setup
    monkeypatch.setattr(TR, "module", _module("torch", "torch"))
    comps, grads, _ = TR.run_steps(tgold, "small", feats_of, labels, DEV, "hip")
    TR.check_steps(tgold, "small", comps, grads, "gpu hip linear + fusion")


def test_one_step_without_keypoints_stays_finite(golden_dataset_nokp, tgold):
    """The four-modality layout (M = 4): one loss_components backward from the golden checkpoint on the device against
    the float64 CPU run of the default module; the ratios are printed, losses and gradients must be finite.  Measured on
    an MI355X: components 0.53 r, gradient norms 2.83 r (state_enc.beta.blocks.0.norm.bias)."""
    from vge import eval as E, ops, train as T, validate as V
    from vge.data import sample_all_windows_npz
    from vge.losses import TCL, SupConWithHardNegatives
    paths, _ = golden_dataset_nokp
    dp = V.build_data_path(paths["real"], None, device=DEV)
    samples = sample_all_windows_npz(dp.train_ds, 32, 8)
    windows = E._window_tensor(samples, {it.path: i for i, it in enumerate(dp.train_ds.items)}, DEV)
    labels = torch.as_tensor([dp.label_dict[it.cls] for it, _ in samples], dtype=torch.int64)
    b = torch.from_numpy(tgold["steps_kp_batches"][0].astype(np.int64)) % len(samples)
    feats = ops.featurize(dp.train_store, windows[b.to(DEV)], dp.stats.mean, dp.stats.std, layout=dp.stats.layout)
    table = torch.from_numpy(tgold["steps_kp_tables"][0].astype(np.int32))
    runs = {}
    for tag, build, device, dtype in (("f64", TR.module, "cpu", torch.float64), ("f32", TR.module, "cpu", torch.float32),
                                      ("hip", _module("torch", "torch"), DEV, torch.float32)):
        m, sd = build("nokp")
        TR.load(m, sd).to(device=device, dtype=dtype).train()
        f = feats.to(device=device, dtype=dtype)
        comps = T.loss_components(m, TCL(), SupConWithHardNegatives(), f, T.window_variants(f, table),
                                  labels[b].to(device))
        sum(comps).backward()
        runs[tag] = ([float(c.detach()) for c in comps], {n: float(p.grad.double().norm()) for n, p in m.named_parameters()})
    assert len(m.modalities) == 4 and m.fusion_backend == "hip"
    rc = max(abs(h - a) / max(abs(c - a), _ulp32(a)) for a, c, h in zip(runs["f64"][0], runs["f32"][0], runs["hip"][0]))
    ratio = {n: abs(runs["hip"][1][n] - v) / max(abs(runs["f32"][1][n] - v), _ulp32(v)) for n, v in runs["f64"][1].items()}
    worst = max(ratio, key=ratio.get)
    print(f"nokp (M = 4) one step: components {rc:.3f} r, gradient norms {ratio[worst]:.3f} r ({worst})")
    assert all(math.isfinite(v) for v in runs["hip"][0]) and all(math.isfinite(v) for v in runs["hip"][1].values())


@pytest.mark.parametrize("ckpt", ("kp", "small"))
def test_four_steps_with_all_four_backends_on_hip(ckpt, tgold, train_setup, monkeypatch):
    """All four backends on "hip": the ratios are printed (DESIGN.md 5e records them), every loss and gradient must be
    finite, and the four steps run twice give the same losses and step-0 gradients bit for bit.  Measured on an MI355X:
    d_model 256 components 1.80, gradient norms 5.68 (temporal.layers.1.norm1.bias); d_model 64 components 1.99,
    gradient norms 7.16 (temporal.layers.0.norm2.bias); the two runs agree in every bit."""
    _, feats_of, labels = train_setup
    monkeypatch.setattr(TR, "module", _module("hip", "hip"))
    comps, grads, _ = TR.run_steps(tgold, ckpt, feats_of, labels, DEV, "hip")
    comps2, grads2, _ = TR.run_steps(tgold, ckpt, feats_of, labels, DEV, "hip")
    p = f"steps_{ckpt}_"
    names = [str(n) for n in tgold[p + "names"]]
    rk = np.abs(comps - tgold[p + "comp_f64"]) / tgold[p + "r_k"]
    norms = np.array([np.linalg.norm(grads[n].ravel()) for n in names])
    rn = np.abs(norms - tgold[p + "norm_f64"]) / tgold[p + "r_norm"]
    differ = [n for n in names if not np.array_equal(grads[n], grads2[n])]
    print(f"gpu all four backends on hip {ckpt}: components {rk.max():.3f}, gradient norms {rn.max():.3f} "
          f"({names[int(rn.argmax())]}); factor of the fixture {int(tgold[p + 'factor'][0])}; two runs: losses "
          f"{'equal' if np.array_equal(comps, comps2) else 'differ'}, step-0 gradients differing in bits: {differ[:6]}")
    assert np.isfinite(comps).all() and all(np.isfinite(g).all() for g in grads.values())
    assert np.array_equal(comps, comps2) and not differ


def _dropout_step_norms(backend, device, dtype, feats, table, labels, monkeypatch):
    """Per-tensor gradient norms of one loss_components backward of the d_model 256 checkpoint in training mode with
    dropout 0.1 on replayed masks (conv blocks and temporal layers on torch, attention dropout of the temporal stack
    off: torch's cannot be replayed)."""
    from vge import train as T
    from vge.losses import TCL, SupConWithHardNegatives
    m, sd = _module("torch", "torch", backend, backend)("kp", dropout=0.1)
    TR.load(m, sd).to(device=device, dtype=dtype).train()
    for layer in m.temporal.layers:
        layer.self_attn.dropout = 0.0
    f = feats.to(device=device, dtype=dtype)
    monkeypatch.setattr(torch.nn.functional, "dropout", _ReplayedDropout(4242))
    comps = T.loss_components(m, TCL(), SupConWithHardNegatives(), f, T.window_variants(f, table), labels.to(device))
    (comps[0] + comps[1] + comps[2] + comps[3]).backward()
    monkeypatch.undo()
    return {n: float(p.grad.double().norm()) for n, p in m.named_parameters()}


def test_hip_linear_and_fusion_under_replayed_dropout(tgold, train_setup, monkeypatch):
    """Dropout 0.1, replayed masks: the new backends' worst per-tensor gradient-norm ratio against the float64 CPU run
    (r from the float32 CPU run of the same computation) is at most the larger of 8 and the torch backends' worst
    ratio measured here.  Measured on an MI355X: torch backends 9.44 r (fusion.logit_temp), hip linear + fusion 5.64 r
    (state_enc.pose.blocks.0.norm.weight)."""
    _, feats_of, labels = train_setup
    b = torch.from_numpy(tgold["steps_kp_batches"][0].astype(np.int64))
    feats = feats_of(b).cpu()
    table = torch.from_numpy(tgold["steps_kp_tables"][0].astype(np.int32))
    args = (feats, table, labels[b], monkeypatch)
    f64 = _dropout_step_norms("torch", "cpu", torch.float64, *args)
    f32 = _dropout_step_norms("torch", "cpu", torch.float32, *args)
    tor = _dropout_step_norms("torch", DEV, torch.float32, *args)
    hip = _dropout_step_norms("hip", DEV, torch.float32, *args)
    r = {n: max(abs(f32[n] - f64[n]), _ulp32(f64[n])) for n in f64}
    vs64 = {k: max((abs(v[n] - f64[n]) / r[n], n) for n in f64) for k, v in (("torch", tor), ("hip", hip))}
    print(f"dropout 0.1 on replayed masks, against the float64 norms: torch backends {vs64['torch'][0]:.3f} r "
          f"({vs64['torch'][1]}), hip linear + fusion {vs64['hip'][0]:.3f} r ({vs64['hip'][1]})")
    assert vs64["hip"][0] <= max(8.0, vs64["torch"][0])


def test_the_fusion_multiplier_is_torchs_mask():
    """One seed, dropout 0.1, training mode, the fusion alone on the device: m_attn is drawn as
    F.dropout(ones(B,T,M)) where _Fusion.dropout draws on the attention weights [B,T,M], a contiguous tensor of the
    same shape, so the multiplier IS torch's mask and the outputs differ by float32 rounding only (another mask would
    move them by O(0.1); measured on an MI355X 3.0e-7 at max|out| 0.80)."""
    from vge import fusion as FU
    from vge.model import _Fusion
    torch.manual_seed(1)
    mod = _Fusion(64, 5, 0.1).to(DEV).train()
    s = torch.randn(6, 32, 5, 64, device=DEV)
    torch.manual_seed(7)
    want = mod(torch.nn.functional.layer_norm(s, (64,))).detach()
    torch.manual_seed(7)
    m_attn = torch.nn.functional.dropout(torch.ones(6, 32, 5, device=DEV), 0.1, True)
    got = FU.fusion(s, FU.fusion_params(mod), m_attn).detach()
    err = float((got - want).abs().max())
    print(f"fusion dropout 0.1, one seed: max|out_hip - out_torch| {err:.3e} (max|out| {float(want.abs().max()):.3f})")
    assert err <= 1e-4


def test_train_one_epoch_on_the_hip_linear_and_fusion(golden_dataset, tmp_path):
    from vge import eval as E, train as T, validate as V
    paths, _ = golden_dataset
    (rec,) = T.train(paths["real"], paths["real_kp"], str(tmp_path / "run"), epochs=1, P=4, K=3,
                     eval_batch=R.FLOW_SMALL_BATCH, device=DEV, linear_backend="hip", fusion_backend="hip")
    print({k: rec[k] for k in ("train_loss", "steps", "eval_loss", "linear_backend", "fusion_backend", "validated_by")})
    assert rec["linear_backend"] == "hip" and rec["fusion_backend"] == "hip"
    assert rec["conv_backend"] == "torch" and rec["time_backend"] == "torch"
    assert rec["steps"] > 0 and math.isfinite(rec["train_loss"]) and rec["checkpoint"] is not None
    dp = V.build_data_path(paths["real"], paths["real_kp"], device=DEV)
    assert isinstance(E.load_model(rec["checkpoint"], dp.dims_raw, dp.dims_diff, device=DEV), E.ops.Encoder)
    again = V.rank_checkpoints(paths["real"], paths["real_kp"], [rec["checkpoint"]], batch=R.FLOW_SMALL_BATCH,
                               device=DEV)[0]
    assert again["loss"] == rec["eval_loss"] and again["n_batches"] == rec["n_batches"]
