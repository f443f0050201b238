"""The conv block's forward and backward kernels (vge_convblock.hip) on the GPU, through vge.ops, vge.convblock and the
module with conv_backend="hip".

Reference and bar.  The reference is float64 autograd of vge.model._Block on the CPU.  Per tensor -- y and each of
dx, dw1, dw2, dgamma, dbeta -- max|gpu - f64| <= 8 r, r being the distance of the float32 CPU autograd from the float64
one on the same inputs, floored at one float32 ulp of the tensor's largest float64 magnitude (_check_grad
of tests/test_train_gpu.py).  Every test prints its ratios.

Measured on an MI355X, largest max|gpu - f64| / r per tensor (bar 8) over the eight shapes with and without a mask, the
all-zero mask, the all-zero sample, x scaled by 10 and the autograd function:
  y 1.09  dx 1.18  dw1 0.76  dw2 1.57  dgamma 2.23  dbeta 0.39
The module-level tests carry their own figures; all of them are in DESIGN.md 5e."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_ref as TR
from tests import validate_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = -12345.0
NAMES = ("y", "dx", "dw1", "dw2", "dgamma", "dbeta")

# (B, T, C, dilation): the smallest shapes at which the kernels can go wrong
CASES = [(1, 1, 32, 1),        # only the centre tap is inside; statistics over C alone
         (1, 5, 32, 8),        # T < dilation: every off-centre tap is padding
         (3, 9, 64, 8),        # taps +-8 land on exactly one row, +-16 never
         (2, 17, 96, 2),       # T one past an MFMA tile: fill rows stay out of the statistics and the weight gradients
         (2, 33, 96, 4),       # the same past two tiles; C not a power of two
         (5, 64, 256, 8),      # largest T and C
         (17, 32, 256, 1),     # batch not a multiple of a weight-gradient chunk
         (240, 32, 256, 4)]    # the training batch
VARIANTS = ("nomask", "mask")


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@functools.lru_cache(maxsize=None)
def _case(shape, variant):
    """Inputs (float32 numpy) and the CPU references of one case, computed once: {name: (f64, f32)}."""
    from vge.model import _Block
    B, T, Cn, dil = shape
    g = torch.Generator().manual_seed(7919 * B + 31 * T + Cn + dil)
    x = torch.randn(B, T, Cn, generator=g)
    w1, w2 = (torch.randn(Cn, Cn, 5, generator=g) / (5 * Cn) ** 0.5 for _ in range(2))
    gamma = 1.0 + 0.3 * torch.randn(Cn, generator=g)
    beta = 0.2 * torch.randn(Cn, generator=g)
    dy = torch.randn(B, T, Cn, generator=g)
    mask = None
    if variant in ("mask", "zero_sample", "x10"):
        mask = (torch.rand(B, T, Cn, generator=g) >= 0.3).float() / 0.7
    if variant == "zero_mask":
        mask = torch.zeros(B, T, Cn)
    if variant == "zero_sample":
        x[B - 1] = 0.0
    if variant == "x10":
        x = x * 10.0
    ref = {}
    for dtype in (torch.float64, torch.float32):
        blk = _Block(Cn, dil, 0.0).to(dtype)
        with torch.no_grad():
            for p, v in ((blk.conv1.weight, w1), (blk.conv2.weight, w2), (blk.norm.weight, gamma), (blk.norm.bias, beta)):
                p.copy_(v)
        xr = x.to(dtype).clone().requires_grad_(True)       # a copy: x itself stays a plain input
        h = F.gelu(blk.conv1(xr))
        if mask is not None:
            h = h * mask.to(dtype)
        y = blk.norm(F.gelu(blk.conv2(h) + xr))
        grads = torch.autograd.grad(y, (xr, blk.conv1.weight, blk.conv2.weight, blk.norm.weight, blk.norm.bias),
                                    dy.to(dtype))
        ref[dtype] = [t.detach().numpy() for t in (y,) + grads]
    inputs = dict(x=x, w1=w1, w2=w2, gamma=gamma, beta=beta, dy=dy, mask=mask)
    return inputs, {n: (a, b) for n, a, b in zip(NAMES, ref[torch.float64], ref[torch.float32])}


def _guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _run(inputs, dil):
    """Forward + backward through vge.ops into guard-banded outputs -> {name: device tensor} (with a, u, mean, rstd)."""
    from vge import ops
    d = {k: (None if v is None else v.to(DEV)) for k, v in inputs.items()}
    B, T, Cn = d["x"].shape
    shapes = {"y": (B, T, Cn), "a": (B, T, Cn), "u": (B, T, Cn), "mean": (B,), "rstd": (B,), "dx": (B, T, Cn),
              "dw1": (Cn, Cn, 5), "dw2": (Cn, Cn, 5), "dgamma": (Cn,), "dbeta": (Cn,)}
    bufs, out = {}, {}
    for k, s in shapes.items():
        bufs[k], out[k] = _guarded(s)
    saved = tuple(out[k] for k in ("a", "u", "mean", "rstd"))
    ops.convblock_forward(d["x"], d["w1"], d["w2"], d["gamma"], d["beta"], dil, d["mask"], y=out["y"], saved=saved)
    ops.convblock_backward(d["dy"], d["x"], d["w1"], d["w2"], d["gamma"], dil, saved, d["mask"],
                           out=tuple(out[k] for k in ("dx", "dw1", "dw2", "dgamma", "dbeta")))
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()), f"guard band of {k}"
    return out


def _check(tag, out, ref):
    worst = {}
    for n in NAMES:
        f64, f32 = ref[n]
        got = out[n].cpu().numpy()
        r = max(float(np.abs(f32.astype(np.float64) - f64).max()), _ulp32(np.abs(f64).max()))
        err = float(np.abs(got.astype(np.float64) - f64).max())
        worst[n] = err / r
        print(f"{tag} {n}: max|gpu-f64| {err:.3e} r {r:.3e} ratio {err / r:.4f}")
    for n in NAMES:
        assert np.isfinite(out[n].cpu().numpy()).all(), (tag, n)
        assert worst[n] <= 8.0, (tag, n, worst[n])
    return worst


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "B%d_T%d_C%d_d%d" % s)
def test_block_against_float64_autograd(shape, variant):
    """y and the five gradients within 8 r of float64 autograd of _Block; guard bands intact; a second call gives
    the same bits."""
    inputs, ref = _case(shape, variant)
    out = _run(inputs, shape[3])
    _check("B%d_T%d_C%d_d%d %s" % (*shape, variant), out, ref)
    again = _run(inputs, shape[3])
    for k in out:
        assert _same_bits(out[k], again[k]), k


def test_zero_mask_cuts_the_first_convolution_off():
    """An all-zero mask: h = 0, so u = x, da = 0, dw1 is exactly 0 and dx is du alone -- a function of x, dy and gamma
    only, so other weights leave its bits unchanged."""
    shape = (3, 9, 64, 8)
    inputs, ref = _case(shape, "zero_mask")
    out = _run(inputs, shape[3])
    _check("zero_mask", out, ref)
    assert bool((out["dw1"] == 0).all())
    assert bool((out["dw2"] == 0).all())           # h = 0
    assert _same_bits(out["u"], inputs["x"].to(DEV))
    other = dict(inputs, w1=inputs["w2"] * 3.0, w2=inputs["w1"] - 1.0)
    assert _same_bits(_run(other, shape[3])["dx"], out["dx"])
    # dx == du: with w1 = 0 the convolution of da contributes exact zeros whatever da is, and dx has the same bits
    assert _same_bits(_run(dict(inputs, w1=torch.zeros_like(inputs["w1"])), shape[3])["dx"], out["dx"])


def test_zero_sample():
    """One all-zero sample: its variance is 0, rstd = 1 / sqrt(eps), g^ = 0."""
    shape = (3, 9, 64, 8)
    inputs, ref = _case(shape, "zero_sample")
    out = _run(inputs, shape[3])
    _check("zero_sample", out, ref)
    assert float(out["mean"][2]) == 0.0 and abs(float(out["rstd"][2]) - 1e-5 ** -0.5) <= 1e-4 * 1e-5 ** -0.5
    assert _same_bits(out["y"][2], inputs["beta"].to(DEV).expand(9, 64).contiguous())


def test_inputs_in_the_tails_of_gelu():
    shape = (2, 17, 96, 2)
    inputs, ref = _case(shape, "x10")
    _check("x10", _run(inputs, shape[3]), ref)


def test_nan_stays_in_its_sample():
    from vge import ops
    shape = (3, 9, 64, 8)
    inputs, _ = _case(shape, "mask")
    d = {k: (None if v is None else v.to(DEV)) for k, v in inputs.items()}
    y, _ = ops.convblock_forward(d["x"], d["w1"], d["w2"], d["gamma"], d["beta"], 8, d["mask"])
    xn = d["x"].clone()
    xn[1, 4, 7] = float("nan")
    yn, saved = ops.convblock_forward(xn, d["w1"], d["w2"], d["gamma"], d["beta"], 8, d["mask"])
    grads = ops.convblock_backward(d["dy"], xn, d["w1"], d["w2"], d["gamma"], 8, saved, d["mask"])
    torch.cuda.synchronize()                        # the calls return
    assert bool(torch.isnan(yn[1]).any())
    assert _same_bits(yn[0], y[0]) and _same_bits(yn[2], y[2])
    assert bool(torch.isfinite(grads[0][0]).all()) and bool(torch.isfinite(grads[0][2]).all())


def test_refusals_launch_nothing():
    from vge import ops
    from vge.lib import UnsupportedModelError, VgeError

    def args(B, T, Cn):
        return (torch.zeros(B, T, Cn, device=DEV), torch.zeros(Cn, Cn, 5, device=DEV), torch.zeros(Cn, Cn, 5, device=DEV),
                torch.ones(Cn, device=DEV), torch.zeros(Cn, device=DEV))
    sentinel = torch.full((2, 8, 48), SENTINEL, device=DEV)
    with pytest.raises(UnsupportedModelError, match="C must be"):
        ops.convblock_forward(*args(2, 8, 48), 1, y=sentinel)
    with pytest.raises(UnsupportedModelError, match="T must be"):
        ops.convblock_forward(*args(2, 65, 64), 1)
    with pytest.raises(UnsupportedModelError, match="dilation"):
        ops.convblock_forward(*args(2, 8, 64), 3)
    with pytest.raises(VgeError, match="w1"):
        x, w1, w2, g, b = args(2, 8, 64)
        ops.convblock_forward(x, w1[:, :32], w2, g, b, 1)
    with pytest.raises(VgeError, match="alias"):
        x, w1, w2, g, b = args(2, 8, 64)
        ops.convblock_forward(x, w1, w2, g, b, 1, y=x)
    torch.cuda.synchronize()
    assert bool((sentinel == SENTINEL).all())


def test_autograd_function_under_a_non_unit_upstream_gradient(monkeypatch):
    """vge.convblock.convblock on device tensors: gradients of (y * dy).sum() * 0.37 against the float64 reference
    scaled the same way; under no_grad, and when nothing requires grad, the kernel is asked for no saved set."""
    from vge import convblock as CB
    shape = (2, 33, 96, 4)
    inputs, ref = _case(shape, "mask")
    d = {k: (None if v is None else v.to(DEV)) for k, v in inputs.items()}
    leaves = [d[k].clone().requires_grad_(True) for k in ("x", "w1", "w2", "gamma", "beta")]
    y = CB.convblock(*leaves, shape[3], d["mask"])
    assert y.grad_fn is not None and len(y.grad_fn.saved_tensors) == 9
    ((y * d["dy"]).sum() * 0.37).backward()
    out = {"y": y.detach()}
    out.update({n: t.grad for n, t in zip(NAMES[1:], leaves)})
    scaled = {n: ((a, b) if n == "y" else (a * 0.37, b * np.float32(0.37))) for n, (a, b) in ref.items()}
    _check("function", out, scaled)
    calls = []
    real = CB.ops.convblock_forward

    def spy(*a, save=True, **k):
        calls.append(save)
        return real(*a, save=save, **k)
    monkeypatch.setattr(CB.ops, "convblock_forward", spy)
    with torch.no_grad():                                   # leaves that require grad: still nothing is saved
        y2 = CB.convblock(*leaves, shape[3], d["mask"])
    y3 = CB.convblock(*[t.detach() for t in leaves], shape[3], d["mask"])      # grad mode on, nothing requires grad
    y4 = CB.convblock(*leaves, shape[3], d["mask"])
    assert calls == [False, False, True]
    assert y2.grad_fn is None and y3.grad_fn is None and len(y4.grad_fn.saved_tensors) == 9
    assert _same_bits(y2, y.detach()) and _same_bits(y3, y.detach())


def test_forward_without_the_saved_set():
    """ops.convblock_forward(save=False) -- the kernel's NULL saved set -- inside guard bands: y has the bits of the
    saving run, and the forward takes a workspace of vge_convblock_forward_workspace_bytes(C)."""
    from vge import ops
    for shape, variant in (((2, 33, 96, 4), "mask"), ((17, 32, 256, 1), "nomask")):
        inputs, _ = _case(shape, variant)
        d = {k: (None if v is None else v.to(DEV)) for k, v in inputs.items()}
        want, saved = ops.convblock_forward(d["x"], d["w1"], d["w2"], d["gamma"], d["beta"], shape[3], d["mask"])
        buf, y = _guarded(shape[:3])
        got, none = ops.convblock_forward(d["x"], d["w1"], d["w2"], d["gamma"], d["beta"], shape[3], d["mask"],
                                          save=False, y=y)
        torch.cuda.synchronize()
        assert none is None and saved is not None and got.data_ptr() == y.data_ptr()
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
        assert _same_bits(got, want)


# ----------------------------------------------------------------------------- the module

@pytest.fixture(scope="module")
def tgold():
    from tests.conftest import GOLDEN
    return dict(np.load(GOLDEN / "train_golden.npz"))


@pytest.fixture(scope="module")
def train_setup(golden_dataset):
    """The data path of vge.train on the golden real set (as in tests/test_train_gpu.py)."""
    from vge import eval as E, ops, validate as V
    from vge.data import sample_all_windows_npz
    paths, _ = golden_dataset
    dp = V.build_data_path(paths["real"], paths["real_kp"], device=DEV)
    samples = sample_all_windows_npz(dp.train_ds, 32, 8)
    windows = E._window_tensor(samples, {it.path: i for i, it in enumerate(dp.train_ds.items)}, DEV)
    labels = torch.as_tensor([dp.label_dict[it.cls] for it, _ in samples], dtype=torch.int64)

    def feats_of(b):
        return ops.featurize(dp.train_store, windows[b.to(DEV)], dp.stats.mean, dp.stats.std, layout=dp.stats.layout)
    return dp, feats_of, labels


def _module(conv_backend):
    """train_ref.module with the backend set: the same checkpoint, modalities and hyper-parameters."""
    def build(layout, dropout=0.0):
        from tests.golden.dataset_spec import SMALL_HP, golden_state_dict
        from vge import synth
        from vge.model import HumanActionScorer
        sd = golden_state_dict(layout)
        mods = list(synth.DIMS_RAW)[:4 if layout == "nokp" else 5]
        hp = dict(SMALL_HP) if layout == "small" else {}
        m = HumanActionScorer({k: synth.DIMS_RAW[k] for k in mods}, {k: synth.DIMS_DIFF[k] for k in mods},
                              dropout=dropout, conv_backend=conv_backend, **hp)
        return m, sd
    return build


def test_four_steps_reproduce_the_reference_on_the_hip_blocks(tgold, train_setup, monkeypatch):
    """Fixture (c)'s four recorded steps of the d_model 256 checkpoint with conv_backend="hip", under the fixture's own
    factor (8).  Measured on an MI355X, largest |gpu - f64| / r: components 2.94, small tensors 1.07, gradient norms
    5.56 (motion_enc.pose.blocks.3.norm.bias, whose r is one ulp of its norm)."""
    _, feats_of, labels = train_setup
    monkeypatch.setattr(TR, "module", _module("hip"))
    comps, grads, m = TR.run_steps(tgold, "kp", feats_of, labels, DEV, "hip")
    assert m.conv_backend == "hip"
    TR.check_steps(tgold, "kp", comps, grads, "gpu hip blocks")


def test_four_steps_of_the_small_checkpoint_stay_finite(tgold, train_setup, monkeypatch):
    """The d_model 64 checkpoint sits at 15.7 r of its bar of 16 on the torch blocks, on tensors whose r is at the
    one-ulp floor: here the same steps run, the ratios are printed (DESIGN.md 5e records them) and every step's loss
    must be finite.  Measured on an MI355X: components 1.42, gradient norms 11.7 (state_enc.global.blocks.3.norm.weight)."""
    _, feats_of, labels = train_setup
    monkeypatch.setattr(TR, "module", _module("hip"))
    comps, grads, _ = TR.run_steps(tgold, "small", feats_of, labels, DEV, "hip")
    p = "steps_small_"
    names = [str(n) for n in tgold[p + "names"]]
    rk = np.abs(comps - tgold[p + "comp_f64"]) / tgold[p + "r_k"]
    norms = np.array([np.linalg.norm(grads[n].ravel()) for n in names])
    rn = np.abs(norms - tgold[p + "norm_f64"]) / tgold[p + "r_norm"]
    print(f"gpu hip blocks small: components {rk.max():.3f}, gradient norms {rn.max():.3f} "
          f"({names[int(rn.argmax())]}); bar of the torch blocks {int(tgold[p + 'factor'][0])}")
    assert np.isfinite(comps).all()


def test_hip_block_draws_the_torch_blocks_mask():
    """One seed, dropout 0.1, training mode: the hip block's multiplier is the mask the torch block's nn.Dropout draws,
    so the two outputs differ by float32 rounding only (another mask would move them by O(1))."""
    from vge.model import _Block
    torch.manual_seed(1)
    bt, bh = _Block(64, 2, 0.1).to(DEV).train(), _Block(64, 2, 0.1, conv_backend="hip").to(DEV).train()
    bh.load_state_dict(bt.state_dict())
    x = torch.randn(5, 32, 64, device=DEV)
    ys = []
    for blk in (bt, bh):
        torch.manual_seed(7)
        ys.append(blk(x).detach())
    err = float((ys[0] - ys[1]).abs().max())
    print(f"dropout 0.1, one seed: max|y_hip - y_torch| {err:.3e} (max|y| {float(ys[0].abs().max()):.3f})")
    assert err <= 1e-4


class _ReplayedDropout:
    """F.dropout with masks from a seeded CPU generator: the same masks on the CPU and on the device, in float32 and in
    float64 (torch's own masks depend on the device and on the dtype), scaled by 1 / (1 - p) in the input's dtype."""

    def __init__(self, seed):
        self.gen = torch.Generator().manual_seed(seed)

    def __call__(self, input, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return input
        keep = torch.rand(input.shape, generator=self.gen) >= p
        return input * (keep.to(device=input.device, dtype=input.dtype) / (1.0 - p))


def _dropout_step_norms(backend, device, dtype, feats, table, labels, monkeypatch):
    """Per-tensor gradient norms of one loss_components backward of the d_model 256 checkpoint in training mode with
    dropout 0.1 on replayed masks.  The attention-weight dropout inside scaled_dot_product_attention cannot be
    replayed and is set to 0; every nn.Dropout and the blocks' multiplier are on."""
    from vge import train as T
    from vge.losses import TCL, SupConWithHardNegatives
    m, sd = _module(backend)("kp", dropout=0.1)
    TR.load(m, sd).to(device=device, dtype=dtype).train()
    for layer in m.temporal.layers:
        layer.self_attn.dropout = 0.0
    f = feats.to(device=device, dtype=dtype)
    monkeypatch.setattr(torch.nn.functional, "dropout", _ReplayedDropout(4242))
    comps = T.loss_components(m, TCL(), SupConWithHardNegatives(), f, T.window_variants(f, table), labels.to(device))
    (comps[0] + comps[1] + comps[2] + comps[3]).backward()
    monkeypatch.undo()
    return {n: float(p.grad.double().norm()) for n, p in m.named_parameters()}


def test_backends_agree_under_dropout(tgold, train_setup, monkeypatch):
    """Dropout 0.1, one seed, the same masks for everyone: the two backends' step-0 gradient norms on the device differ
    by at most 8 r, measured between each other.  r is, per tensor, the distance of the float32 CPU norm from the
    float64 CPU norm of this same computation (torch blocks, same batch, same masks), floored at one float32 ulp of
    the float64 norm.

    r comes from the computation that is compared, not from fixture (c), which was recorded without dropout: under
    dropout the hard-negative terms are out of saturation (3.3 each against 6.9) and every float32 route, the CPU's
    included, sits further from float64.
    Measured on an MI355X: largest ratio 4.63 (motion_enc.beta.blocks.3.conv1.weight); against the float64 norms the
    torch blocks are 9.44 r away at worst, the hip blocks 7.32 r.  (With every convolution output summed as one
    fmaf chain over its 5 C products the ratio was 228: the kernels sum in three short levels instead.)"""
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
    ratio = {n: abs(hip[n] - tor[n]) / r[n] for n in f64}
    vs64 = {k: max(abs(v[n] - f64[n]) / r[n] for n in f64) for k, v in (("torch", tor), ("hip", hip))}
    worst = max(ratio, key=ratio.get)
    print(f"dropout 0.1, replayed masks: largest |norm_hip - norm_torch| / r {ratio[worst]:.3f} ({worst}); against the "
          f"float64 norms: torch blocks {vs64['torch']:.3f} r, hip blocks {vs64['hip']:.3f} r")
    assert ratio[worst] <= 8.0


def test_train_one_epoch_on_the_hip_blocks(golden_dataset, tmp_path):
    from vge import eval as E, train as T, validate as V
    paths, _ = golden_dataset
    (rec,) = T.train(paths["real"], paths["real_kp"], str(tmp_path / "run"), epochs=1, P=4, K=3,
                     eval_batch=R.FLOW_SMALL_BATCH, device=DEV, conv_backend="hip")
    print({k: rec[k] for k in ("train_loss", "steps", "eval_loss", "conv_backend", "validated_by")})
    assert rec["conv_backend"] == "hip" and rec["steps"] > 0 and math.isfinite(rec["train_loss"])
    assert rec["checkpoint"] is not None
    dp = V.build_data_path(paths["real"], paths["real_kp"], device=DEV)
    assert isinstance(E.load_model(rec["checkpoint"], dp.dims_raw, dp.dims_diff, device=DEV), E.ops.Encoder)
