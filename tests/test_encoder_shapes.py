"""The encoder and the reductions behind it at every checkpoint shape vge_encoder_create accepts.

load_model builds the encoder from the checkpoint's own d_model / time_layers / time_heads (eval.py:136-152), so a
2- or 9-layer checkpoint, or one of another width, is an ordinary input.  The reference of every GPU case here is the
oracle (oracle/encoder.py) run in float64 on the same float32 weights and input; the oracle itself is pinned to the
reference's HumanActionScorer at every shape by tests/golden/golden_shapes.npz (make_golden.py shapes).

  CPU  the float32 and the float64 oracle within 1e-5 of every golden_shapes.npz entry
  GPU  tiled kernels (d_model 256, 8 heads): time_layers 1, 2, 3, 5, 8 in f32x3 (fused transformer_x3_kernel),
       f32x3 with VGE_X3_UNFUSED=1 (per-layer gemm_x3 / attn / ffn_x3 kernels), f32 and f16; 4 layers per-layer;
       two windows per workgroup; the fp16 two-workgroups-per-CU variant; 9 and 12 layers (f32x3 falls back to the
       per-layer kernels, f16 refuses); 4 modalities
       generic exact-f32 kernels (vge_encoder_gen.hip): d_model 32..256, head dims 8..64, 4 modalities, null outputs,
       and the shapes it must refuse
       tc_windows / centroid_accumulate / centroid_finalize / score_videos at d 32, 96, 160, 224, 256

Tolerances.  f32-class modes (f32x3 fused and per-layer, f32, generic): the project's bar (embeddings 2e-5, window TC
1e-5) and a tight one calibrated in the test: e_ref = max |oracle_f32 - oracle_f64| on the same input, GPU error
against the float64 oracle <= max(20 e_ref, 2e-6) (20x: another, equally valid f32 summation order; several times
below the fp16 mode's error, which the 2e-5 bar cannot tell from the 3xfp16 split).  f16 is not a parity mode:
embeddings 2e-4 up to 4 layers (the existing bar), F16_BAR beyond; its window TC bar is half its embedding bar, the
ratio of the existing 4-layer bars (1e-4 : 2e-4, tests/test_bench_parity.py).

Measured on an MI355X (max over the cases of a mode; seq / frame / TC error against the float64 oracle; e_ref was
5.6e-8 to 2.1e-7, the tight bar 2e-6 to 4.2e-6):
  f32x3 fused      1.4e-7 / 1.7e-7 / 5.9e-8   (worst error / tight bar 0.07)
  f32x3 per-layer  1.3e-7 / 1.9e-7 / 1.1e-7   (0.06)
  f32 tiled        1.3e-7 / 2.7e-7 / 1.2e-7   (0.08)
  f32 generic      9.7e-8 / 3.1e-7 / 1.5e-7   (0.11)
  f16 1, 2, 3 layers   seq 2.0e-6, 3.9e-6, 4.9e-6; frames 6.5e-5, 7.2e-5, 8.0e-5; TC up to 1.7e-5
  f16 5 layers     6.1e-6 / 8.4e-5 / 6.5e-6   -> bar 2e-4 (2 x 8.4e-5 = 1.7e-4, rounded up to one digit)
  f16 8 layers     7.9e-6 / 8.6e-5 / 7.0e-6   -> bar 2e-4 (2 x 8.6e-5 = 1.7e-4, rounded up to one digit)
  tc_windows 2.7e-7; class sums 3.6e-6, centroids 1.2e-7
"""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.golden.dataset_spec import (GENERIC_SHAPES, TILED_SHAPES, shape_dims, shape_key, shape_state_dict,
                                       shape_windows)

gpu = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN_SHAPES = "golden_shapes.npz"

# f16 embedding bars beyond 4 layers: 2x the error measured on the first MI355X run (8.4e-5 at 5 layers, 8.6e-5 at 8;
# the module docstring), rounded up to one digit, and no more than 4e-4 (linear in depth from the 4-layer bar 2e-4)
F16_BAR = {5: 2e-4, 8: 2e-4}


def _oracle(shape, dtype):
    from oracle.encoder import OracleEncoder
    d, heads, layers, n_mod = shape
    raw, diff = shape_dims(n_mod)
    return OracleEncoder(_sd(shape), raw, diff, d_model=d, time_layers=layers, time_heads=heads, dtype=dtype)


def _sd(shape):
    if shape not in _sd.cache:
        _sd.cache[shape] = shape_state_dict(shape, max_len=40)
    return _sd.cache[shape]


_sd.cache = {}


# ------------------------------------------------------------------------------------------------------ CPU

@pytest.fixture(scope="module")
def golden_shapes():
    return dict(np.load(Path(__file__).resolve().parent / "golden" / GOLDEN_SHAPES))


def test_golden_shapes_fixture_holds_every_shape(golden_shapes):
    keys = {shape_key(s) + suffix for s in TILED_SHAPES + GENERIC_SHAPES for suffix in ("_seq", "_frames")}
    assert set(golden_shapes) == keys
    for s in TILED_SHAPES + GENERIC_SHAPES:
        assert golden_shapes[shape_key(s) + "_seq"].shape == (3, s[0])
        assert golden_shapes[shape_key(s) + "_frames"].shape == (33, s[0])
        assert golden_shapes[shape_key(s) + "_seq"].dtype == np.float32


@pytest.mark.parametrize("shape", TILED_SHAPES + GENERIC_SHAPES, ids=shape_key)
def test_oracle_matches_reference_at_shape(shape, golden_shapes):
    """The oracle, in float32 and in float64, within 1e-5 of HumanActionScorer's own output at this shape (the bar of
    test_oracle_small_embeddings)."""
    x = shape_windows(shape[3])
    ref_seq, ref_fr = golden_shapes[shape_key(shape) + "_seq"], golden_shapes[shape_key(shape) + "_frames"]
    for dtype in (torch.float32, torch.float64):
        seq, fr, _ = _oracle(shape, dtype).forward(x)
        assert seq.dtype == dtype
        e_seq = np.abs(seq.double().numpy() - ref_seq).max()
        e_fr = np.abs(fr[0].double().numpy() - ref_fr).max()
        print(f"{shape_key(shape)} {dtype}: seq {e_seq:.2e} frames {e_fr:.2e}")
        assert e_seq < 1e-5 and e_fr < 1e-5, (dtype, e_seq, e_fr)


# ------------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def vg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vge import lib as L
    from vge import ops
    return L, ops


def _tc_ref(frames):
    f = frames[:, 1:]
    return (f[:, 1:] - f[:, :-1]).pow(2).sum(-1).sqrt().mean(-1)


def _reference(shape, n_max):
    """Random z-scored windows [n_max, 32, feat_dim] (fixed seed) and the float64 oracle on them: computed once per
    (shape, n_max), sliced by the cases, never modified (the float32 oracle run joins it when an f32-class case first
    asks for e_ref)."""
    key = (shape, n_max)
    if key not in _reference.cache:
        raw, diff = shape_dims(shape[3])
        torch.manual_seed(1000 + n_max)
        x = torch.randn(n_max, 32, sum(raw.values()) + sum(diff.values()))
        s64, f64, _ = _oracle(shape, torch.float64).forward(x)
        _reference.cache[key] = dict(shape=shape, x=x, seq=s64, frames=f64, tc=_tc_ref(f64))
    return _reference.cache[key]


_reference.cache = {}


def _e_ref(ref, n):
    """max |oracle_f32 - oracle_f64| over seq and frame embeddings of the first n windows."""
    if "seq32" not in ref:
        s32, f32, _ = _oracle(ref["shape"], torch.float32).forward(ref["x"])
        ref["seq32"], ref["frames32"] = s32.double(), f32.double()
    return max((ref["seq32"][:n] - ref["seq"][:n]).abs().max().item(),
               (ref["frames32"][:n] - ref["frames"][:n]).abs().max().item())


def _encoder(ops, shape, compute):
    d, heads, layers, n_mod = shape
    return ops.Encoder(_sd(shape), time_layers=layers, time_heads=heads, d_model=d, device=DEV, compute=compute,
                       n_modalities=n_mod)


def _check(tag, out, ref, n, f16_layers=None):
    """seq, all 33 frame rows and the per-window TC of the first n reference windows.  f16_layers None: an f32-class
    mode (project bar + the tight bar); else the f16 bars at that depth."""
    seq, fe, tcw = out
    e_seq = (seq.cpu().double() - ref["seq"][:n]).abs().max().item()
    e_fe = (fe.cpu().double() - ref["frames"][:n]).abs().max().item()
    e_tc = (tcw.cpu().double() - ref["tc"][:n]).abs().max().item()
    if f16_layers is None:
        e_ref = _e_ref(ref, n)
        tight = max(20 * e_ref, 2e-6)
        print(f"{tag}: seq {e_seq:.2e} frame {e_fe:.2e} tc {e_tc:.2e} (e_ref {e_ref:.2e}, tight bar {tight:.2e})")
        assert e_seq < 2e-5 and e_fe < 2e-5 and e_tc < 1e-5, (e_seq, e_fe, e_tc)
        assert e_seq <= tight and e_fe <= tight, (e_seq, e_fe, tight)
    else:
        bar = 2e-4 if f16_layers <= 4 else F16_BAR[f16_layers]
        print(f"{tag}: seq {e_seq:.2e} frame {e_fe:.2e} tc {e_tc:.2e} (f16 bar {bar:.0e})")
        assert e_seq < bar and e_fe < bar and e_tc < bar / 2, (e_seq, e_fe, e_tc, bar)


def _run_tiled(vg, monkeypatch, layers, mode, n, n_max, n_mod=5, tx_w=0, same_bits_k=None):
    """One tiled-encoder case.  mode: f32x3 | f32x3-unfused | f32 | f16; tx_w: windows per transformer workgroup forced
    through vge_debug_set_tx_windows (0: automatic); same_bits_k: f16 only, encode(feats[:k]) must equal seq[:k] bit
    for bit."""
    L, ops = vg
    shape = (256, 8, layers, n_mod)
    ref = _reference(shape, n_max)
    if mode == "f32x3-unfused":
        monkeypatch.setenv("VGE_X3_UNFUSED", "1")
    compute = mode.split("-")[0]
    enc = _encoder(ops, shape, compute)
    feats = ref["x"][:n].to(DEV)
    so = L.load()
    so.vge_debug_set_tx_windows(tx_w)
    try:
        out = enc.encode(feats, frame_embed=True, tc=True)
        torch.cuda.synchronize()
        if same_bits_k:
            s2, _, _ = enc.encode(feats[:same_bits_k].contiguous(), frame_embed=False, tc=True)
            torch.cuda.synchronize()
    finally:
        so.vge_debug_set_tx_windows(0)
    _check(f"{mode} layers={layers} n={n} mods={n_mod} W={tx_w or 'auto'}", out, ref, n,
           f16_layers=layers if compute == "f16" else None)
    if same_bits_k:
        assert torch.equal(s2, out[0][:same_bits_k])


TILED_MODES = ["f32x3", "f32x3-unfused", "f32", "f16"]


@gpu
@pytest.mark.parametrize("mode", TILED_MODES)
@pytest.mark.parametrize("layers", [1, 2, 3, 5, 8])
def test_tiled_layer_counts(vg, monkeypatch, layers, mode):
    """The layer-count-dependent code of the tiled kernels: the fused transformer's nseg = 1 + 12 n_layers segment
    ring (its last refill re-reads its own chunks), its special-cased last layer and its 8-entry layer table; the
    per-layer 3xfp16 kernels; the exact-f32 layer loop.  Odd batch: the last conv workgroup is half empty."""
    _run_tiled(vg, monkeypatch, layers, mode, 37, 37, same_bits_k=19 if mode == "f16" else None)


@gpu
@pytest.mark.parametrize("mode", TILED_MODES)
@pytest.mark.parametrize("layers", [1, 8])
def test_tiled_layer_counts_one_window(vg, monkeypatch, layers, mode):
    _run_tiled(vg, monkeypatch, layers, mode, 1, 37)


@gpu
@pytest.mark.parametrize("n", [1, 37])
def test_per_layer_x3_path_at_the_golden_shape(vg, monkeypatch, n):
    """VGE_X3_UNFUSED=1 at 4 layers: the per-layer 3xfp16 kernels (what VGE_F32X3 runs above 8 layers) at the golden
    checkpoint's shape."""
    _run_tiled(vg, monkeypatch, 4, "f32x3-unfused", n, 37)


@gpu
@pytest.mark.parametrize("mode", ["f32x3", "f16"])
@pytest.mark.parametrize("layers", [1, 8])
def test_tiled_two_windows_per_workgroup(vg, monkeypatch, layers, mode):
    """W = 2 forced; n = 5: the last workgroup holds one window."""
    _run_tiled(vg, monkeypatch, layers, mode, 5, 37, tx_w=2, same_bits_k=3 if mode == "f16" else None)


@gpu
@pytest.mark.parametrize("layers", [1, 3])
def test_f16_two_workgroups_per_cu(vg, monkeypatch, layers):
    """transformer_x3_kernel<false, false, 1, 2>, chosen by itself above one window per CU (293 > 256 CUs); the first
    64 windows encoded alone (one workgroup per CU) give the same bits."""
    _run_tiled(vg, monkeypatch, layers, "f16", 293, 293, same_bits_k=64)


@gpu
@pytest.mark.parametrize("mode", ["f32x3", "f32"])
@pytest.mark.parametrize("layers", [9, 12])
def test_tiled_more_than_eight_layers(vg, monkeypatch, layers, mode):
    """Beyond the fused kernel's layer table: only the values are asserted, not which kernels ran."""
    _run_tiled(vg, monkeypatch, layers, mode, 5, 5)


@gpu
@pytest.mark.parametrize("layers", [9, 12])
def test_f16_refuses_more_than_eight_layers(vg, layers):
    L, ops = vg
    with pytest.raises(L.UnsupportedModelError):
        _encoder(ops, (256, 8, layers, 5), "f16")


@gpu
@pytest.mark.parametrize("mode", ["f32x3", "f32"])
def test_tiled_four_modalities(vg, monkeypatch, mode):
    """The keypoint-less layout (feats rows of 2356, 8 conv encoders) at 2 layers."""
    _run_tiled(vg, monkeypatch, 2, mode, 5, 5, n_mod=4)


# ---- the generic exact-f32 kernels (vge_encoder_gen.hip)

GENERIC_5 = [s for s in GENERIC_SHAPES if s[3] == 5]


@gpu
@pytest.mark.parametrize("n", [1, 5, 37])
@pytest.mark.parametrize("shape", GENERIC_5, ids=shape_key)
def test_generic_widths_and_heads(vg, shape, n):
    """d_model 96 .. 256: gen_conv_kernel's second ci0 pass and its co >= cout mask, the lane + 64 j < d masks of
    gen_fuse / gen_add_ln / gen_embed_tc with a partial last group, gen_gemm_kernel's ragged N; head dims 8 .. 64."""
    _, ops = vg
    ref = _reference(shape, 37)
    enc = _encoder(ops, shape, "f32")
    out = enc.encode(ref["x"][:n].to(DEV), frame_embed=True, tc=True)
    assert out[0].shape == (n, shape[0]) and out[1].shape == (n, 33, shape[0])
    _check(f"generic {shape_key(shape)} n={n}", out, ref, n)


@gpu
def test_generic_four_modalities(vg):
    """col_diff = VGE_RAW_DIM_NOKP: the 4-modality column offsets of the generic path."""
    _, ops = vg
    shape = (96, 3, 2, 4)
    ref = _reference(shape, 5)
    enc = _encoder(ops, shape, "f32")
    assert enc.feat_dim == 2356
    _check(f"generic {shape_key(shape)} n=5", enc.encode(ref["x"].to(DEV), frame_embed=True, tc=True), ref, 5)


@gpu
@pytest.mark.parametrize("frame_embed,tc", [(False, True), (True, False)])
def test_generic_null_outputs(vg, frame_embed, tc):
    """gen_embed_tc_kernel with a null frame / TC destination: the outputs that are requested keep their values."""
    _, ops = vg
    shape = (160, 5, 2, 5)
    ref = _reference(shape, 37)
    enc = _encoder(ops, shape, "f32")
    seq, fe, tcw = enc.encode(ref["x"][:5].to(DEV), frame_embed=frame_embed, tc=tc)
    assert (fe is None) == (not frame_embed) and (tcw is None) == (not tc)
    tight = max(20 * _e_ref(ref, 5), 2e-6)
    e_seq = (seq.cpu().double() - ref["seq"][:5]).abs().max().item()
    assert e_seq < 2e-5 and e_seq <= tight, (e_seq, tight)
    if fe is not None:
        e_fe = (fe.cpu().double() - ref["frames"][:5]).abs().max().item()
        assert e_fe < 2e-5 and e_fe <= tight, (e_fe, tight)
    if tcw is not None:
        assert (tcw.cpu().double() - ref["tc"][:5]).abs().max().item() < 1e-5


@gpu
@pytest.mark.parametrize("d_model,heads", [(48, 3), (288, 9), (256, 2), (96, 5)])
def test_generic_refuses_unsupported_shapes(vg, d_model, heads):
    """d_model no multiple of 32, above 256, a head dim of 128, a head count that does not divide d_model:
    VGE_ERR_UNSUPPORTED from vge_encoder_create's shape check, before any weight is read."""
    L, ops = vg
    with pytest.raises(L.UnsupportedModelError):
        ops.Encoder({}, time_layers=2, time_heads=heads, d_model=d_model, device=DEV, compute="f32")


# ---- the reductions behind the encoder (vge_score.hip) at those widths

WIDTHS = [32, 96, 160, 224, 256]


def _unit_rows(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(*shape, generator=g), dim=-1)


@gpu
@pytest.mark.parametrize("d", WIDTHS)
def test_tc_windows_at_width(vg, d):
    """B = 7 (no multiple of the 4 windows per workgroup), T1 = 33, unit rows, against float64; T1 = 2 has no pair of
    frames: NaN."""
    _, ops = vg
    fe = _unit_rows(7, 33, d, seed=d)
    ref = _tc_ref(fe.double())
    got = ops.tc_windows(fe.to(DEV)).cpu()
    err = (got.double() - ref).abs().max().item()
    print(f"tc_windows d={d}: {err:.2e}")
    assert err < 1e-5
    assert torch.isnan(ops.tc_windows(fe[:, :2].contiguous().to(DEV)).cpu()).all()


def _class_ids(layout, used):
    """1,300 windows in the 3 classes `used`.  sorted: runs with boundaries at windows 127|128 (a 128-window wave
    quarter), 512|513 (one past a 512-window segment) and 671|672 (a 32-row load block inside a quarter); interleaved:
    class = used[i % 3], runs of length 1."""
    n = 1300
    i = torch.arange(n)
    if layout == "interleaved":
        y = torch.tensor(used)[i % 3]
    else:
        y = torch.empty(n, dtype=torch.int64)
        y[:128], y[128:513], y[513:672], y[672:] = used[0], used[1], used[2], used[0]
    return y


@gpu
@pytest.mark.parametrize("layout,C,used", [("sorted", 5, (0, 2, 4)), ("interleaved", 5, (0, 2, 4)),
                                           ("sorted", 70, (3, 65, 69))])
@pytest.mark.parametrize("d", WIDTHS)
def test_centroids_grouped_by_class_at_width(vg, d, layout, C, used):
    """centroid_partial_kernel's register runs across load blocks, wave quarters and segments (the real set comes
    grouped by class), two class blocks (C = 70), classes without windows (centroid = the zero vector), ids outside
    [0, C) (ignored), against float64: counts exact, sums 1e-3, centroids 2e-5; two launches give the same bits."""
    _, ops = vg
    n = 1300
    seq = _unit_rows(n, d, seed=d + C)
    y = _class_ids(layout, used)
    y[40], y[700] = -1, C + 3          # no class of this set
    ok = (y >= 0) & (y < C)
    ref_s = torch.zeros(C, d, dtype=torch.float64).index_add_(0, y[ok], seq[ok].double())
    ref_c = torch.zeros(C, dtype=torch.float64).index_add_(0, y[ok], torch.ones(int(ok.sum()), dtype=torch.float64))
    m = ref_s / ref_c.clamp_min(1).unsqueeze(1)
    ref = m / m.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    ds, dy = seq.to(DEV), y.to(torch.int32).to(DEV)
    outs = []
    for _ in range(2):
        s = torch.zeros(C, d, device=DEV)
        c = torch.zeros(C, device=DEV)
        ops.centroid_accumulate(ds, dy, s, c)
        cent = ops.centroid_finalize(s, c)
        outs.append((s.cpu(), c.cpu(), cent.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    s, c, cent = outs[0]
    assert torch.equal(c.double(), ref_c)
    e_s = (s.double() - ref_s).abs().max().item()
    e_c = (cent.double() - ref).abs().max().item()
    print(f"centroids d={d} {layout} C={C}: sums {e_s:.2e} centroids {e_c:.2e}")
    assert e_s < 1e-3 and e_c < 2e-5
    empty = [k for k in range(C) if k not in used]
    assert (ref_c[empty] == 0).all() and (cent[empty] == 0).all()


@gpu
@pytest.mark.parametrize("d", WIDTHS)
def test_score_videos_at_width(vg, d):
    """V = 6 (no multiple of the 4 videos per workgroup); videos of 1, 2, 0, 65, 130 and 2 windows (the TC loop
    strides 64 lanes); the 65-window video has class -1 (AC NaN, TC computed); the 0-window video has neither; the
    last video's two windows are opposite, so its mean is exactly zero, the 1e-12 clamp decides and its AC is the
    centroid's norm."""
    _, ops = vg
    counts = [1, 2, 0, 65, 130, 2]
    vcls = [1, 0, 2, -1, 2, 1]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    n = int(first[-1])
    seq = _unit_rows(n, d, seed=3 * d)
    seq[n - 1] = -seq[n - 2]
    g = torch.Generator().manual_seed(d)
    tcw = torch.rand(n, generator=g)
    cent = _unit_rows(3, d, seed=5 * d) * torch.tensor([[0.7], [1.3], [1.0]])
    ac, tc = ops.score_videos(seq.to(DEV), tcw.to(DEV), torch.from_numpy(first).to(DEV),
                              torch.tensor(vcls, dtype=torch.int32, device=DEV), cent.to(DEV))
    ac, tc = ac.cpu(), tc.cpu()
    assert ac.dtype == torch.float32 and tc.dtype == torch.float64
    for v, (k, c) in enumerate(zip(counts, vcls)):
        w0, w1 = int(first[v]), int(first[v + 1])
        if k == 0:
            assert torch.isnan(tc[v]) and torch.isnan(ac[v])
            continue
        ref_tc = tcw[w0:w1].double().mean().item()
        assert abs(tc[v].item() - ref_tc) <= 1e-12 * abs(ref_tc), (v, tc[v].item(), ref_tc)
        if c < 0:
            assert torch.isnan(ac[v])
            continue
        z = seq[w0:w1].double().mean(0)
        z = z / z.norm().clamp_min(1e-12)
        ref_ac = (z - cent[c].double()).norm().item()
        assert abs(ac[v].item() - ref_ac) < 1e-5, (v, ac[v].item(), ref_ac)
    assert abs(ac[5].item() - cent[1].double().norm().item()) < 1e-5   # the zero-mean video
    print(f"score_videos d={d}: ac {ac.tolist()} tc {tc.tolist()}")
