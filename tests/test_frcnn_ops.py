"""The gate detector's non-GEMM kernels op by op, through the vge_op_* entry points of include/vge_frcnn.h (each one
calls the launcher vge_frcnn_detect calls), on the crafted cases of tests/frcnn_op_cases.py: every test gives the
oracle the GPU's exact inputs.  tests/test_frcnn_op_cases.py asserts, without a GPU, that each case has the property
it is named for.

  preprocess     resized == the oracle's PIL resample byte for byte; the bf16 tensor == bf16(f32((f32(v) - mean) / std))
                 bit for bit in BGR order (numpy float32: a subtract and a divide, correctly rounded on both sides,
                 then one round to nearest even), +0 in channels 3..7 and in the padding, over a NaN pre-fill
  pool_s2        == torch max_pool2d of the bf16 values
  stem_pool      float64 conv 7x7 / 2 + bias + ReLU on the bf16 operands, one bf16 rounding, max_pool2d(3, 2, 1):
                 |d| <= 2^-7 |ref| + 1e-4 (the grouped conv test's bound for the same rounding point)
  rpn_proposals  oracle proposals(): n_prop equal, scores bit-equal in order, boxes within 2e-3 (exact where every
                 delta is 0); the per-level top-k (`sel`) against find_top_rpn_proposals' own, so a failure is placed
  roi_align      oracle box_features() on the same bf16 levels: |d| <= 2^-7 |ref| + max(1e-6, 2^-20 sum |w v| / count),
                 the sum taken by the oracle's ROIAlign of |features| (the weights are >= 0); the three kernels
  det_post       oracle inference() + postprocess(): counts, classes, order, persons equal; scores rtol 2e-6; boxes
                 rtol 1e-5 + 2e-3 (resized pixels) / 1e-3 (frame pixels), as tests/frcnn_checks.py
No case is skipped for a probability near the score threshold: the cases keep every probability 1e-3 away from it
or exactly on it (asserted on the CPU).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import frcnn as O
from tests import frcnn_op_cases as FC

DEV = "cuda:0"
gpu = pytest.mark.gpu
BF = torch.bfloat16
SENT16 = 0x7FC1
NAN = float("nan")


def _lib():
    from vge import frcnn as FR
    from vge import lib as L
    return FR._sig(L.load())


def _report(tag, err, bound):
    """worst error / bound over the elements, printed (pytest -s) before the assertion"""
    ratio = float((err / bound).max()) if err.numel() else 0.0
    print(f"{tag}: worst error / bound {ratio:.3f} (max error {float(err.max()) if err.numel() else 0.0:.3e})")
    return ratio


# ------------------------------------------------------------------------------ CPU: refusals, no GPU work
_N = None
_HW5 = (C.c_int * 10)(20, 20, 10, 10, 5, 5, 3, 3, 1, 1)
_HW5_BAD = (C.c_int * 10)(20, 20, 10, 0, 5, 5, 3, 3, 1, 1)
_HW5_BIG = (C.c_int * 10)(8192, 4096, 10, 10, 5, 5, 3, 3, 1, 1)
_HW4 = (C.c_int * 8)(8, 8, 4, 4, 2, 2, 1, 1)
_HW4_BIG = (C.c_int * 8)(2048, 2048, 4, 4, 2, 2, 1, 1)
_P5, _P4 = (C.c_void_p * 5)(), (C.c_void_p * 4)()     # null level pointers: a launch would fault, none happens


def _det(**kw):
    a = dict(head=_N, ld=408, P=1000, K=80, dpi=100, props=_N, n_prop=_N, n=1, ih=800, iw=800, oh=256, ow=256,
             st=0.25, nt=0.5, gt=0.5)
    a.update(kw)
    return (a["head"], a["ld"], a["P"], a["K"], a["dpi"], a["props"], a["n_prop"], a["n"], a["ih"], a["iw"], a["oh"],
            a["ow"], a["st"], a["nt"], a["gt"], _N, _N, _N, _N, _N, _N, _N)


REFUSALS = [
    ("vge_op_frcnn_preprocess", "null pointers", (_N, 1, 64, 64, 32, 64, _N, _N, _N)),
    ("vge_op_frcnn_preprocess", "n 0", (_N, 0, 64, 64, 32, 64, _N, _N, _N)),
    ("vge_op_frcnn_preprocess", "W 0", (_N, 1, 64, 0, 32, 64, _N, _N, _N)),
    ("vge_op_frcnn_preprocess", "min_size 0", (_N, 1, 64, 64, 0, 64, _N, _N, _N)),
    ("vge_op_frcnn_preprocess", "max_size < min_size", (_N, 1, 64, 64, 32, 16, _N, _N, _N)),
    ("vge_op_frcnn_preprocess", "an axis rounds to 0", (_N, 1, 1, 667, 8, 333, _N, _N, _N)),
    ("vge_op_frcnn_preprocess", "2^31 pixels", (_N, 4096, 1024, 1024, 1024, 1024, _N, _N, _N)),
    ("vge_op_frcnn_pool_s2", "null pointers", (_N, _N, 1, 8, 8, 64, 3, _N)),
    ("vge_op_frcnn_pool_s2", "K 2", (_N, _N, 1, 8, 8, 64, 2, _N)),
    ("vge_op_frcnn_pool_s2", "C % 8", (_N, _N, 1, 8, 8, 60, 3, _N)),
    ("vge_op_frcnn_pool_s2", "C 0", (_N, _N, 1, 8, 8, 0, 3, _N)),
    ("vge_op_frcnn_pool_s2", "H 0", (_N, _N, 1, 0, 8, 64, 3, _N)),
    ("vge_op_frcnn_pool_s2", "n 0", (_N, _N, 0, 8, 8, 64, 1, _N)),
    ("vge_op_frcnn_stem_pool", "null pointers", (_N, _N, _N, _N, 1, 32, 32, _N)),
    ("vge_op_frcnn_stem_pool", "hp % 32", (_N, _N, _N, _N, 1, 48, 32, _N)),
    ("vge_op_frcnn_stem_pool", "wp % 32", (_N, _N, _N, _N, 1, 32, 36, _N)),
    ("vge_op_frcnn_stem_pool", "n 0", (_N, _N, _N, _N, 0, 32, 32, _N)),
    ("vge_op_frcnn_stem_pool", "2^31 pixels", (_N, _N, _N, _N, 4096, 1024, 1024, _N)),
    ("vge_op_rpn_proposals", "null pointers", (_P5, _HW5, 1, 1000, 1000, 0.7, 80, 80, _N, _N, _N, _N, _N, _N)),
    ("vge_op_rpn_proposals", "null arrays", (_N, _N, 1, 1000, 1000, 0.7, 80, 80, _N, _N, _N, _N, _N, _N)),
    ("vge_op_rpn_proposals", "pre_topk 1025", (_P5, _HW5, 1, 1025, 1000, 0.7, 80, 80, _N, _N, _N, _N, _N, _N)),
    ("vge_op_rpn_proposals", "pre_topk 0", (_P5, _HW5, 1, 0, 1000, 0.7, 80, 80, _N, _N, _N, _N, _N, _N)),
    ("vge_op_rpn_proposals", "post_topk 1025", (_P5, _HW5, 1, 1000, 1025, 0.7, 80, 80, _N, _N, _N, _N, _N, _N)),
    ("vge_op_rpn_proposals", "nms_thresh 0", (_P5, _HW5, 1, 1000, 1000, 0.0, 80, 80, _N, _N, _N, _N, _N, _N)),
    ("vge_op_rpn_proposals", "nms_thresh 1.5", (_P5, _HW5, 1, 1000, 1000, 1.5, 80, 80, _N, _N, _N, _N, _N, _N)),
    ("vge_op_rpn_proposals", "n 0", (_P5, _HW5, 0, 1000, 1000, 0.7, 80, 80, _N, _N, _N, _N, _N, _N)),
    ("vge_op_rpn_proposals", "img_w 0", (_P5, _HW5, 1, 1000, 1000, 0.7, 80, 0, _N, _N, _N, _N, _N, _N)),
    ("vge_op_rpn_proposals", "a level of width 0", (_P5, _HW5_BAD, 1, 1000, 1000, 0.7, 80, 80, _N, _N, _N, _N, _N, _N)),
    ("vge_op_rpn_proposals", "a level of 2^25 cells", (_P5, _HW5_BIG, 1, 1000, 1000, 0.7, 80, 80, _N, _N, _N, _N, _N, _N)),
    ("vge_op_roi_align", "null pointers", (_P4, _HW4, _N, _N, 1, 100, _N, _N)),
    ("vge_op_roi_align", "null arrays", (_N, _N, _N, _N, 1, 100, _N, _N)),
    ("vge_op_roi_align", "P 1025", (_P4, _HW4, _N, _N, 1, 1025, _N, _N)),
    ("vge_op_roi_align", "P 0", (_P4, _HW4, _N, _N, 1, 0, _N, _N)),
    ("vge_op_roi_align", "n 0", (_P4, _HW4, _N, _N, 0, 100, _N, _N)),
    ("vge_op_roi_align", "a level of 2^22 cells", (_P4, _HW4_BIG, _N, _N, 1, 100, _N, _N)),
    ("vge_op_det_post", "null pointers", _det()),
    ("vge_op_det_post", "score_thresh 0.19", _det(st=0.19)),
    ("vge_op_det_post", "score_thresh 1", _det(st=1.0)),
    ("vge_op_det_post", "K 128", _det(K=128, ld=648)),
    ("vge_op_det_post", "K 0", _det(K=0)),
    ("vge_op_det_post", "P 1025", _det(P=1025)),
    ("vge_op_det_post", "det_per_img 1025", _det(dpi=1025)),
    ("vge_op_det_post", "det_per_img 0", _det(dpi=0)),
    ("vge_op_det_post", "ld < 5 K + 1", _det(ld=400)),
    ("vge_op_det_post", "nms_thresh 0", _det(nt=0.0)),
    ("vge_op_det_post", "n 0", _det(n=0)),
    ("vge_op_det_post", "frame height 0", _det(oh=0)),
]


@pytest.mark.parametrize("entry,what,args", REFUSALS, ids=[f"{e[7:]}-{w}" for e, w, _ in REFUSALS])
def test_op_entry_refuses(entry, what, args):
    lib = _lib()
    assert getattr(lib, entry)(*args) == 1, what
    assert entry.encode() in lib.vge_last_error(), lib.vge_last_error()


# ------------------------------------------------------------------------------ GPU helpers
@pytest.fixture(scope="module")
def FR():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vge import frcnn
    return frcnn


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nan_bf16(shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device=DEV).view(BF)


# ------------------------------------------------------------------------------ preprocess
PRE_GEOMS = {  # H, W, min_size, max_size -> resized, padded
    "up-pad-both": (5, 7, 16, 27),            # 16 x 22 in 32 x 32
    "up-pad-h": (40, 24, 32, 64),             # 53 x 32 in 64 x 32
    "capped-pad-both": (33, 70, 64, 107),     # 50 x 107 in 64 x 128
    "one-row": (1, 40, 8, 333),               # 8 x 320 in 32 x 320
    "down-pad-w": (64, 96, 32, 64),           # 32 x 48 in 32 x 64
    "down-no-pad": (128, 64, 32, 64),         # 64 x 32
}


@gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", list(PRE_GEOMS))
def test_preprocess_bit_exact(FR, geom, n):
    H, W, mn, mx = PRE_GEOMS[geom]
    nh, nw = O.output_shape(H, W, mn, mx)
    hp, wp = -(-nh // 32) * 32, -(-nw // 32) * 32
    if geom == "down-no-pad":
        assert (hp, wp) == (nh, nw) and nh < H
    if geom == "up-pad-both":
        assert hp > nh and wp > nw and nh > H
    rng = np.random.default_rng(H * 100 + W + n)
    fr = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    fr.reshape(-1)[:4] = (0, 255, 0, 255)
    out = _nan_bf16((n, hp, wp, 8))
    resized = torch.full((n, nh, nw, 3), 0xAB, dtype=torch.uint8, device=DEV)
    FR.preprocess(torch.from_numpy(fr).to(DEV), mn, mx, out, resized)
    got_r = resized.cpu().numpy()
    want_r = np.stack([O.resize_pil(f, nh, nw) for f in fr])
    np.testing.assert_array_equal(got_r, want_r)
    mean = np.asarray(O.PIXEL_MEAN, np.float32)
    std = np.asarray(O.PIXEL_STD, np.float32)
    v = want_r[..., ::-1].astype(np.float32)                      # BGR
    x = ((v - mean) / std).astype(np.float32)
    want = np.zeros((n, hp, wp, 8), np.int16)
    want[:, :nh, :nw, :3] = torch.from_numpy(x).to(BF).view(torch.int16).numpy()
    got = out.view(torch.int16).cpu().numpy()
    assert (got[..., 3:] == 0).all() and (got[:, nh:] == 0).all() and (got[:, :, nw:] == 0).all(), "+0 expected"
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist())


# ------------------------------------------------------------------------------ pool_s2
@gpu
@pytest.mark.parametrize("K", [3, 1])
@pytest.mark.parametrize("Cc", [64, 256])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (9, 10), (8, 8), (2, 3)])
def test_pool_s2_equals_max_pool2d(FR, H, W, Cc, K):
    n = 3
    x = torch.randn((n, H, W, Cc), generator=_gen(H * 31 + W + Cc + K)).to(BF)
    x[0, 0, 0, :8] = torch.tensor([-1.0, 0.0, -0.0, 3.0, -3.0e38, 3.0e38, 1e-30, -1e-30]).to(BF)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = _nan_bf16((n, Ho, Wo, Cc))
    FR.pool_s2(x.to(DEV), out, K)
    ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), K, 2, K // 2).permute(0, 2, 3, 1)
    assert ref.shape == (n, Ho, Wo, Cc)
    assert torch.equal(out.float().cpu(), ref)


# ------------------------------------------------------------------------------ stem + pool
@gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hp,wp", [(32, 32), (32, 96), (96, 32), (64, 64)])
def test_stem_pool_vs_float64(FR, hp, wp, n):
    g = _gen(hp * 7 + wp + n)
    x = torch.zeros((n, hp, wp, 8))
    x[..., :3] = torch.randn((n, hp, wp, 3), generator=g) * 1.5
    if n > 1:      # a frame whose valid region ends inside the last tile (7 x 16 pooled pixels), zeros beyond it
        x[1, hp - 13:] = 0
        x[1, :, wp - 19:] = 0
    x = x.to(BF)
    w = torch.randn((64, 3, 7, 7), generator=g) / 12.0
    b = 0.1 * torch.randn(64, generator=g)
    out = _nan_bf16((n, hp // 4, wp // 4, 64))
    FR.stem_pool(x.to(DEV), w.numpy(), b.numpy(), out)
    y = F.conv2d(x[..., :3].double().permute(0, 3, 1, 2), w.to(BF).double(), b.double(), stride=2, padding=3).relu()
    ref = F.max_pool2d(y.float().to(BF).float(), 3, 2, 1).permute(0, 2, 3, 1)
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    assert float((ref > 0).float().mean()) > 0.5 and float(ref.max()) > 1.0
    err = (got - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 1e-4
    _report(f"stem_pool {hp} x {wp} n {n}", err, bound)
    assert bool((err <= bound).all()), float((err - bound).max())


# ------------------------------------------------------------------------------ RPN proposals
def _bits(t):
    return t.contiguous().view(torch.int32)


@gpu
@pytest.mark.parametrize("name", FC.RPN_NAMES)
def test_rpn_proposals_vs_oracle(FR, name):
    c = FC.rpn_cases()[name]
    n, P = c.n, c.post_topk
    props = torch.full((n, P, 5), NAN, device=DEV)
    n_prop = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    sel = torch.full((n, 5, 1024, 8), NAN, device=DEV)
    kept = torch.full((n, 5, 1024, 8), NAN, device=DEV)
    kcount = torch.full((n, 5), -1, dtype=torch.int32, device=DEV)
    FR.rpn_proposals([torch.from_numpy(t).to(DEV) for t in c.levels], c.pre_topk, P, c.nms, c.image_size, props,
                     n_prop, sel, kept, kcount)
    props, n_prop, sel, kcount = props.cpu(), n_prop.cpu(), sel.cpu(), kcount.cpu()
    worst = 0.0
    for f in range(n):
        for l in range(5):          # select: the level's top-k in order, the decoded boxes, the valid flags
            v, i, box, ok = FC.rpn_select_oracle(c, f, l)
            k = v.shape[0]
            s = sel[f, l, :k]
            assert torch.equal(_bits(s[:, 4]), _bits(v)), f"frame {f} level {l}: the top-{k} logits or their order"
            assert torch.equal(s[:, 5] != 0, ok), f"frame {f} level {l}: valid flags"
            if bool(ok.any()):
                d = (s[ok][:, :4] - box[ok]).abs()
                assert float(d.max()) <= (0.0 if c.zero_deltas else 2e-3), (f, l, float(d.max()))
        pb, ps = FC.rpn_oracle(c, f)
        m = int(n_prop[f])
        assert m == pb.shape[0], (f, m, pb.shape[0])
        assert int(kcount[f].sum()) >= m
        g = props[f, :m]
        assert torch.equal(_bits(g[:, 4]), _bits(ps)), f"frame {f}: proposal order / scores differ"
        err = float((g[:, :4] - pb).abs().max()) if m else 0.0
        worst = max(worst, err)
        assert err <= (0.0 if c.zero_deltas else 2e-3), (f, err)
        assert bool(torch.isnan(props[f, m:]).all()), "rows behind n_prop were written"
    print(f"rpn_proposals {name}: n_prop {n_prop.tolist()}, max |box d| {worst:.2e} (bound "
          f"{0.0 if c.zero_deltas else 2e-3:.0e}; {c.note})")


# ------------------------------------------------------------------------------ ROIAlign
@pytest.fixture(scope="module")
def roi(FR):
    """The three kernels' outputs on the one ROI case, and the oracle's reference with its per-bin magnitude."""
    c = FC.roi_case()
    lib = _lib()
    lib.vge_debug_set_roi_direct.argtypes = [C.c_int]
    n, P = c.props.shape[:2]
    lv = [t.to(DEV) for t in c.levels]
    props, n_prop = torch.from_numpy(c.props).to(DEV), torch.from_numpy(c.n_prop).to(DEV)
    got = {}
    try:
        for mode in (0, 1, 2):
            lib.vge_debug_set_roi_direct(mode)
            out = _nan_bf16((n, P, 49, 256))
            FR.roi_align(lv, props, n_prop, out)
            got[mode] = out.cpu()
    finally:
        lib.vge_debug_set_roi_direct(0)
    plain = O.OracleFrcnn({}, FC.oracle().c, bf16=False)
    to_rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, 49, 256)  # noqa: E731
    ref, mag = {}, {}
    for f in (0, 2):      # each frame has its own maps; frame 2 holds the first boxes of frame 0
        m = int(c.n_prop[f])
        pf = [t[f].float().permute(2, 0, 1).contiguous() for t in c.levels]
        ref[f] = to_rows(FC.oracle().box_features(pf, c.boxes()[:m]))                  # [m, 49, 256], bf16 values
        mag[f] = to_rows(plain.box_features([p.abs() for p in pf], c.boxes()[:m]))    # sum |w v| / count per bin
    return dict(case=c, got=got, ref=ref, mag=mag)


@gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_roi_align_vs_oracle(roi, mode):
    c = roi["case"]
    lv = O.assign_levels(c.boxes())
    for f in (0, 2):
        m = int(c.n_prop[f])
        ref, mag = roi["ref"][f].double(), roi["mag"][f].double()
        bound = 2.0 ** -7 * ref.abs() + torch.clamp(2.0 ** -20 * mag, min=1e-6)
        got = roi["got"][mode][f, :m].double()
        assert torch.isfinite(got).all()
        err = (got - ref).abs()
        for name, sl in c.groups.items():
            if sl.start < m:
                e, b = err[sl.start:min(sl.stop, m)], bound[sl.start:min(sl.stop, m)]
                _report(f"roi_align mode {mode} frame {f} {name} (levels {sorted(set(lv[sl].tolist()))})", e, b)
        assert bool((err <= bound).all()), float((err / bound).max())


@gpu
def test_roi_align_sample_loop_equals_sample_order_kernel(roi):
    assert torch.equal(roi["got"][2].view(torch.int16), roi["got"][1].view(torch.int16))


@gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_roi_align_empty_slots_are_zero(roi, mode):
    c = roi["case"]
    bits = roi["got"][mode].view(torch.int16)
    assert c.n_prop.tolist()[1] == 0
    for f, m in enumerate(c.n_prop.tolist()):
        assert bool((bits[f, m:] == 0).all()), f"frame {f}: slots from n_prop on must be +0"
        assert not bool((bits[f, :m] == SENT16).any())


# ------------------------------------------------------------------------------ box inference + postprocess
@gpu
@pytest.mark.parametrize("name", FC.DET_NAMES)
def test_det_post_vs_oracle(FR, name):
    c = FC.det_cases()[name]
    n = len(c.n_prop)
    out = FR.det_post(torch.from_numpy(c.head).to(DEV), torch.from_numpy(c.props).to(DEV),
                      torch.from_numpy(c.n_prop).to(DEV), c.K, c.det_per_img, c.image_size, c.frame_hw,
                      c.score_thresh, c.nms_thresh, c.gate_thresh)
    out = {k: v.cpu() for k, v in out.items()}
    worst = 0.0
    for f in range(n):
        r = FC.det_oracle(c, f)
        m = int(out["n_pre"][f])
        assert m == r["b"].shape[0], (f, m, r["b"].shape[0])
        g = out["pre_dets"][f, :m]
        assert torch.equal(g[:, 5].long(), r["k"]), f"frame {f}: classes / order differ"
        if m:
            rel = float(((g[:, 4] - r["s"]).abs() / r["s"]).max())
            worst = max(worst, rel)
        np.testing.assert_allclose(g[:, 4].numpy(), r["s"].numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(g[:, :4].numpy(), r["b"].numpy(), rtol=1e-5, atol=2e-3)
        assert torch.equal((g[:, 2] - g[:, 0]) > 0, (r["b"][:, 2] - r["b"][:, 0]) > 0), "empty boxes differ"
        nd = int(out["n_dets"][f])
        assert nd == r["fb"].shape[0], (f, nd, r["fb"].shape[0])
        d = out["dets"][f, :nd]
        np.testing.assert_allclose(d[:, :4].numpy(), r["fb"].numpy(), rtol=1e-5, atol=1e-3)
        np.testing.assert_allclose(d[:, 4].numpy(), r["fs"].numpy(), rtol=2e-6, atol=1e-7)
        assert torch.equal(d[:, 5].long(), r["fk"])
        assert int(out["n_person"][f]) == r["n_person"], (f, int(out["n_person"][f]), r["n_person"])
        pers = r["fk"] == 0
        np_ = min(2, int(pers.sum()))
        for j in range(np_):   # which two persons are reported: the first two class-0 instances
            np.testing.assert_allclose(out["person"][f, j, :4].numpy(), r["fb"][pers][j].numpy(), rtol=1e-5, atol=1e-3)
            np.testing.assert_allclose(out["person"][f, j, 4].numpy(), r["fs"][pers][j].numpy(), rtol=2e-6)
        assert bool((out["person"][f, np_:] == 0).all())
        assert bool(torch.isnan(out["pre_dets"][f, m:]).all()) and bool(torch.isnan(out["dets"][f, nd:]).all())
    print(f"det_post {name}: n_pre {out['n_pre'].tolist()} n_dets {out['n_dets'].tolist()} n_person "
          f"{out['n_person'].tolist()}; worst score error / 2e-6 = {worst / 2e-6:.3f}")
