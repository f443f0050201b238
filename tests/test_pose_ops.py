"""The pose extractors' non-GEMM kernels (vge_cnn.hip, vge_pose_head.hip), op by op through the vge_op_* entry points
of include/vge_dwpose.h, each against a plain high-precision reference of the same operation:

  depthwise 3 / 5 / 5 (one thread per output)  float64 conv + SiLU; the two 5 x 5 kernels bit-equal
  SPP pools, generic and LDS kernel             exact vs torch.max_pool2d; the two kernels bit-equal
  channel attention                             float64 mean -> fc -> hardsigmoid within the worst-case bound of
                                                sequential f32 sums; the scaled map exact from the att read back
  2x upsample, warp, letterbox + Focus          exact (the latter two vs the float32 host oracles, every uint8)
  ScaleNorms                                    within 1 bf16 ulp of float64
  GAU token mixing, VALU and MFMA kernel        float64, 4 x the error of torch float32 on the same lines + 1 bf16 ulp
  SimCC decode, YOLOX decode + two-person NMS   crafted inputs (ties, thresholds, borders), exact

Every output buffer sits in a guard band (rows before and after, a pixel stride wider than the channels written)
filled with a NaN bit pattern that must come back untouched.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

DEV = "cuda:0"
gpu = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 3                       # guard rows before and after every banded buffer
SENT16 = 0x7FC1                 # a bf16 quiet NaN
SENT32 = 0x7FC12345             # an f32 quiet NaN


# ------------------------------------------------------------------------------ CPU: refusals, no GPU work
def _lib():
    from vge import dwpose as D
    from vge import lib as L
    return D._sig(L.load())


# entry -> list of (what is refused, the arguments); every pointer is null, so a launch would fault: none happens
_N = None
REFUSALS = [
    ("vge_op_dwconv_bf16", "C % 8", (_N, 16, _N, _N, _N, 16, 1, 4, 4, 12, 5, _N)),
    ("vge_op_dwconv_bf16", "K", (_N, 16, _N, _N, _N, 16, 1, 4, 4, 16, 7, _N)),
    ("vge_op_dwconv_bf16", "ldy < C", (_N, 16, _N, _N, _N, 8, 1, 4, 4, 16, 5, _N)),
    ("vge_op_dwconv_bf16", "ldx < C", (_N, 8, _N, _N, _N, 16, 1, 4, 4, 16, 3, _N)),
    ("vge_op_spp_pool_bf16", "C % 8", (_N, 64, 1, 4, 4, 4, 5, 9, 13, 0, _N)),
    ("vge_op_spp_pool_bf16", "ld < 4 C", (_N, 24, 1, 4, 4, 8, 5, 9, 13, 0, _N)),
    ("vge_op_spp_pool_bf16", "variant 2 above 400 positions", (_N, 64, 1, 21, 20, 16, 5, 9, 13, 2, _N)),
    ("vge_op_spp_pool_bf16", "variant 2 on other pools", (_N, 64, 1, 4, 4, 16, 3, 5, 7, 2, _N)),
    ("vge_op_spp_pool_bf16", "variant 3", (_N, 64, 1, 4, 4, 16, 5, 9, 13, 3, _N)),
    ("vge_op_chan_attn_bf16", "C % 8", (_N, 16, 1, 4, 12, _N, _N, _N, _N, _N)),
    ("vge_op_chan_attn_bf16", "ld < C", (_N, 8, 1, 4, 16, _N, _N, _N, _N, _N)),
    ("vge_op_chan_attn_bf16", "C > 2048", (_N, 4096, 1, 4, 2056, _N, _N, _N, _N, _N)),
    ("vge_op_upsample2x_bf16", "C % 8", (_N, 16, _N, 16, 1, 2, 2, 4, _N)),
    ("vge_op_upsample2x_bf16", "ldy < C", (_N, 16, _N, 8, 1, 2, 2, 16, _N)),
    ("vge_op_warp_prep", "null pointers", (_N, 1, 4, 4, _N, _N, 1, 64, 32, _N, _N, _N)),
    ("vge_op_warp_prep", "no instance", (_N, 1, 4, 4, _N, _N, 0, 64, 32, _N, _N, _N)),
    ("vge_op_letterbox_focus", "odd S", (_N, 1, 4, 4, 63, _N, _N)),
    ("vge_op_letterbox_focus", "frame too small", (_N, 1, 1, 200, 64, _N, _N)),
    ("vge_op_head_scalenorm_t", "hw > 256", (_N, 136, 257, 133, 512, 1.0, 133, _N, _N)),
    ("vge_op_head_scalenorm_t", "Kp > 256", (_N, 136, 108, 133, 512, 1.0, 133, _N, _N)),
    ("vge_op_head_scalenorm_t", "ldy < K", (_N, 128, 108, 133, 128, 1.0, 133, _N, _N)),
    ("vge_op_scalenorm_rows", "D > 512", (_N, 520, 1.0, 4, _N, _N)),
    ("vge_op_gau_attn", "K > 136 on the VALU kernel", (_N, 1, 137, 128, 8, _N, _N, _N, 1, _N)),
    ("vge_op_gau_attn", "S = 160 on the VALU kernel", (_N, 1, 136, 128, 160, _N, _N, _N, 1, _N)),
    ("vge_op_gau_attn", "S = 168 on the MFMA kernel", (_N, 1, 136, 128, 168, _N, _N, _N, 2, _N)),
    ("vge_op_gau_attn", "S = 168 on either", (_N, 1, 136, 128, 168, _N, _N, _N, 0, _N)),
    ("vge_op_gau_attn", "odd S on the MFMA kernel", (_N, 1, 133, 128, 7, _N, _N, _N, 2, _N)),
    ("vge_op_gau_attn", "E % 128", (_N, 1, 133, 64, 8, _N, _N, _N, 0, _N)),
    ("vge_op_simcc_decode", "ld < WX + WY", (_N, 100, 64, 64, 2.0, 1, _N, _N)),
    ("vge_op_yolox_decode_nms", "null pointers", (_N, _N, _N, 16, 8, 4, 8, 16, 32, 1, 1.0, _N, _N, _N, _N, _N)),
    ("vge_op_yolox_decode_nms", "grid 0", (_N, _N, _N, 16, 0, 4, 8, 16, 32, 1, 1.0, _N, _N, _N, _N, _N)),
]


@pytest.mark.parametrize("entry,what,args", REFUSALS, ids=[f"{e[7:]}-{w}" for e, w, _ in REFUSALS])
def test_op_entry_refuses(entry, what, args):
    lib = _lib()
    assert getattr(lib, entry)(*args) == 1, what
    assert entry.encode() in lib.vge_last_error(), lib.vge_last_error()


def gau_lds_bytes(K, S):
    """(VALU kernel, MFMA kernel) LDS bytes of one instance, restated from the kernels' layouts: the VALU form is
    sized for 136 tokens (k-matrix rows of S + 1 floats, reused for 128-column v chunks; the 136 x 137 kernel
    matrix; 4 q rows), the MFMA form for K (base rows of S + 1 floats, reused for v rows of 160; K x (K | 1))."""
    valu = 4 * (136 * max(S + 1, 128) + 136 * 137 + 4 * S)
    mfma = 4 * (max(K * (S + 1), ((K + 1) & ~1) * 160) + K * (K | 1))
    return valu, mfma


GAU_LDS_LIMIT = 160 * 1024


def test_gau_lds_limit_arithmetic():
    """At 136 tokens the MFMA kernel fits up to S = 160 (162112 B) and not 168 (166464 B), the VALU kernel up to 152
    (160192 B) and not 160 (164672 B); the formerly accepted 256 needs 214336 / 218432 B."""
    assert gau_lds_bytes(136, 152) == (160192, 161568)
    assert gau_lds_bytes(136, 160) == (164672, 162112)
    assert gau_lds_bytes(136, 168) == (169152, 166464)
    assert gau_lds_bytes(136, 256) == (218432, 214336)
    assert max(gau_lds_bytes(136, 152)) <= GAU_LDS_LIMIT < min(gau_lds_bytes(136, 168))
    assert gau_lds_bytes(136, 160)[1] <= GAU_LDS_LIMIT < gau_lds_bytes(136, 160)[0]


# ------------------------------------------------------------------------------ GPU helpers
@pytest.fixture(scope="module")
def D():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vge import dwpose
    return dwpose


class Band:
    """rows x ld elements of `dtype` (bf16 / f32 / i32) with GUARD rows of sentinel before and after; `body` is the
    [rows, ld] view the kernel is given.  check(cols) asserts every element outside body[:, :cols] still holds the
    sentinel."""

    def __init__(self, rows, ld, dtype=BF):
        self.rows, self.ld = rows, ld
        self.two = dtype == BF
        self.raw = torch.full((rows + 2 * GUARD, ld), SENT16 if self.two else SENT32,
                              dtype=torch.int16 if self.two else torch.int32, device=DEV)
        self.body = (self.raw if dtype == torch.int32 else self.raw.view(dtype))[GUARD:GUARD + rows]

    def bits(self):
        return self.raw[GUARD:GUARD + self.rows].cpu()

    def check(self, cols, keep=None):
        """cols: the leading columns the kernel may write; keep = (n, bits): the first n of them must still hold
        `bits` (the input of an in-place op)."""
        raw = self.raw.cpu()
        sent = SENT16 if self.two else SENT32
        assert bool((raw[:GUARD] == sent).all()) and bool((raw[GUARD + self.rows:] == sent).all()), "guard rows written"
        body = raw[GUARD:GUARD + self.rows]
        assert bool((body[:, cols:] == sent).all()), "columns beyond the channels written were touched"
        if keep is not None:
            assert torch.equal(body[:, :keep[0]], keep[1]), "input channels changed"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ depthwise conv
DW_CASES = [  # n, H, W, C, ldx, ldy
    (2, 33, 7, 16, 24, 32),    # a strip of 1 row after a full one
    (1, 34, 3, 8, 16, 24),     # a strip of 2 rows; the window is wider than the map
    (1, 1, 1, 8, 16, 16),
    (3, 12, 9, 64, 72, 80),
    (1, 37, 2, 32, 40, 48),    # 5 rows in the second strip: one whole inner unroll
    (2, 96, 5, 8, 16, 16),     # three exact strips
    (1, 5, 64, 24, 40, 32),    # C / 4 and C / 8 channel groups with unequal strides
]


def _dw_run(D, x, w, b, K, ldx, ldy):
    n, H, W, Cc = x.shape
    xb, yb = Band(n * H * W, ldx), Band(n * H * W, ldy)
    xb.body[:, :Cc] = x.reshape(-1, Cc).to(DEV)
    D.dwconv_bf16(xb.body, ldx, w.to(DEV), b.to(DEV), yb.body, ldy, n, H, W, Cc, K)
    _sync()
    yb.check(Cc)
    return yb.body[:, :Cc].cpu().reshape(n, H, W, Cc)


def _dw_ref(x, w, b, k):
    Cc = x.shape[3]
    wt = w.double().t().reshape(Cc, 1, k, k)
    y = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), wt, b.double(), padding=k // 2, groups=Cc)
    return torch.nn.functional.silu(y).permute(0, 2, 3, 1)


@gpu
@pytest.mark.parametrize("n,H,W,Cc,ldx,ldy", DW_CASES)
def test_dwconv_vs_float64(D, n, H, W, Cc, ldx, ldy):
    """Unused input channels hold NaN, so a read past C shows.  Tolerance: test_conv_bf16_vs_torch's."""
    x = _randn((n, H, W, Cc), 1).to(BF)
    for k in (5, 3):
        w, b = _randn((k * k, Cc), 2, 1.0 / k), _randn((Cc,), 3, 0.1)
        ref = _dw_ref(x, w, b, k)
        tol = 2e-5 * float(ref.abs().max()) + 2.0 ** -8 * ref.abs()
        outs = {K: _dw_run(D, x, w, b, K, ldx, ldy) for K in ((5, 55) if k == 5 else (3,))}
        for K, out in outs.items():
            err = (out.double() - ref).abs()
            print(f"K={K} max err / tol {float((err / tol).max()):.3f}")
            assert bool((err <= tol).all()), (K, float(err.max()))
        if k == 5:  # the sliding-window kernel sums the same taps in the same order
            assert torch.equal(_bits(outs[5]), _bits(outs[55]))


# ------------------------------------------------------------------------------ SPP pools
def _spp_input(n, H, W, Cc, seed):
    x = _randn((n, H, W, Cc), seed)
    x[..., 0::8] = -x[..., 0::8].abs() - 0.5   # all-negative channels: a zero-initialised max would show
    x[..., 1::8] = -x[..., 1::8].abs() - 0.5
    x[:, 0] = -x[:, 0].abs() - 0.25            # and an all-negative first row in every channel
    return x.to(BF)


def _spp_run(D, x, ks, variant):
    n, H, W, Cc = x.shape
    ld = 4 * Cc + 8
    b = Band(n * H * W, ld)
    b.body[:, :Cc] = x.reshape(-1, Cc).to(DEV)
    D.spp_pool_bf16(b.body, ld, n, H, W, Cc, ks, variant)
    _sync()
    b.check(4 * Cc, keep=(Cc, _bits(x.reshape(-1, Cc))))
    return b.body[:, Cc:4 * Cc].cpu().reshape(n, H, W, 3, Cc)


def _spp_ref(x, ks):
    xf = x.float().permute(0, 3, 1, 2)
    return torch.stack([torch.nn.functional.max_pool2d(xf, k, 1, k // 2).permute(0, 2, 3, 1) for k in ks], 3).to(BF)


@gpu
@pytest.mark.parametrize("n,H,W,Cc,lds", [
    (2, 4, 3, 8, True),
    (1, 20, 20, 72, True),     # the LDS kernel's 400-position limit, a last slab of 8 channels
    (1, 12, 9, 64, True),
    (2, 1, 7, 16, True),
    (1, 21, 20, 16, False),    # 420 positions: the generic kernel, as for any detector input above 640
])
def test_spp_pools_exact(D, n, H, W, Cc, lds):
    from vge.lib import VgeError
    x = _spp_input(n, H, W, Cc, 5)
    ks = (5, 9, 13)
    ref = _bits(_spp_ref(x, ks))
    auto, generic = _bits(_spp_run(D, x, ks, 0)), _bits(_spp_run(D, x, ks, 1))
    assert torch.equal(generic, ref)
    assert torch.equal(auto, generic)
    if lds:
        assert torch.equal(_bits(_spp_run(D, x, ks, 2)), generic)
    else:
        with pytest.raises(VgeError, match="variant 2"):
            _spp_run(D, x, ks, 2)


@gpu
def test_spp_generic_other_pool_sizes(D):
    x = _spp_input(1, 6, 5, 8, 6)
    ref = _bits(_spp_ref(x, (3, 5, 7)))
    for variant in (0, 1):
        assert torch.equal(_bits(_spp_run(D, x, (3, 5, 7), variant)), ref)


# ------------------------------------------------------------------------------ channel attention
@gpu
@pytest.mark.parametrize("n,HW,Cc", [
    (2, 12, 48),       # a 6-lane slab: 42 pixel rows in flight, 4 idle threads
    (1, 108, 1024),    # four slabs, one chunk
    (2, 1300, 128),    # three chunks, a ragged last one
    (1, 513, 264),     # two chunks, a last slab of 8 channels
    (3, 1, 8),
])
def test_chan_attn_vs_float64(D, n, HW, Cc):
    """att within the worst-case bound of the kernel's sequential f32 sums (HW terms per mean, C per fc row):
    (HW + C) 2^-24 (sum_k |Wt[k][c]| mean_k|x| + |b_c|) / 6, + 1 f32 ulp of the result -- derived, not measured."""
    x = (_randn((n, HW, Cc), 7) + 0.3).to(BF)
    Wt, b = _randn((Cc, Cc), 8, Cc ** -0.5), _randn((Cc,), 9, 0.5)
    b[0], b[1] = 50.0, -50.0                   # both hardsigmoid clamps
    if Cc > 8:
        b[Cc - 1], b[Cc - 2] = -50.0, 50.0
    ld = Cc + 8
    xb, ab = Band(n * HW, ld), Band(n, Cc, torch.float32)
    xb.body[:, :Cc] = x.reshape(-1, Cc).to(DEV)
    mean = torch.empty(n * 2048, device=DEV)
    D.chan_attn_bf16(xb.body, ld, n, HW, Cc, Wt.to(DEV), b.to(DEV), mean, ab.body)
    _sync()
    xb.check(Cc)
    ab.check(Cc)
    att = ab.body.cpu()
    xd = x.double()
    z = xd.mean(1) @ Wt.double() + b.double()
    ref = (z + 3).clamp(0, 6) / 6
    assert float(ref[:, 0].min()) == 1.0 and float(ref[:, 1].max()) == 0.0
    mag = xd.abs().mean(1) @ Wt.double().abs() + b.double().abs()
    bound = (HW + Cc) * 2.0 ** -24 * mag / 6 + torch.from_numpy(np.spacing(ref.float().numpy())).double()
    ratio = float(((att.double() - ref).abs() / bound).max())
    print(f"att max err / bound {ratio:.4f}")
    assert ratio <= 1.0
    want = (x.float() * att[:, None, :]).to(BF)  # one f32 product, one rounding, from the att the kernel left
    assert torch.equal(_bits(xb.body[:, :Cc].cpu().reshape(n, HW, Cc)), _bits(want))


# ------------------------------------------------------------------------------ 2x upsample
@gpu
@pytest.mark.parametrize("n,H,W,Cc,ldx,ldy", [(2, 3, 5, 8, 16, 24), (1, 1, 1, 24, 32, 40)])
def test_upsample2x_exact(D, n, H, W, Cc, ldx, ldy):
    x = _randn((n, H, W, Cc), 10).to(BF)
    xb, yb = Band(n * H * W, ldx), Band(n * 4 * H * W, ldy)
    xb.body[:, :Cc] = x.reshape(-1, Cc).to(DEV)
    D.upsample2x_bf16(xb.body, ldx, yb.body, ldy, n, H, W, Cc)
    _sync()
    yb.check(Cc)
    want = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    assert torch.equal(_bits(yb.body[:, :Cc].cpu().reshape(n, 2 * H, 2 * W, Cc)), _bits(want))


# ------------------------------------------------------------------------------ warp (pose model input)
IN_H, IN_W = 64, 32


def _warp_boxes(H, W):
    """(name, box) for an H x W frame; model input 64 x 32, so a box of 25.6 x 51.2 has scale (32, 64): k = 1."""
    cx, cy = W // 2, H // 2
    return [
        ("inside", [W * 0.25, H * 0.2, W * 0.75, H * 0.8]),
        ("left border", [-W * 0.3, H * 0.2, W * 0.4, H * 0.7]),
        ("right border", [W * 0.6, H * 0.2, W * 1.4, H * 0.7]),
        ("top border", [W * 0.2, -H * 0.5, W * 0.8, H * 0.4]),
        ("bottom border", [W * 0.2, H * 0.6, W * 0.8, H * 1.7]),
        ("outside", [3.0 * W + 50, 3.0 * H + 50, 3.0 * W + 60, 3.0 * H + 70]),
        ("negative", [-40.7, -33.3, -1.2, -0.6]),
        ("whole frame", [0.0, 0.0, float(W), float(H)]),
        ("identity", [cx - 12.8, cy - 25.6, cx + 12.8, cy + 25.6]),
        ("zero width", [W * 0.5, H * 0.25, W * 0.5, H * 0.75]),
    ]


@gpu
@pytest.mark.parametrize("H,W", [(24, 40), (40, 24), (1, 1)])
def test_warp_prep_equals_oracle(D, H, W):
    """Every uint8 of the bilinear warp, through bf16: the kernel and oracle.dwpose.warp_input state the same float32
    operations.  Instances run over three frames out of frame order, two of them the same box on different frames."""
    from oracle.dwpose import MEAN_BGR, STD_BGR, warp_input
    from vge import synth
    frames = synth.make_frames(11, 3, H, W)
    names, boxes = zip(*_warp_boxes(H, W))
    frame_of = [(2 * i + 1) % 3 for i in range(len(boxes))] + [2, 2, 0]
    boxes = list(boxes) + [boxes[0], boxes[0], boxes[8]]
    names = list(names) + ["inside again", "inside twice", "identity on frame 0"]
    n = len(boxes)
    ob = Band(n * IN_H * IN_W, 8)
    D.warp_prep(torch.from_numpy(frames).to(DEV), np.array(boxes, np.float32), np.array(frame_of), IN_H, IN_W, ob.body)
    _sync()
    ob.check(8)
    out = ob.body.cpu().reshape(n, IN_H, IN_W, 8)
    assert bool((_bits(out[..., 3:]) == 0).all())
    mean, std = np.array(MEAN_BGR, np.float32), np.array(STD_BGR, np.float32)
    for i in range(n):
        ref = warp_input(frames[frame_of[i]], np.array(boxes[i], np.float32), IN_W, IN_H).transpose(1, 2, 0)
        got, want = _bits(out[i, ..., :3]), _bits(torch.from_numpy(np.ascontiguousarray(ref)).to(BF))
        assert torch.equal(got, want), (names[i], int((got != want).sum()))
        if names[i] == "outside":
            assert torch.equal(want, _bits(torch.from_numpy(np.broadcast_to((0 - mean) / std, ref.shape).copy()).to(BF)))
        if names[i].startswith("identity"):  # model pixel (v, u) is frame pixel (v - 32 + cy, u - 16 + cx), 0 outside
            pad = np.zeros((IN_H, IN_W, 3), np.float32)
            ys, xs = np.arange(IN_H) - IN_H // 2 + H // 2, np.arange(IN_W) - IN_W // 2 + W // 2
            oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
            pad[np.ix_(oky, okx)] = frames[frame_of[i]][np.ix_(ys[oky], xs[okx])][..., ::-1]
            assert torch.equal(got, _bits(torch.from_numpy((pad - mean) / std).to(BF))), names[i]
    if H > 1:
        assert not torch.equal(_bits(out[0]), _bits(out[n - 3]))  # the same box on another frame differs


# ------------------------------------------------------------------------------ letterbox + Focus (detector input)
def _letterbox_f64(frame, S):
    """onnxdet.preprocess in float64: cv2.resize(img, (int(W r), int(H r)), INTER_LINEAR) samples the source at
    (x + 0.5) * (W / rw) - 0.5, clamped to the image, into the top-left of a 114 canvas.  Unrounded values."""
    H, W = frame.shape[:2]
    r = min(S / H, S / W)
    rh, rw = int(H * r), int(W * r)
    img = frame[..., ::-1].astype(np.float64)

    def axis(n_out, n_in):
        s = np.clip((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0, n_in - 1)
        i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), s - i0

    x0, x1, fx = axis(rw, W)
    y0, y1, fy = axis(rh, H)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = (1 - fx) * img[y0][:, x0] + fx * img[y0][:, x1]
    bot = (1 - fx) * img[y1][:, x0] + fx * img[y1][:, x1]
    canvas = np.full((S, S, 3), 114.0)
    canvas[:rh, :rw] = (1 - fy) * top + fy * bot
    return canvas


def _focus_nhwc(canvas):
    return np.concatenate([canvas[0::2, 0::2], canvas[1::2, 0::2], canvas[0::2, 1::2], canvas[1::2, 1::2]], -1)


@gpu
@pytest.mark.parametrize("H,W,S", [
    (64, 64, 64),      # r = 1: the frame itself
    (48, 64, 64),      # padding rows
    (50, 30, 64),      # portrait: padding columns, an odd resized width (38)
    (20, 36, 64),      # upscale, r > 1
    (37, 53, 64),
    (1, 64, 64),
    (240, 320, 128),   # the detector test's frames
])
def test_letterbox_focus_equals_oracle(D, H, W, S):
    from oracle.yolox import letterbox_focus
    from vge import synth
    F = 3
    frames = synth.make_frames(13, F, H, W)
    S2 = S // 2
    ob = Band(F * S2 * S2, 16)
    D.letterbox_focus(torch.from_numpy(frames).to(DEV), S, ob.body)
    _sync()
    ob.check(16)
    out = ob.body.cpu().reshape(F, S2, S2, 16)
    assert bool((_bits(out[..., 12:]) == 0).all())
    got = out[..., :12].float().numpy()
    for f in range(F):
        np.testing.assert_array_equal(got[f], letterbox_focus(frames[f], S).transpose(1, 2, 0), err_msg=f"frame {f}")
        wide = _focus_nhwc(_letterbox_f64(frames[f], S))
        assert float(np.abs(got[f] - wide).max()) <= 1.0, f
        if (H, W) == (S, S):
            np.testing.assert_array_equal(got[f], _focus_nhwc(frames[f][..., ::-1].astype(np.float32)))
    assert not np.array_equal(got[0], got[1])


# ------------------------------------------------------------------------------ ScaleNorms
def _bf16_ulp(v):
    """spacing of bfloat16 (8 significand bits) at |v|, float64 array"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    return 2.0 ** (e - 7)


def _scalenorm64(x, g):
    """x float64 [..., n]: x / max(||x|| / sqrt(n), 1e-5) * g"""
    norm = np.sqrt((x * x).sum(-1, keepdims=True)) / math.sqrt(x.shape[-1])
    return x / np.maximum(norm, 1e-5) * g


@gpu
@pytest.mark.parametrize("inst,K,hw,Kp,ldy", [(2, 133, 12, 32, 136), (1, 133, 108, 128, 136), (1, 136, 256, 256, 136),
                                              (3, 133, 1, 32, 136)])
def test_head_scalenorm_t_vs_float64(D, inst, K, hw, Kp, ldy):
    g = 1.3
    y = torch.full((inst, hw, ldy), float("nan"))
    y[..., :K] = _randn((inst, hw, K), 14, 0.7)
    y[0, :, 3] = 0.0                         # the clamp with a zero row: zeros, not NaN
    y[inst - 1, :, 7] = 1e-7 * (1 + torch.arange(hw) % 3) * (1 - 2 * (torch.arange(hw) % 2))  # and a non-zero row
    rows = inst * K
    yb, ob = Band(inst * hw, ldy, torch.float32), Band(rows, Kp)   # NaN rows behind the last instance's positions
    yb.body[:] = y.reshape(-1, ldy).to(DEV)
    D.head_scalenorm_t(yb.body, ldy, hw, K, Kp, g, rows, ob.body)
    _sync()
    ob.check(Kp)
    out = ob.body.cpu().reshape(inst, K, Kp)
    assert bool((_bits(out[..., hw:]) == 0).all())
    assert bool((_bits(out[0, 3]) == 0).all())
    x = y[..., :K].double().numpy().transpose(0, 2, 1)      # [inst, K, hw]
    ref = _scalenorm64(x, g)
    small = ref[inst - 1, 7]
    np.testing.assert_allclose(small, x[inst - 1, 7] / 1e-5 * g, rtol=1e-12)  # premise: the clamp is what divides
    assert np.abs(small).max() > 1e-3
    err = np.abs(out[..., :hw].double().numpy() - ref)
    print(f"max err / ulp {float((err / _bf16_ulp(ref)).max()):.3f}")
    assert (err <= _bf16_ulp(ref)).all()


@gpu
@pytest.mark.parametrize("Dm", [8, 64, 256, 512])
@pytest.mark.parametrize("rows", [1, 5, 266])
def test_scalenorm_rows_vs_float64(D, Dm, rows):
    g = 0.8
    x = _randn((rows, Dm), 16, 2.0)
    x[0] *= 1e-8                              # the clamp
    ob = Band(rows, Dm)
    D.scalenorm_rows(x.to(DEV), Dm, g, rows, ob.body)
    _sync()
    ob.check(Dm)
    ref = _scalenorm64(x.double().numpy(), g)
    err = np.abs(ob.body.cpu().double().numpy() - ref)
    assert (err <= _bf16_ulp(ref)).all(), float((err / _bf16_ulp(ref)).max())


# ------------------------------------------------------------------------------ GAU token mixing
def _gau_lines(uv, gamma, beta, E, S):
    """OracleRtmpose.head's q / k / kernel / u * (kernel @ v) lines in uv's dtype"""
    u, v, base = uv[..., :E], uv[..., E:2 * E], uv[..., 2 * E:]
    base = base.unsqueeze(2) * gamma[None, None] + beta
    q, k = base[:, :, 0], base[:, :, 1]
    kern = torch.square(torch.relu((q @ k.transpose(1, 2)) / math.sqrt(S)))
    return u * (kern @ v)


@gpu
@pytest.mark.parametrize("n,K,E,S", [
    (3, 133, 512, 128),    # the published model's shape
    (1, 136, 128, 8),
    (2, 135, 256, 152),    # the largest S the VALU kernel holds
    (1, 133, 128, 64),
    (2, 136, 128, 160),    # the largest S create accepts: the MFMA kernel alone holds it
])
def test_gau_attn_vs_float64(D, n, K, E, S):
    """Tolerance per element: 4 x (the max error of the same lines in torch float32 on the CPU, relative to the
    output scale) x scale + 1 bf16 ulp of the reference.  Yardsticks measured on the cases above, in order: 4.7e-7,
    2.9e-7, 5.7e-7, 4.0e-7, 4.0e-7; both kernels' max error is 0.50 of the tolerance (the bf16 output rounding).
    Pad tokens K..159 of the MFMA tiles are the next instance's rows (n > 1) and must read as zero."""
    from vge.lib import VgeError
    uv = torch.nn.functional.silu(_randn((n, K, 2 * E + S), 17, 0.6))
    gamma, beta = _randn((2, S), 18), _randn((2, S), 19, 0.1)
    ref = _gau_lines(uv.double(), gamma.double(), beta.double(), E, S)
    scale = float(ref.abs().max())
    yard = float((_gau_lines(uv, gamma, beta, E, S).double() - ref).abs().max()) / scale
    tol = 4 * yard * scale + torch.from_numpy(_bf16_ulp(ref.numpy()))
    outs = {}
    for variant, nbytes in zip((1, 2), gau_lds_bytes(K, S)):
        ob = Band(n * K, E)
        args = (uv.reshape(n * K, -1).to(DEV), n, K, E, S, gamma.to(DEV), beta.to(DEV), ob.body, variant)
        if nbytes > GAU_LDS_LIMIT:
            with pytest.raises(VgeError, match="LDS"):
                D.gau_attn(*args)
            continue
        D.gau_attn(*args)
        _sync()
        ob.check(E)
        outs[variant] = ob.body.cpu().double().reshape(n, K, E)
        err = (outs[variant] - ref).abs()
        print(f"variant {variant}: scale {scale:.3g}, f32 yardstick {yard:.3g}, max err / scale "
              f"{float(err.max()) / scale:.3g}, max err / tol {float((err / tol).max()):.3f}")
        assert bool((err <= tol).all()), (variant, float((err / tol).max()))
    assert 2 in outs
    if 1 in outs:
        assert bool(((outs[1] - outs[2]).abs() <= tol).all())
    ob = Band(n * K, E)                       # what the model calls: one of the two, whichever it is
    D.gau_attn(uv.reshape(n * K, -1).to(DEV), n, K, E, S, gamma.to(DEV), beta.to(DEV), ob.body, 0)
    _sync()
    auto = ob.body.cpu().double().reshape(n, K, E)
    assert any(torch.equal(auto, o) for o in outs.values())


# ------------------------------------------------------------------------------ SimCC decode
def _simcc_rows(WX, WY, rows, ld, seed):
    rng = np.random.default_rng(seed)
    lg = np.full((rows, ld), 1e9, np.float32)              # columns past the bins would win if read
    lg[:, :WX + WY] = rng.uniform(-1.0, 0.9, (rows, WX + WY)).astype(np.float32)
    x, y = lg[:, :WX], lg[:, WX:WX + WY]

    def peaks(a, r, bins, v):
        a[r, [min(b, a.shape[1] - 1) for b in bins]] = v

    for r in range(rows):
        p = r % 9
        if p == 0:
            peaks(x, r, [0], 1.5), peaks(y, r, [WY - 1], 1.25)
        elif p == 1:
            peaks(x, r, [5, 69], 1.5), peaks(y, r, [63, 64], 1.75)       # same lane 64 apart; neighbouring lanes
        elif p == 2:
            peaks(x, r, [0, WX - 1], 2.0)
            y[r] = 0.625                                                  # every bin equal
        elif p == 3:
            x[r] = np.minimum(x[r], -0.1)
            peaks(x, r, [7], 0.0), peaks(y, r, [1], 0.5)                 # val exactly 0 -> -1
        elif p == 4:
            peaks(x, r, [WX // 2], 3.0), peaks(y, r, [2], 1.0)           # x max above y max
        elif p == 5:
            peaks(x, r, [WX - 1], 1.0), peaks(y, r, [0], 3.0)            # and the reverse
        elif p == 6:
            x[r] = -np.abs(x[r]) - 0.01                                   # all negative
            y[r] = -np.abs(y[r]) - 0.01
        elif p == 7:
            x[r] = 1.0                                                    # every bin equal, both axes
            y[r] = 1.0
    return lg


@gpu
@pytest.mark.parametrize("WX,WY,split", [(192, 256, 2.0), (576, 768, 2.0), (70, 3, 3.0)])
@pytest.mark.parametrize("rows", [1, 6, 133 * 3])
def test_simcc_decode_exact(D, WX, WY, split, rows):
    ld = WX + WY + 5
    lg = _simcc_rows(WX, WY, rows, ld, 20)
    ob = Band(rows, 3, torch.float32)
    D.simcc_decode(torch.from_numpy(lg).to(DEV), ld, WX, WY, split, rows, ob.body)
    _sync()
    ob.check(3)
    x, y = lg[:, :WX], lg[:, WX:WX + WY]
    vals = np.minimum(x.max(1), y.max(1))
    locs = np.stack([x.argmax(1), y.argmax(1)], 1).astype(np.float32)    # numpy: the first index of the maximum
    locs[vals <= 0] = -1
    want = np.concatenate([locs / np.float32(split), vals[:, None]], 1)
    if rows >= 6:
        assert want[3, 2] == 0.0 and want[3, 0] < 0 and want[1, 0] * split == 5 and want[2, 0] == 0
    np.testing.assert_array_equal(ob.body.cpu().numpy(), want)


# ------------------------------------------------------------------------------ YOLOX decode + two-person NMS
GRIDS, STRIDES = (16, 8, 4), (8, 16, 32)
A0, A1, A2 = 256, 64, 16
N_ANCH = A0 + A1 + A2
HI = 20.0        # sigmoid(20) == 1 in float32, so an anchor's score is sigmoid(obj logit)


def _logit(p):
    return math.log(p / (1 - p))


class _Heads:
    """Head outputs of one frame: every anchor far below the score threshold until set()."""

    def __init__(self, ratio, seed):
        rng = np.random.default_rng(seed)
        self.ratio = ratio
        self.o = [np.concatenate([rng.uniform(-0.5, 1.5, (g * g, 2)), rng.uniform(-1, 1, (g * g, 2)),
                                  np.full((g * g, 2), -10.0), np.zeros((g * g, 2))], 1).astype(np.float32) for g in GRIDS]

    def set(self, a, box, score):
        """anchor index a (level-major) gets the frame-pixel box (x0, y0, x1, y1) and the score"""
        lvl = 0 if a < A0 else 1 if a < A0 + A1 else 2
        i = a - (0, A0, A0 + A1)[lvl]
        g, st = GRIDS[lvl], STRIDES[lvl]
        x0, y0, x1, y1 = (v * self.ratio for v in box)
        self.o[lvl][i] = [(x0 + x1) / 2 / st - i % g, (y0 + y1) / 2 / st - i // g, math.log((x1 - x0) / st),
                          math.log((y1 - y0) / st), _logit(score), HI, 0, 0]
        return self


def _yolox_cases(ratio):
    """(name, heads, premise(kept boxes, n, cand) asserted on the oracle's result)"""
    far = lambda k: [200.0 + 60 * k, 30.0, 240.0 + 60 * k, 90.0]   # boxes that overlap nothing else
    base = [20.0, 20.0, 80.0, 80.0]
    near = lambda d: [20.0 + d, 20.0, 80.0 + d, 80.0]
    box41 = [10.0, 10.0, 50.0, 50.0]   # 41 x 41 with the + 1: shifted by d, IoU = (41 - d) / (41 + d) at ratio 1
    is_ = lambda cand, kept, p, a: np.array_equal(kept[p], cand[a, :4])
    H = lambda s: _Heads(ratio, s)
    return [
        ("a none above 0.3", H(1).set(9, base, 0.29).set(300, far(0), 0.2),
         lambda k, n, c: n == 0 and c[9, 4] > 0.28),
        ("b one above", H(2).set(77, base, 0.6).set(3, far(0), 0.29),
         lambda k, n, c: n == 1 and is_(c, k, 0, 77)),
        ("c second suppressed, third kept", H(3).set(40, base, 0.9).set(41, near(6), 0.8).set(270, far(1), 0.7),
         lambda k, n, c: n == 2 and is_(c, k, 0, 40) and is_(c, k, 1, 270)),
        ("d all others suppressed", H(4).set(130, base, 0.9).set(2, near(4), 0.8).set(258, near(-5), 0.7)
         .set(330, near(9), 0.6), lambda k, n, c: n == 1 and is_(c, k, 0, 130)),
        ("e tie 64 apart", H(5).set(74, base, 0.8).set(10, near(7), 0.8),
         lambda k, n, c: n == 1 and c[10, 4] == c[74, 4] and is_(c, k, 0, 10)),
        ("e tie 1 apart, second pass", H(6).set(200, far(2), 0.9).set(91, base, 0.7).set(90, far(0), 0.7),
         lambda k, n, c: n == 2 and c[90, 4] == c[91, 4] and is_(c, k, 0, 200) and is_(c, k, 1, 90)),
        ("e tie across levels, one thread", H(7).set(261, base, 0.8).set(5, near(7), 0.8),
         lambda k, n, c: n == 1 and c[5, 4] == c[261, 4] and is_(c, k, 0, 5)),
        ("e tie across levels", H(8).set(325, far(1), 0.75).set(200, far(0), 0.75).set(300, base, 0.75),
         lambda k, n, c: n == 2 and c[200, 4] == c[300, 4] == c[325, 4] and is_(c, k, 0, 200) and is_(c, k, 1, 300)),
        ("f IoU under 0.45", H(9).set(50, box41, 0.9).set(51, [v + (15.7 if j % 2 == 0 else 0) for j, v in enumerate(box41)], 0.8),
         lambda k, n, c: n == 2 and is_(c, k, 1, 51)),
        ("f IoU over 0.45", H(10).set(50, box41, 0.9).set(51, [v + (15.4 if j % 2 == 0 else 0) for j, v in enumerate(box41)], 0.8),
         lambda k, n, c: n == 1),
    ]


def _decode64(o, lvl, ratio):
    """demo_postprocess + xyxy / ratio + score in float64 -> (corners, magnitude of each corner's operands, score)"""
    g, st = GRIDS[lvl], STRIDES[lvl]
    o = o.astype(np.float64)
    gy, gx = np.divmod(np.arange(g * g), g)
    cx, cy = (o[:, 0] + gx) * st, (o[:, 1] + gy) * st
    w, h = np.exp(o[:, 2]) * st, np.exp(o[:, 3]) * st
    box = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1) / ratio
    mag = np.stack([np.abs(cx) + w / 2, np.abs(cy) + h / 2] * 2, 1) / ratio
    sig = lambda v: 1 / (1 + np.exp(-v))
    return box, mag, sig(o[:, 4]) * sig(o[:, 5])


@gpu
@pytest.mark.parametrize("ratio", [1.0, 0.4, 2.5])
def test_yolox_decode_nms_crafted(D, ratio):
    """One launch, one crafted frame per case; the ratio scales the head outputs so every case keeps its geometry in
    frame pixels.  cand vs a float64 decode (4 f32 ulp of the operands' magnitude); boxes / n / scores exactly the
    oracle's greedy NMS of the kernel's own cand, each case's premise asserted on that result first."""
    from oracle.yolox import iou_plus1, two_persons
    ratio = float(np.float32(ratio))
    cases = _yolox_cases(ratio)
    F = len(cases)
    outs = [torch.from_numpy(np.stack([h.o[l] for _, h, _ in cases])).to(DEV) for l in range(3)]
    bb, nb = Band(F, 8, torch.float32), Band(F, 1, torch.int32)
    sb, cb = Band(F, 2, torch.float32), Band(F * N_ANCH, 5, torch.float32)
    D.yolox_decode_nms(outs, GRIDS, STRIDES, F, ratio, bb.body, nb.body, sb.body, cb.body)
    _sync()
    for b, cols in ((bb, 8), (nb, 1), (sb, 2), (cb, 5)):
        b.check(cols)
    boxes, npers = bb.body.cpu().numpy().reshape(F, 2, 4), nb.body.cpu().numpy().reshape(F)
    scores, cand = sb.body.cpu().numpy(), cb.body.cpu().numpy().reshape(F, N_ANCH, 5)
    for f, (name, heads, premise) in enumerate(cases):
        ref = [_decode64(heads.o[l], l, ratio) for l in range(3)]
        box, mag, sc = (np.concatenate([r[j] for r in ref]) for j in range(3))
        assert (np.abs(cand[f, :, :4] - box) <= 4 * np.spacing(mag.astype(np.float32))).all(), name
        assert (np.abs(cand[f, :, 4] - sc) <= 4 * np.spacing(sc.astype(np.float32))).all(), name
        kept, n = two_persons(cand[f, :, :4], cand[f, :, 4])
        assert premise(kept, n, cand[f]), f"premise of case {name!r} does not hold"
        if name.startswith("f IoU"):
            iou = float(iou_plus1(cand[f, 50, :4], cand[f, 51, :4]))
            assert abs(iou - 0.45) > 1e-4 and (iou < 0.45) == ("under" in name), (name, iou)
        assert int(npers[f]) == n, name
        np.testing.assert_array_equal(boxes[f, :n], kept, err_msg=name)
        assert (boxes[f, n:] == 0).all() and (scores[f, n:] == 0).all(), name
        for p in range(n):
            a = int(np.flatnonzero((cand[f, :, :4] == kept[p]).all(1))[0])
            assert scores[f, p] == cand[f, a, 4], name
    b2, n2 = Band(F, 8, torch.float32), Band(F, 1, torch.int32)          # scores = NULL, cand = NULL
    D.yolox_decode_nms(outs, GRIDS, STRIDES, F, ratio, b2.body, n2.body)
    _sync()
    b2.check(8), n2.check(1)
    assert torch.equal(b2.bits(), bb.bits()) and torch.equal(n2.bits(), nb.bits())
