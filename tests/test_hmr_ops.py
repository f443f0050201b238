"""The mesh extractor's kernels around its GEMMs (vge_vit.hip), op by op through the vge_op_* entry points of
include/vge_hmr.h, each against a plain high-precision reference of the same operation:

  patchify              bit-exact: every (u - mean) / std lies >= 8.5 float32 ulps from a bf16 rounding tie (asserted
                        here on the CPU), so the bf16 value table of 256 x 3 entries is unambiguous
  ViT attention         float64 softmax(Q K^T / sqrt(hd)) V of the bf16 inputs; per element
                        2^-8 (sum_k a_k |v_k| + |ref|) + 20 e_ref: the kernel rounds P and the output to bf16
  one-query attention   float64; 2^-8 |ref| + 20 e_ref (one bf16 rounding, of the output)
  softmax rows          float64; 2^-8 |ref| + 20 e_ref, row sums within 2^-8 of 1
  readout               float64 Gram-Schmidt; per joint 16 * 2^-24 (1 + |a2| / |u|), u = a2's part orthogonal to a1
                        (a float32 restatement reaches 5.3 of those units over 200,000 vectors); betas exact
  cast / bcast / copy   bit-exact

e_ref = max |the same lines in torch float32 on the CPU, no bf16 rounding - float64|, the yardstick of
tests/test_encoder_shapes.py.  Outputs sit in buffers of a NaN bit pattern wider and longer than what the kernel may
write; everything beyond must come back untouched.  Unused input columns hold NaN, so reading them shows.
"""
import math

import numpy as np
import pytest
import torch

DEV = "cuda:0"
gpu = pytest.mark.gpu
BF = torch.bfloat16
U8 = 2.0 ** -8                  # bf16 unit roundoff
SENT16 = 0x7FC1                 # a bf16 quiet NaN
SENT32 = 0x7FC12345             # an f32 quiet NaN
IMG_MEAN = (123.675, 116.28, 103.53)
IMG_STD = (58.395, 57.12, 57.375)


# ------------------------------------------------------------------------------ CPU: refusals, no GPU work
def _lib():
    from vge import hmr as H
    from vge import lib as L
    return H._sig(L.load())


# entry -> (what is refused, the arguments); every pointer is null, so a launch would fault: none happens
_N = None
REFUSALS = [
    ("vge_op_patchify", "null pointers", (_N, 1, 256, 256, 256, 192, 16, 2, _N, _N)),
    ("vge_op_patchify", "F 0", (_N, 0, 256, 256, 256, 192, 16, 2, _N, _N)),
    ("vge_op_patchify", "img_h != in_h", (_N, 1, 256, 256, 252, 192, 16, 2, _N, _N)),
    ("vge_op_patchify", "odd margin", (_N, 1, 256, 257, 256, 192, 16, 2, _N, _N)),
    ("vge_op_patchify", "img_w > in_w", (_N, 1, 256, 180, 256, 192, 16, 2, _N, _N)),
    ("vge_op_patchify", "patch 8", (_N, 1, 256, 256, 256, 192, 8, 2, _N, _N)),
    ("vge_op_patchify", "17 patch rows", (_N, 1, 272, 256, 272, 192, 16, 2, _N, _N)),
    ("vge_op_patchify", "13 patch columns", (_N, 1, 256, 256, 256, 208, 16, 0, _N, _N)),
    ("vge_op_patchify", "11 patch columns", (_N, 1, 256, 256, 256, 186, 16, 2, _N, _N)),
    ("vge_op_xattn1", "null pointers", (_N, 256, _N, 512, _N, 256, 1, 4, 192, _N)),
    ("vge_op_xattn1", "ctx 0", (_N, 256, _N, 512, _N, 256, 1, 4, 0, _N)),
    ("vge_op_xattn1", "ctx 257", (_N, 256, _N, 512, _N, 256, 1, 4, 257, _N)),
    ("vge_op_xattn1", "ldq % 8", (_N, 260, _N, 512, _N, 256, 1, 4, 192, _N)),
    ("vge_op_xattn1", "ldkv % 8", (_N, 256, _N, 516, _N, 256, 1, 4, 192, _N)),
    ("vge_op_xattn1", "ldo % 8", (_N, 256, _N, 512, _N, 260, 1, 4, 192, _N)),
    ("vge_op_xattn1", "ldq < 64 heads", (_N, 248, _N, 512, _N, 256, 1, 4, 192, _N)),
    ("vge_op_xattn1", "ldkv < 128 heads", (_N, 256, _N, 504, _N, 256, 1, 4, 192, _N)),
    ("vge_op_xattn1", "ldo < 64 heads", (_N, 256, _N, 512, _N, 248, 1, 4, 192, _N)),
    ("vge_op_xattn1", "F 0", (_N, 256, _N, 512, _N, 256, 0, 4, 192, _N)),
    ("vge_op_xattn1", "heads 0", (_N, 256, _N, 512, _N, 256, 1, 0, 192, _N)),
    ("vge_op_softmax_rows_bf16", "null pointers", (_N, _N, 4, 256, _N)),
    ("vge_op_softmax_rows_bf16", "rows 0", (_N, _N, 0, 256, _N)),
    ("vge_op_softmax_rows_bf16", "C 0", (_N, _N, 4, 0, _N)),
    ("vge_op_hmr_readout", "null pointers", (_N, 256, _N, 256, _N, _N, _N, _N, _N, 1, _N)),
    ("vge_op_hmr_readout", "F 0", (_N, 256, _N, 256, _N, _N, _N, _N, _N, 0, _N)),
    ("vge_op_hmr_readout", "ldrd < 31", (_N, 30, _N, 256, _N, _N, _N, _N, _N, 1, _N)),
    ("vge_op_hmr_readout", "ldbp < 126", (_N, 256, _N, 125, _N, _N, _N, _N, _N, 1, _N)),
    ("vge_op_cast_rows_bf16", "null pointers", (_N, 16, _N, 16, 1, 8, _N)),
    ("vge_op_cast_rows_bf16", "D % 4", (_N, 16, _N, 16, 1, 6, _N)),
    ("vge_op_cast_rows_bf16", "ldx < D", (_N, 4, _N, 16, 1, 8, _N)),
    ("vge_op_cast_rows_bf16", "ldy < D", (_N, 16, _N, 4, 1, 8, _N)),
    ("vge_op_cast_rows_bf16", "ldx % 4", (_N, 18, _N, 16, 1, 8, _N)),
    ("vge_op_cast_rows_bf16", "ldy % 4", (_N, 16, _N, 18, 1, 8, _N)),
    ("vge_op_cast_rows_bf16", "rows 0", (_N, 16, _N, 16, 0, 8, _N)),
    ("vge_op_bcast_rows", "null pointers", (_N, _N, 1, 8, _N)),
    ("vge_op_bcast_rows", "rows 0", (_N, _N, 0, 8, _N)),
    ("vge_op_bcast_rows", "D 0", (_N, _N, 1, 0, _N)),
    ("vge_op_copy_rows", "null pointers", (_N, 16, _N, 16, 1, 8, _N)),
    ("vge_op_copy_rows", "ldx < D", (_N, 7, _N, 16, 1, 8, _N)),
    ("vge_op_copy_rows", "ldy < D", (_N, 16, _N, 7, 1, 8, _N)),
    ("vge_op_copy_rows", "rows 0", (_N, 16, _N, 16, 0, 8, _N)),
]


@pytest.mark.parametrize("entry,what,args", REFUSALS, ids=[f"{e[7:]}-{w}" for e, w, _ in REFUSALS])
def test_op_entry_refuses(entry, what, args):
    lib = _lib()
    assert getattr(lib, entry)(*args) == 1, what
    assert entry.encode() in lib.vge_last_error(), lib.vge_last_error()


_SMALL = dict(embed_dim=256, depth=1, heads=4, mlp_dim=256, dec_dim=256, dec_depth=1, dec_heads=4, dec_mlp=256,
              tok_num=1, tok_classes=256, tok_code_dim=256)
# one config per clause of vge_hmr_create's rule (cfg_ok in vge_hmr.cpp), each a one-field change of an accepted one
BAD_CONFIGS = [
    dict(img_h=252), dict(in_w=257), dict(in_w=180), dict(img_w=0), dict(patch=8), dict(pad=8), dict(img_w=208, pad=0),
    dict(embed_dim=1000), dict(embed_dim=1536, heads=24), dict(embed_dim=0), dict(embed_dim=512, heads=4),
    dict(heads=0), dict(heads=3), dict(mlp_dim=1000), dict(mlp_dim=0), dict(depth=-1),
    dict(dec_dim=300), dict(dec_dim=0), dict(dec_dim=1536), dict(dec_dim_head=32), dict(dec_heads=6),
    dict(dec_heads=0), dict(dec_mlp=100), dict(dec_mlp=0), dict(dec_depth=-1),
    dict(tok_num=0), dict(tok_classes=100), dict(tok_classes=0), dict(tok_code_dim=128), dict(tok_code_dim=0),
]


@pytest.mark.parametrize("change", BAD_CONFIGS, ids=["-".join(f"{k}={v}" for k, v in c.items()) for c in BAD_CONFIGS])
def test_create_refuses_config(change):
    import ctypes as C
    from vge import hmr as H
    lib = _lib()
    out = C.c_void_p()
    ok = H._cfg_c(H.HmrConfig(**_SMALL))
    assert lib.vge_hmr_create(C.byref(ok), None, 0, C.byref(out)) != 1  # the unchanged one is no argument error
    bad = H._cfg_c(H.HmrConfig(**{**_SMALL, **change}))
    assert lib.vge_hmr_create(C.byref(bad), None, 0, C.byref(out)) == 1
    assert b"vge_hmr_create: unsupported config" in lib.vge_last_error()
    assert not out.value


def _patch_table64():
    """(u - mean) / std in float64, of the float32 constants the kernel holds: [3][256]."""
    u = np.arange(256, dtype=np.float64)
    return np.stack([(u - float(np.float32(m))) / float(np.float32(s)) for m, s in zip(IMG_MEAN, IMG_STD)])


def test_patchify_table_is_far_from_bf16_ties():
    """The premise of the bit-exact patchify test: in units of the float32 ulp of each table value, the distance to the
    nearest bf16 rounding tie (float32 low half 0x8000) is >= 8.5, far beyond the error of a float32 subtract and
    divide, correctly rounded (1 ulp) or not (2.5); and neighbouring pixel values give different bf16 values."""
    t = np.abs(_patch_table64())
    e = np.floor(np.log2(t))
    frac = np.mod(t / 2.0 ** (e - 23), 65536.0)
    dist = np.abs(frac - 32768.0)
    assert dist.min() >= 8.5, dist.min()
    tb = torch.from_numpy(_patch_table64()).float().to(BF).view(torch.int16).numpy()
    assert all(len(set(tb[c].tolist())) == 256 for c in range(3))


# ------------------------------------------------------------------------------ GPU helpers
@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vge import hmr
    return hmr


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class Buf:
    """[rows + spare][ld] elements of bf16 / f32 filled with a NaN bit pattern; `t` is the typed tensor the kernel is
    given.  check(rows, cols) asserts that everything outside [:rows, :cols] still holds the pattern."""

    def __init__(self, rows, ld, dtype, spare=3):
        self.two = dtype == BF
        self.raw = torch.full((rows + spare, ld), SENT16 if self.two else SENT32,
                              dtype=torch.int16 if self.two else torch.int32, device=DEV)
        self.t = self.raw.view(dtype)

    def check(self, rows, cols):
        raw = self.raw.cpu()
        sent = SENT16 if self.two else SENT32
        assert bool((raw[rows:] == sent).all()), "rows behind the last one were written"
        assert bool((raw[:rows, cols:] == sent).all()), "columns beyond the width were written"
        return self.t[:rows, :cols].cpu()


def _with_nan_cols(x, ld):
    """x [rows, n] -> [rows, ld] with NaN in the columns from n on (input columns a kernel must not read)."""
    out = torch.full((x.shape[0], ld), float("nan"), dtype=x.dtype)
    out[:, :x.shape[1]] = x
    return out


def _report(tag, err, bound):
    """worst error / bound over the elements, printed (pytest -s) before the assertion"""
    ratio = float((err / bound).max())
    print(f"{tag}: worst error / bound {ratio:.3f} (max error {float(err.max()):.3e})")
    return ratio


# ------------------------------------------------------------------------------ patchify
V0 = 77  # the pixel value kept out of the part of a frame the patch grid reads, when there is another part

PATCH_GEOMS = {  # in_h (= img_h), in_w, img_w, pad
    "default": (256, 256, 192, 2),
    "pad0": (256, 256, 192, 0),
    "x0=0": (256, 192, 192, 2),
    "x0=0-pad0": (256, 192, 192, 0),
    "rows-and-columns-dropped": (260, 208, 200, 2),
}


def _patch_frames(F, in_h, in_w, img_w, pad, seed):
    """uint8 frames whose patch-grid-visible pixels -- rows [0, min(in_h, 256 - pad)), columns x0 + [0, min(img_w,
    192 - pad)) -- hold every value in every channel, except V0 when the frame has pixels the grid must not read (the
    margins left and right of the crop, rows and columns past the grid): those hold V0 and nothing else."""
    rng = np.random.default_rng(seed)
    x0 = (in_w - img_w) // 2
    vh, vw = min(in_h, 256 - pad), min(img_w, 192 - pad)
    hidden = vh < in_h or vw < in_w
    vals = np.array([v for v in range(256) if not (hidden and v == V0)], np.uint8)
    fr = np.full((F, in_h, in_w, 3), V0, np.uint8)
    vis = vals[rng.integers(0, len(vals), size=(F, vh, vw, 3))]
    vis.reshape(F, -1, 3)[:, :len(vals)] = vals[:, None]   # every value, in every channel, from the first pixel on
    k = min(vh, len(vals))
    vis[:, :k, 0, :] = vals[::-1][:k, None]                # ... and down the first column, next to the padded border
    assert vis.flags["C_CONTIGUOUS"]
    fr[:, :vh, x0:x0 + vw] = vis
    return fr, hidden


def _patch_ref(fr, img_w, pad):
    """-> (bf16 bits [F * 192, 768], mask of the elements that lie in the zero padding)"""
    F, in_h, in_w, _ = fr.shape
    x0 = (in_w - img_w) // 2
    tab = torch.from_numpy(_patch_table64()).float().to(BF).view(torch.int16).numpy()   # [3][256] bf16 bits
    crop = fr[:, :, x0:x0 + img_w].astype(np.int64)
    val = np.stack([tab[c][crop[..., c]] for c in range(3)], 1)                        # [F, 3, in_h, img_w]
    Hc, Wc = max(in_h + 2 * pad, 256), max(img_w + 2 * pad, 192)
    canvas = np.zeros((F, 3, Hc, Wc), np.int16)
    inside = np.zeros((Hc, Wc), bool)
    canvas[:, :, pad:pad + in_h, pad:pad + img_w] = val
    inside[pad:pad + in_h, pad:pad + img_w] = True
    rows = canvas[:, :, :256, :192].reshape(F, 3, 16, 16, 12, 16).transpose(0, 2, 4, 1, 3, 5).reshape(F * 192, 768)
    zero = ~np.broadcast_to(inside[:256, :192], (F, 3, 256, 192))
    zero = zero.reshape(F, 3, 16, 16, 12, 16).transpose(0, 2, 4, 1, 3, 5).reshape(F * 192, 768)
    return rows, zero


@gpu
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("geom", list(PATCH_GEOMS))
def test_patchify_bit_exact(H, geom, F):
    in_h, in_w, img_w, pad = PATCH_GEOMS[geom]
    fr, hidden = _patch_frames(F, in_h, in_w, img_w, pad, seed=100 + F)
    assert hidden == (geom not in ("x0=0-pad0",))
    x0 = (in_w - img_w) // 2
    vis = fr[:, :min(in_h, 256 - pad), x0:x0 + min(img_w, 192 - pad)]
    for c in range(3):  # the premise: every value (but V0) where the grid reads, V0 nowhere there
        assert len(np.unique(vis[..., c])) == (255 if hidden else 256)
        assert hidden == (V0 not in vis[..., c])
    want, zero = _patch_ref(fr, img_w, pad)
    assert zero.any() == (pad > 0)
    buf = Buf(F * 192, 768, BF)
    H.patchify(torch.from_numpy(fr).to(DEV), buf.t, img_w=img_w, pad=pad)
    got = buf.check(F * 192, 768).view(torch.int16).numpy()
    assert (got[zero] == 0).all(), "the conv's zero padding must be +0 exactly"
    if hidden:  # pixels outside the crop, or past the grid, never appear
        tab = torch.from_numpy(_patch_table64()).float().to(BF).view(torch.int16).numpy()
        for c in range(3):
            assert not (got[:, 256 * c:256 * (c + 1)] == tab[c][V0]).any(), f"a hidden pixel shows in channel {c}"
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist())


# ------------------------------------------------------------------------------ ViT self-attention
ATTN_SHAPES = [(256, 4), (512, 8), (768, 12), (1024, 16), (1280, 16), (1280, 20)]


def _attn_check(H, qkv, F, D, heads, tag):
    hd = D // heads
    out = Buf(F * 192, D, BF)
    H.vit_attention(qkv.to(DEV), heads, out=out.t)
    got = out.check(F * 192, D).double()

    def parts(t):
        q, k, v = t.view(F, 192, 3, heads, hd).permute(2, 0, 3, 1, 4)
        a = torch.softmax((q @ k.transpose(-2, -1)) / math.sqrt(hd), -1)
        return a, v

    def rows(t):
        return t.transpose(1, 2).reshape(F * 192, D)

    a, v = parts(qkv.double())
    ref, mag = rows(a @ v), rows(a @ v.abs())
    a32, v32 = parts(qkv.float())
    e_ref = float((rows(a32 @ v32).double() - ref).abs().max())
    bound = U8 * (mag + ref.abs()) + 20 * e_ref
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    _report(f"vit_attention {tag} (e_ref {e_ref:.2e})", err, bound)
    assert bool((err <= bound).all()), float((err / bound).max())
    return a


@gpu
@pytest.mark.parametrize("scale", [0.05, 1.5, 4.0])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("D,heads", ATTN_SHAPES)
def test_vit_attention_vs_float64(H, D, heads, F, scale):
    """0.05: near-uniform rows; 1.5: ordinary; 4.0: near-one-hot (logits of standard deviation 16 sqrt(hd))."""
    qkv = (torch.randn((F * 192, 3 * D), generator=_gen(7 + D + heads + F)) * scale).to(BF)
    a = _attn_check(H, qkv, F, D, heads, f"D {D} heads {heads} F {F} scale {scale}")
    if scale == 1.5:  # the absolute bars this test's predecessor (test_hmr.py::test_vit_attention) held at this scale
        hd = D // heads
        got = H.vit_attention(qkv.to(DEV), heads).float().cpu()
        q, k, v = qkv.float().view(F, 192, 3, heads, hd).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-2, -1)) / hd ** 0.5
        e = torch.exp(s - s.amax(-1, keepdim=True))
        stored = ((e.to(BF).float() @ v) / e.sum(-1, keepdim=True)).transpose(1, 2).reshape(F * 192, D)
        exact = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(F * 192, D)
        assert float((got - stored).abs().max()) < 2e-2
        assert float((got - exact).abs().max()) < 5e-2
    top = float(a.amax(-1).median())
    assert (top < 0.01) if scale == 0.05 else (top > 0.8) if scale == 4.0 else (0.01 < top < 0.8), top


@gpu
@pytest.mark.parametrize("D,heads", [(1280, 16), (512, 8)])
def test_vit_attention_one_dominant_key(H, D, heads):
    """Every query's first component is 16 and so is key 77's (131 in the second frame), zero in the other keys: that
    key's logit lies 256 / sqrt(hd) above the rest, and the output is its value row."""
    F, hd = 2, D // heads
    qkv = torch.randn((F * 192, 3 * D), generator=_gen(11)).to(BF).view(F, 192, 3, heads, hd).clone()
    qkv[:, :, 0, :, 0] = 16.0
    qkv[:, :, 1, :, 0] = 0.0
    qkv[0, 77, 1, :, 0] = 16.0
    qkv[1, 131, 1, :, 0] = 16.0
    a = _attn_check(H, qkv.view(F * 192, 3 * D), F, D, heads, f"D {D} heads {heads} dominant key")
    assert float(a[0, :, :, 77].min()) > 0.999 and float(a[1, :, :, 131].min()) > 0.999


# ------------------------------------------------------------------------------ the decoder's one-query attention
@gpu
@pytest.mark.parametrize("ctx", [192, 1, 63, 64, 65, 256])
@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("heads", [4, 8, 12])
def test_xattn1_vs_float64(H, heads, F, ctx):
    inner = 64 * heads
    ldq, ldkv, ldo = inner + 8, 2 * inner + 16, inner + 24
    g = _gen(1000 * heads + 10 * F + ctx)
    q = torch.randn((F, inner), generator=g).to(BF)
    kv = torch.randn((F * ctx, 2 * inner), generator=g).to(BF)
    kv[:, :inner] *= 1.5    # logits of standard deviation 1.5: ordinary softmax rows
    out = Buf(F, ldo, BF)
    H.xattn1(_with_nan_cols(q, ldq).to(DEV), ldq, _with_nan_cols(kv, ldkv).to(DEV), ldkv, out.t, ldo, F, heads, ctx)
    got = out.check(F, inner).double()

    def run(qq, kk):
        k = kk[:, :inner].view(F, ctx, heads, 64).transpose(1, 2)
        v = kk[:, inner:].view(F, ctx, heads, 64).transpose(1, 2)
        a = torch.softmax((qq.view(F, heads, 1, 64) @ k.transpose(-2, -1)) * 0.125, -1)
        return (a @ v).reshape(F, inner)

    ref = run(q.double(), kv.double())
    e_ref = float((run(q.float(), kv.float()).double() - ref).abs().max())
    bound = U8 * ref.abs() + 20 * e_ref
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    _report(f"xattn1 heads {heads} F {F} ctx {ctx} (e_ref {e_ref:.2e})", err, bound)
    assert bool((err <= bound).all()), float((err / bound).max())


# ------------------------------------------------------------------------------ softmax rows
def _softmax_check(H, x, tag):
    rows, Cc = x.shape
    out = Buf(rows, Cc, BF)
    H.softmax_rows_bf16(x.to(DEV), out.t, rows, Cc)
    got = out.check(rows, Cc).double()
    ref = torch.softmax(x.double(), -1)
    e_ref = float((torch.softmax(x, -1).double() - ref).abs().max())
    bound = U8 * ref + 20 * e_ref
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    _report(f"softmax_rows {tag} (e_ref {e_ref:.2e})", err, bound)
    assert bool((err <= bound).all()), float((err / bound).max())
    sums = got.sum(-1)
    assert float((sums - 1).abs().max()) <= U8, float((sums - 1).abs().max())
    return got


@gpu
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("rows", [1, 5, 1024])
@pytest.mark.parametrize("Cc", [256, 2048, 100])
def test_softmax_rows_vs_float64(H, Cc, rows, scale):
    x = torch.randn((rows, Cc), generator=_gen(Cc + rows)) * scale
    _softmax_check(H, x, f"C {Cc} rows {rows} scale {scale}")


@gpu
@pytest.mark.parametrize("Cc", [256, 2048, 100])
def test_softmax_rows_crafted(H, Cc):
    """Row 0: equal values -> 1 / C in every column; row 1: one entry 200 above the rest -> that entry is 1 and the
    rest 0 (e^-200 is below bf16's range); row 2 and 3: the same two, shifted far from 0; row 4: ordinary."""
    x = torch.randn((5, Cc), generator=_gen(5)) * 3
    x[0] = 0.75
    x[1, Cc // 3] = float(x[1].max()) + 200.0
    x[2] = -1.0e4
    x[3] = x[1] + 3.0e4
    got = _softmax_check(H, x, f"C {Cc} crafted")
    want = float(torch.tensor(1.0 / Cc).to(BF))
    assert bool((got[0] == want).all()) and bool((got[2] == want).all())
    for r in (1, 3):
        assert float(got[r, Cc // 3]) == 1.0 and float(got[r].sum()) == 1.0


# ------------------------------------------------------------------------------ readout
def _rot6d_64(x):
    """rot6d_to_rotmat (Gram-Schmidt, F.normalize eps 1e-12) in float64: x [n, 6] -> (R [n, 3, 3], |a2| / |u|)"""
    a1, a2 = x[:, :3], x[:, 3:]
    b1 = a1 / np.maximum(np.linalg.norm(a1, axis=1, keepdims=True), 1e-12)
    u = a2 - (b1 * a2).sum(1, keepdims=True) * b1
    nu = np.linalg.norm(u, axis=1, keepdims=True)
    b2 = u / np.maximum(nu, 1e-12)
    b3 = np.cross(b1, b2)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(nu[:, 0] > 0, np.linalg.norm(a2, axis=1) / nu[:, 0], 1.0)
    return np.stack([b1, b2, b3], -1), ratio


def _init_pose():
    """nonzero, and different for every joint and component: 144 values in +-[0.3, 1.73], alternating sign"""
    i = np.arange(144)
    return ((0.3 + 0.01 * i) * np.where(i % 2, -1.0, 1.0)).astype(np.float32)


def _readout_run(H, six, shape, F):
    """six f32 [F, 24, 6]: the network's part of every joint's 6D vector (before init_pose), laid out as the model's
    buffers hold it; -> pose [F, 23, 9], gori [F, 9], betas [F, 10], the float64 rotations and |a2| / |u|"""
    ip, ib = _init_pose(), (np.arange(10, dtype=np.float32) - 4.5) * np.float32(0.37)
    rd = np.full((F, 256), np.nan, np.float32)
    bp = np.full((F, 256), np.nan, np.float32)
    rd[:, 0:6] = six[:, 0]
    rd[:, 6:18] = six[:, 22:24].reshape(F, 12)
    rd[:, 18:28] = shape
    rd[:, 28:31] = 123.0   # cam: computed by the model's readout GEMM, not used
    bp[:, :126] = six[:, 1:22].reshape(F, 126)
    pose, gori, betas = Buf(F, 207, torch.float32), Buf(F, 9, torch.float32), Buf(F, 10, torch.float32)
    dv = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    H.hmr_readout(dv(rd), 256, dv(bp), 256, dv(ip), dv(ib), pose.t, gori.t, betas.t, F)
    x = six.astype(np.float64) + ip.astype(np.float64).reshape(1, 24, 6)
    R, ratio = _rot6d_64(x.reshape(-1, 6))
    got = np.concatenate([gori.check(F, 9).numpy().reshape(F, 1, 9), pose.check(F, 207).numpy().reshape(F, 23, 9)], 1)
    assert np.array_equal(betas.check(F, 10).numpy(), shape + ib[None, :]), "betas is one float32 add"
    return got.reshape(F * 24, 3, 3), R, ratio


@gpu
@pytest.mark.parametrize("F", [1, 11, 300])
def test_readout_vs_float64(H, F):
    """Random 6D vectors, and in every frame four joints (0, 9, 21, 23: one per source range and the last) whose a2 is
    nearly parallel to a1, |a2| / |u| between 30 and 900.  A wrong joint offset or init_pose index moves a 6D vector by
    at least 0.01 (init_pose's step), mostly by O(1).  The random vectors are redrawn until |a2| / |u| <= 20: R R^T = I
    is asserted on them at 1e-5, and float32 Gram-Schmidt loses orthogonality as 1e-7 |a2| / |u| (a float32
    restatement on unconditioned normal draws: 9.7e-6 at a ratio of 100, 2.1e-5 worst over 20 x 7,200 vectors)."""
    rng = np.random.default_rng(40 + F)
    six = rng.standard_normal((F, 24, 6)).astype(np.float32)
    ip = _init_pose().reshape(24, 6)
    for _ in range(100):
        redo = (_rot6d_64((six.astype(np.float64) + ip).reshape(-1, 6))[1] > 20).reshape(F, 24)
        if not redo.any():
            break
        six[redo, 3:] = rng.standard_normal((int(redo.sum()), 3)).astype(np.float32)
    for n, j in enumerate((0, 9, 21, 23)):
        a1 = six[:, j, :3].astype(np.float64) + ip[j, :3]
        w = np.cross(a1, rng.standard_normal((F, 3)))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        t = rng.uniform(0.5, 2.0, (F, 1)) * (1 if n % 2 else -1)
        a2 = t * a1 + w * np.abs(t) * np.linalg.norm(a1, axis=1, keepdims=True) / rng.uniform(30, 900, (F, 1))
        six[:, j, 3:] = (a2 - ip[j, 3:]).astype(np.float32)
    shape = rng.standard_normal((F, 10)).astype(np.float32)
    got, R, ratio = _readout_run(H, six, shape, F)
    assert ratio.max() <= 1000.0, ratio.max()
    hard = np.zeros((F, 24), bool)
    hard[:, (0, 9, 21, 23)] = True
    assert ratio[hard.ravel()].min() > 25
    bound = 16 * 2.0 ** -24 * (1 + ratio)
    err = np.abs(got - R).max(axis=(1, 2))
    print(f"readout F {F}: worst error / bound {float((err / bound).max()):.3f}, max |a2|/|u| {ratio.max():.0f}")
    assert (err <= bound).all(), (float((err / bound).max()), int(np.argmax(err / bound)) % 24)
    assert ratio[~hard.ravel()].max() <= 20
    easy = got[~hard.ravel()]  # the random vectors
    assert np.abs(easy @ easy.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5


@gpu
def test_readout_degenerate_vectors(H):
    """a1 = 0 (joints 0, 5, 22 of frame 0): b1 = b3 = 0 exactly and b2 = a2 / |a2|, as F.normalize with eps 1e-12
    gives; a2 = 0 (joints 1, 21, 23 of frame 1): b2 = b3 = 0 exactly and b1 = a1 / |a1|."""
    F = 2
    rng = np.random.default_rng(7)
    six = rng.standard_normal((F, 24, 6)).astype(np.float32)
    ip = _init_pose().reshape(24, 6)
    for j in (0, 5, 22):
        six[0, j, :3] = -ip[j, :3]
    for j in (1, 21, 23):
        six[1, j, 3:] = -ip[j, 3:]
    got, R, ratio = _readout_run(H, six, rng.standard_normal((F, 10)).astype(np.float32), F)
    got, R = got.reshape(F, 24, 3, 3), R.reshape(F, 24, 3, 3)
    bound = (16 * 2.0 ** -24 * (1 + ratio)).reshape(F, 24)
    assert (np.abs(got - R).max(axis=(2, 3)) <= bound).all()
    for j in (0, 5, 22):
        assert (got[0, j][:, 0] == 0).all() and (got[0, j][:, 2] == 0).all()
        assert abs(np.linalg.norm(got[0, j][:, 1].astype(np.float64)) - 1) < 1e-6
    for j in (1, 21, 23):
        assert (got[1, j][:, 1] == 0).all() and (got[1, j][:, 2] == 0).all()
        assert abs(np.linalg.norm(got[1, j][:, 0].astype(np.float64)) - 1) < 1e-6


# ------------------------------------------------------------------------------ cast / bcast / copy rows
def _f32_rows(rows, D, seed):
    """random float32 over many binades, with bf16 rounding ties (to even, both ways), +-0, +-inf and the largest
    float32 (rounds to inf) in the first columns"""
    g = _gen(seed)
    x = torch.randn((rows, D), generator=g) * torch.exp2(torch.randint(-20, 20, (rows, D), generator=g).float())
    special = torch.tensor([1.00390625, 1.01171875, -1.00390625, -1.01171875, 0.0, -0.0, float("inf"), float("-inf"),
                            3.4028234663852886e38, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23, 65280.0])
    n = min(D, len(special))
    x[0, :n] = special[:n]
    return x


@gpu
@pytest.mark.parametrize("rows", [1, 5, 257])
@pytest.mark.parametrize("D", [256, 1024, 12])
def test_cast_rows_bf16_bit_exact(H, D, rows):
    ldx, ldy = D + 4, D + 8
    x = _f32_rows(rows, D, seed=D + rows)
    y = Buf(rows, ldy, BF)
    H.cast_rows_bf16(_with_nan_cols(x, ldx).to(DEV), ldx, y.t, ldy, rows, D)
    got = y.check(rows, D)
    assert torch.equal(got.view(torch.int16), x.to(BF).view(torch.int16))


@gpu
@pytest.mark.parametrize("rows", [1, 5, 257])
@pytest.mark.parametrize("D", [256, 1024, 7])
def test_bcast_rows_bit_exact(H, D, rows):
    vec = _f32_rows(1, D, seed=D)[0]
    y = Buf(rows, D, torch.float32)
    H.bcast_rows(vec.to(DEV), y.t, rows, D)
    got = y.check(rows, D)
    assert torch.equal(got.view(torch.int32), vec.view(torch.int32).expand(rows, D))


@gpu
@pytest.mark.parametrize("rows", [1, 5, 257])
@pytest.mark.parametrize("D", [256, 1024, 7])
def test_copy_rows_bit_exact(H, D, rows):
    ldx, ldy = D + 3, D + 5
    x = _f32_rows(rows, D, seed=2 * D + rows)
    y = Buf(rows, ldy, torch.float32)
    H.copy_rows(_with_nan_cols(x, ldx).to(DEV), ldx, y.t, ldy, rows, D)
    got = y.check(rows, D)
    assert torch.equal(got.view(torch.int32), x.view(torch.int32))
