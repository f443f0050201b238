"""TokenHMR extractor (include/vge_hmr.h, vge_vit.hip): kernels against torch-fp32 restatements of the same ops,
the whole extractor against oracle/hmr.py.

Parity vs the upstream TokenHMR model is UNPINNED (its ViT / decoder / tokenizer are not in the reference and
no weights exist offline); what is pinned here is that the HIP path computes the restated architecture:
  GEMM epilogues       vs torch fp32 on the same bf16 operands: f32 outputs 2e-5 relative to the row scale,
                       bf16 outputs within 1 bf16 ulp (2^-8 relative)
  LayerNorm            1 bf16 ulp
  attention            vs a torch fp32 restatement with the kernel's bf16 storage points: 2e-2 abs on O(1) values
  whole extractor      vs oracle/hmr.py with the same bf16 storage points (bf16=True): rotations 1.5e-2 abs,
                       betas / token_out 2e-2 abs; the fp32 deviation (bf16=False) is printed, not asserted
"""
import numpy as np
import pytest
import torch

DEV = "cuda:0"


def test_oracle_rot6d_identity_and_orthonormal():
    from oracle.hmr import rot6d_to_rotmat
    x = torch.tensor([[1.0, 0, 0, 0, 1, 0]])
    assert torch.allclose(rot6d_to_rotmat(x)[0], torch.eye(3))
    R = rot6d_to_rotmat(torch.randn(64, 6))
    assert float((R @ R.transpose(1, 2) - torch.eye(3)).abs().max()) < 1e-5
    assert torch.allclose(torch.linalg.det(R), torch.ones(64), atol=1e-5)


def test_oracle_patch_grid_is_16x12():
    from oracle.hmr import OracleHmr
    from vge.hmr import HmrConfig
    from vge import synth
    cfg = HmrConfig(embed_dim=256, depth=0, heads=4, mlp_dim=256, dec_dim=256, dec_depth=0, dec_heads=4, dec_mlp=256,
                    tok_num=1, tok_classes=256, tok_code_dim=256)
    sd = synth.make_hmr_state_dict(cfg)
    ctx = OracleHmr(sd, cfg).backbone(synth.make_frames(1, 2))
    assert tuple(ctx.shape) == (2, 192, 256)


def test_hmr_config_rejected_without_gpu_work():
    import ctypes as C
    from vge import hmr as H
    from vge import lib as L
    lib = H._sig(L.load())
    bad = H._cfg_c(H.HmrConfig(embed_dim=1000))
    out = C.c_void_p()
    assert lib.vge_hmr_create(C.byref(bad), None, 0, C.byref(out)) == 1
    assert b"embed_dim" in lib.vge_last_error()


gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vge import hmr
    return hmr


def _bf(shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


@gpu
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (512, 768, 1280), (768, 1280, 5120), (256, 3840, 1280)])
@pytest.mark.parametrize("epi", ["bf16", "gelu_bf16", "res_f32", "pe_f32", "f32"])
def test_gemm_bf16_epilogues(H, M, N, K, epi):
    if epi == "pe_f32" and M % 192:
        M = 768
    A = _bf((M, K), 1.0, 1)
    W = _bf((N, K), K ** -0.5, 2)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(3)) * 0.1
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(4))
    pos = torch.randn(193, N, generator=torch.Generator().manual_seed(5))
    ref = A.double() @ W.double().t() + bias.double()
    Ad, Wd = A.to(DEV), W.to(DEV)
    kw = dict(bias=bias.to(DEV))
    if epi == "res_f32":
        kw["res"] = res.to(DEV)
        ref = ref + res.double()
    if epi == "pe_f32":
        kw["pos"] = pos.to(DEV)
        tok = torch.arange(M) % 192
        ref = ref + pos.double()[1 + tok] + pos.double()[0]
    if epi == "gelu_bf16":
        ref = torch.nn.functional.gelu(ref)
    out = H.gemm_bf16(Ad, Wd, epi, **kw).double().cpu()
    if epi in ("bf16", "gelu_bf16"):
        assert float(((out - ref).abs() / (ref.abs() + 1e-2)).max()) < 2 ** -7
    else:
        assert float((out - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))


@gpu
def test_gemm_bf16_rejects_bad_shapes(H):
    from vge import lib as L
    A = _bf((200, 64)).to(DEV)
    W = _bf((256, 64)).to(DEV)
    with pytest.raises(L.VgeError):
        H.gemm_bf16(A, W)


@gpu
@pytest.mark.parametrize("D", [256, 512, 768, 1024, 1280])
def test_layernorm_bf16(H, D):
    """Every width the kernel is instantiated for, at 1, 5 and 301 rows (4 rows per block: the last block is partly
    past the end), on N(1, 3^2) rows and on rows of mean 1,000 and standard deviation 1 (the variance is taken about the
    mean; E[x^2] - mean^2 would lose it), against float64 within one bf16 rounding, 2^-8 |ref|, plus 20 e_ref, e_ref =
    max |torch float32 layer_norm on the CPU - float64| (tests/test_encoder_shapes.py's yardstick).  x and y have spare
    rows behind `rows`: y's keep their NaN pattern."""
    g = torch.Generator().manual_seed(100 + D)
    w = torch.randn(D, generator=g) * 0.1 + 1
    b = torch.randn(D, generator=g) * 0.1
    for rows in (1, 5, 301):
        for name, mean, std in (("N(1, 9)", 1.0, 3.0), ("N(1000, 1)", 1000.0, 1.0)):
            x = torch.randn(rows + 3, D, generator=g) * std + mean
            ref = torch.nn.functional.layer_norm(x[:rows].double(), (D,), w.double(), b.double(), eps=1e-6)
            e_ref = float((torch.nn.functional.layer_norm(x[:rows], (D,), w, b, eps=1e-6).double() - ref).abs().max())
            raw = torch.full((rows + 3, D), 0x7FC1, dtype=torch.int16, device=DEV)
            H.layernorm_bf16(x.to(DEV), w.to(DEV), b.to(DEV), 1e-6, out=raw.view(torch.bfloat16), rows=rows)
            raw = raw.cpu()
            assert bool((raw[rows:] == 0x7FC1).all()), "rows behind the last one were written"
            out = raw[:rows].view(torch.bfloat16).double()
            bound = 2.0 ** -8 * ref.abs() + 20 * e_ref
            err = (out - ref).abs()
            print(f"layernorm D {D} rows {rows} {name}: worst error / bound {float((err / bound).max()):.3f} "
                  f"(e_ref {e_ref:.2e})")
            assert torch.isfinite(out).all()
            assert bool((err <= bound).all()), (rows, name, float((err / bound).max()))


def _cfg_small(H, wide: bool):
    if wide:  # ViT-H layer shapes (head dim 80), one block
        return H.HmrConfig(embed_dim=1280, depth=1, heads=16, mlp_dim=5120, dec_depth=2, tok_num=8, tok_classes=256,
                           tok_code_dim=256)
    return H.HmrConfig(embed_dim=256, depth=2, heads=4, mlp_dim=1024, dec_dim=256, dec_depth=2, dec_heads=4,
                       dec_mlp=256, tok_num=4, tok_classes=256, tok_code_dim=256)


@gpu
@pytest.mark.parametrize("wide", [True, False])
def test_extractor_vs_oracle(H, wide):
    from oracle.hmr import OracleHmr
    from vge import synth
    cfg = _cfg_small(H, wide)
    sd = synth.make_hmr_state_dict(cfg)
    frames = synth.make_frames(11, 5)  # 5 frames: token rows pad to 1024 and head rows to 256
    ex = H.HmrExtractor(sd, cfg, device=DEV, max_frames=8)
    out = {k: v.cpu() for k, v in ex.extract(torch.from_numpy(frames).to(DEV)).items()}
    ref = OracleHmr(sd, cfg, bf16=True).forward(frames)
    f32 = OracleHmr(sd, cfg, bf16=False).forward(frames)
    # bf16 storage points round to 2^-8: an f32 summation-order difference that flips one rounding moves that
    # value by an ulp and the flip propagates; Gram-Schmidt (rot6d) divides by the 6D vector norms
    tol = {"pose": 1.5e-2, "global_orient": 1.5e-2, "betas": 2e-2, "vit": 2e-2}
    for k, t in tol.items():
        err = float((out[k] - ref[k]).abs().max())
        dev32 = float((out[k] - f32[k]).abs().max())
        print(f"{k}: max|gpu - oracle(bf16 points)| {err:.2e}, vs fp32 model {dev32:.2e}")
        assert err < t, (k, err)
    R = out["pose"].view(-1, 3, 3)
    assert float((R @ R.transpose(1, 2) - torch.eye(3)).abs().max()) < 1e-5
    # a second call with fewer frames reuses the workspace and gives the same rows
    again = ex.extract(torch.from_numpy(frames[:2]).to(DEV))
    assert torch.equal(again["vit"].cpu(), out["vit"][:2])


TOL = {"pose": 1.5e-2, "global_orient": 1.5e-2, "betas": 2e-2, "vit": 2e-2}  # test_extractor_vs_oracle's


def _hmr_cfg(H, E=256, heads=4, Dd=256, dh=4, depth=1, dec_depth=1, **kw):
    base = dict(embed_dim=E, depth=depth, heads=heads, mlp_dim=2 * E, dec_dim=Dd, dec_depth=dec_depth, dec_heads=dh,
                dec_mlp=256, tok_num=4, tok_classes=256, tok_code_dim=256)
    base.update(kw)
    return H.HmrConfig(**base)


# the family vge_hmr_create accepts (include/vge_hmr.h), one member per dimension it varies in; DESIGN section 7
HMR_CONFIGS = {
    "E512-h8-D512-h8": dict(E=512, heads=8, Dd=512, dh=8, depth=2, dec_depth=2),
    "E768-h12-D256-h4": dict(E=768, heads=12, Dd=256, dh=4),
    "E1024-h16-D1280-h12": dict(E=1024, heads=16, Dd=1280, dh=12),
    "E1280-h20-D1024-h8": dict(E=1280, heads=20, Dd=1024, dh=8),
    "E256-h4-D512-h4": dict(E=256, heads=4, Dd=512, dh=4, depth=2, dec_depth=2),
    "depth0-dec1": dict(depth=0, dec_depth=1),
    "dec_depth0": dict(depth=1, dec_depth=0),
    "pad0-img192": dict(pad=0, in_w=192, img_w=192),
    "pad0-margin": dict(pad=0),
    "260x208-img200": dict(in_h=260, img_h=260, in_w=208, img_w=200),
}


def _extract_vs_oracle(H, cfg, frames, ex=None, tag=""):
    from oracle.hmr import OracleHmr
    from vge import synth
    sd = synth.make_hmr_state_dict(cfg)
    ex = ex or H.HmrExtractor(sd, cfg, device=DEV, max_frames=len(frames))
    out = {k: v.cpu() for k, v in ex.extract(torch.from_numpy(frames).to(DEV)).items()}
    ref = OracleHmr(sd, cfg, bf16=True).forward(frames)
    for k, t in TOL.items():
        assert torch.isfinite(out[k]).all(), k
        err = float((out[k] - ref[k]).abs().max())
        print(f"{tag} {k}: max|gpu - oracle(bf16 points)| {err:.2e} (bound {t:.1e})")
        assert err < t, (k, err)
    R = torch.cat([out["global_orient"], out["pose"]], 1).view(-1, 3, 3)
    assert float((R @ R.transpose(1, 2) - torch.eye(3)).abs().max()) < 1e-5
    return ex, out


@gpu
@pytest.mark.parametrize("name", list(HMR_CONFIGS))
def test_extractor_configs_vs_oracle(H, name):
    """One member of every dimension of the accepted family, random weights, at most 2 blocks, 5 frames (token rows
    pad to 1024, head rows to 256), at test_extractor_vs_oracle's tolerances."""
    from vge import synth
    cfg = _hmr_cfg(H, **HMR_CONFIGS[name])
    _extract_vs_oracle(H, cfg, synth.make_frames(21, 5, cfg.in_h, cfg.in_w), tag=name)


@gpu
@pytest.mark.parametrize("F", [1, 4, 257])
def test_extractor_frame_counts_vs_oracle(H, F):
    """1 frame; 4 frames = 768 token rows, no padding rows; 257 frames: the head's rows pad to 512."""
    from vge import synth
    _extract_vs_oracle(H, _hmr_cfg(H), synth.make_frames(22, F), tag=f"F {F}")


@gpu
def test_extractor_reserve_then_extract(H):
    """2 frames in a workspace of 2; then, after reserve() to 300 frames (every buffer reallocated, the head's rows 256
    -> 512), the same call gives the same rows."""
    from vge import synth
    frames = synth.make_frames(23, 2)
    ex, first = _extract_vs_oracle(H, _hmr_cfg(H), frames, tag="reserve 2")
    assert ex.max_frames == 2
    ex.reserve(300)
    assert ex.max_frames == 300
    again = {k: v.cpu() for k, v in ex.extract(torch.from_numpy(frames).to(DEV)).items()}
    for k in TOL:
        assert torch.equal(again[k], first[k]), k


@gpu
@pytest.mark.parametrize("epi", ["bf16", "gelu_bf16"])
@pytest.mark.parametrize("M,N,K", [(20480, 1280, 1280), (49152, 5120, 1280), (12288, 1280, 5120)])
def test_gemm_persistent_matches_one_tile_kernel(H, M, N, K, epi):
    """gemmp_bf16_kernel (one workgroup per CU, one continuous LDS ring across its tiles, the epilogue from registers
    under the next tile's first loads) against the one-tile kernel: the same 16x16x32 MFMAs in the same K order and the
    same epilogue arithmetic (bias, then the activation, then one bf16 rounding) -> bit-identical, on the ViT-H shapes
    (qkv-like, fc1, fc2-like K) with more tiles than CUs."""
    import ctypes as C
    from vge import lib as Lb
    lib = Lb.load()
    lib.vge_debug_set_gemm_persist.argtypes = [C.c_int]
    A = _bf((M, K), 1.0, 11).to(DEV)
    W = _bf((N, K), K ** -0.5, 12).to(DEV)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(13)) * 0.1).to(DEV)
    outs = []
    try:
        for p in (0, 1):
            lib.vge_debug_set_gemm_persist(p)
            outs.append(H.gemm_bf16(A, W, epi, bias=bias))
            torch.cuda.synchronize()
    finally:
        lib.vge_debug_set_gemm_persist(0)
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1]), (outs[0].float() - outs[1].float()).abs().max().item()


def _set_gemm_waves(mode):
    import ctypes as C
    from vge import lib as Lb
    lib = Lb.load()
    lib.vge_debug_set_gemm_waves.argtypes = [C.c_int]
    lib.vge_debug_set_gemm_waves(mode)


@gpu
@pytest.mark.parametrize("epi", ["bf16", "gelu_bf16", "res_f32", "pe_f32", "f32"])
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (512, 512, 192)])
def test_gemm_wave_modes_match_default(H, M, N, K, epi):
    """The GEMM's wave modes (2 = gemm2_bf16_kernel's 128 x 256 tiles with swapped MFMA operands, 4 = four waves of
    128 x 128, 8 / 16 = the 8-wave kernel forced to 32x32x16 / 16x16x32) against the default choice by epilogue (1):
    every form accumulates the same products in the same K order (32-deep stages of two 16-k steps) and applies the
    same epilogue operations in the same order -> bit-identical.  (256, 256, 64) is one tile with two K stages, the
    shortest ring the kernels accept; (512, 512, 192) is four tiles in two column panels with six stages, so the 3-slot
    and the 5-slot rings both wrap.  (Before the LDS ordering point in its epilogue, mode 4 differed from the default by
    5.9-7.2 on res_f32 and pe_f32 at both shapes, in rows 4 k + 3 of its LDS transpose: DESIGN 3.7.)"""
    if epi == "pe_f32":
        M = 768
    A = _bf((M, K), 1.0, 21).to(DEV)
    W = _bf((N, K), K ** -0.5, 22).to(DEV)
    kw = dict(bias=(torch.randn(N, generator=torch.Generator().manual_seed(23)) * 0.1).to(DEV))
    if epi == "res_f32":
        kw["res"] = torch.randn(M, N, generator=torch.Generator().manual_seed(24)).to(DEV)
    if epi == "pe_f32":
        kw["pos"] = torch.randn(193, N, generator=torch.Generator().manual_seed(25)).to(DEV)
    outs = {}
    try:
        for mode in (1, 2, 4, 8, 16):
            _set_gemm_waves(mode)
            outs[mode] = H.gemm_bf16(A, W, epi, **kw)
            torch.cuda.synchronize()
    finally:
        _set_gemm_waves(1)
    assert torch.isfinite(outs[1].float()).all()
    for mode in (2, 4, 8, 16):
        assert torch.equal(outs[1], outs[mode]), (mode, (outs[1].float() - outs[mode].float()).abs().max().item())


@gpu
@pytest.mark.parametrize("n,Hh,Ww,Cin,Cout,act,res", [
    (4, 25, 25, 1024, 1024, "relu", None),   # M = 2500: ragged last 256-row and 128-row tile
    (3, 13, 17, 512, 512, "relu", "pre"),    # M = 663, bf16 residual before the ReLU
])
def test_gemm_wave_modes_partial_m_match_default_conv(n, Hh, Ww, Cin, Cout, act, res):
    """The partial-M instantiations of the same modes, reached through a 1x1 conv with variant 9 forced (ragged shapes of
    test_dwpose.py::test_conv_1x1_gemm_variant_matches_default): bit-identical to the default conv kernel."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctypes as C
    from vge import dwpose as D
    from vge import lib as Lb
    lib = Lb.load()
    lib.vge_debug_set_conv_variant.argtypes = [C.c_int]
    x = _bf((n, Hh, Ww, Cin), seed=31).to(DEV)
    w = _bf((Cout, Cin, 1, 1), (2.0 / Cin) ** 0.5, seed=32).to(DEV)
    b = (torch.randn(Cout, generator=torch.Generator().manual_seed(33)) * 0.1).to(DEV)
    r = _bf((n, Hh, Ww, Cout), seed=34).to(DEV) if res else None
    conv = lambda: D.conv_bf16(x, w, b, stride=1, pad=0, act=act, res=r, res_pre=res == "pre")  # noqa: E731
    want = conv()
    outs = {}
    try:
        lib.vge_debug_set_conv_variant(9)
        for mode in (1, 2, 4, 8, 16):
            _set_gemm_waves(mode)
            outs[mode] = conv()
            torch.cuda.synchronize()
    finally:
        lib.vge_debug_set_conv_variant(0)
        _set_gemm_waves(1)
    assert torch.isfinite(want.float()).all()
    for mode, got in outs.items():
        assert torch.equal(want, got), (mode, (want.float() - got.float()).abs().max().item())


@gpu
@pytest.mark.parametrize("epi", ["bf16", "res_f32", "f32"])
@pytest.mark.parametrize("M,N,K", [(49152, 3840, 1280), (12288, 1280, 5120), (1000, 256, 64), (333, 768, 1024)])
def test_library_gemm_matches_kernel(H, M, N, K, epi):
    """The library path (hipBLASLt through vge_op_gemm_lib: the ViT's bias / f32-residual / f32-out linears and the
    detector's 1x1 convs run there) against gemm_bf16_kernel on the same operands: both accumulate in f32 in their own K
    order, so f32 outputs agree to accumulation error and bf16 outputs to one rounding of it.  Also ragged M, N, K
    that the kernel does not take (compared against the torch f32 product instead)."""
    A = _bf((M, K), 1.0, 21).to(DEV)
    W = _bf((N, K), K ** -0.5, 22).to(DEV)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(23)) * 0.1).to(DEV)
    res = (torch.randn((M, N), generator=torch.Generator().manual_seed(24)) * 0.5).to(DEV) if epi == "res_f32" else None
    got = H.gemm_lib(A, W, epi, bias=bias, res=res)
    ref32 = A.float() @ W.float().t() + bias
    if res is not None:
        ref32 = ref32 + res
    kernel_takes = M % 256 == 0 and N % 256 == 0 and K % 64 == 0
    ref = H.gemm_bf16(A, W, epi, bias=bias, res=res) if kernel_takes else ref32
    torch.cuda.synchronize()
    g, r = got.float(), ref.float()
    assert torch.isfinite(g).all()
    scale = float(ref32.abs().max())
    if epi == "bf16":
        bound = 2.0 ** -7 * r.abs() + 1e-5 * scale
    else:
        bound = torch.full_like(r, 2e-6 * scale * K ** 0.5)
    err = (g - r).abs()
    print(f"{epi} {M}x{N}x{K}: max |lib - {'kernel' if kernel_takes else 'torch f32'}| {float(err.max()):.2e}")
    assert bool((err <= bound).all()), float((err - bound).max())


@gpu
def test_library_path_off_switch(H):
    """vge_debug_set_gemm_lib(0) takes the library path out (VGE_ERR_UNSUPPORTED from vge_op_gemm_lib), and the GELU
    epilogue is never on it (the library's GELU is the tanh form)."""
    import ctypes as C
    from vge import lib as Lb
    lib = Lb.load()
    lib.vge_debug_set_gemm_lib.argtypes = [C.c_int]
    A = _bf((256, 256), 1.0, 31).to(DEV)
    W = _bf((256, 256), 1.0 / 16, 32).to(DEV)
    with pytest.raises(Lb.VgeError):
        H.gemm_lib(A, W, "gelu_bf16")
    try:
        lib.vge_debug_set_gemm_lib(0)
        with pytest.raises(Lb.VgeError):
            H.gemm_lib(A, W, "bf16")
    finally:
        lib.vge_debug_set_gemm_lib(1)
    H.gemm_lib(A, W, "bf16")
    torch.cuda.synchronize()


@gpu
def test_full_depth_extractor_vs_oracle(H):
    """The whole TokenHMR extractor at full size -- HMR2's ViT-H/16 (32 blocks, E 1280, 16 heads, MLP 5120) and the
    6-layer decoder, the configuration config 3 runs (vge.hmr.TOKENHMR) -- on 3 frames vs oracle/hmr.py with the
    kernels' bf16 storage points, at the 2-block test's bounds (measured on the MI355X: pose 6.4e-3, global_orient
    3.0e-3, betas 8.8e-3, vit 1.2e-2 -- a storage rounding flipped by an f32 summation-order difference does not grow
    over the 32 blocks' pre-norm residual stream)."""
    from oracle.hmr import OracleHmr
    from vge import synth
    cfg = H.TOKENHMR
    sd = synth.make_hmr_state_dict(cfg)
    frames = synth.make_frames(13, 3)
    ex = H.HmrExtractor(sd, cfg, device=DEV, max_frames=4)
    out = {k: v.cpu() for k, v in ex.extract(torch.from_numpy(frames).to(DEV)).items()}
    torch.set_num_threads(max(1, min(16, len(__import__("os").sched_getaffinity(0)))))
    ref = OracleHmr(sd, cfg, bf16=True).forward(frames)
    tol = {"pose": 1.5e-2, "global_orient": 1.5e-2, "betas": 2e-2, "vit": 2e-2}
    for k, t in tol.items():
        err = float((out[k] - ref[k]).abs().max())
        print(f"full depth {k}: max|gpu - oracle(bf16 points)| {err:.2e} (bound {t:.0e})")
        assert err < t, (k, err)
    R = out["pose"].view(-1, 3, 3)
    assert float((R @ R.transpose(1, 2) - torch.eye(3)).abs().max()) < 1e-5
