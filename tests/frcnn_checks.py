"""The gate detector's stage-wise parity checks (vge.frcnn.FrcnnDetector against oracle/frcnn.py), shared by
tests/test_frcnn.py (four 256 x 256 frames at the reference's 800-pixel config) and tests/test_frcnn_shapes.py (the
non-square, padded and downscaled geometries).  Not a test module: plain functions of a `run` dict

  cfg, sd      the detector's config and state dict
  frames       uint8 [F, H, W, 3] host frames;  hw = (H, W)
  out, taps    FrcnnDetector.detect's outputs and parity taps, on the host
  shapes       FrcnnDetector.shapes(H, W): resized / padded sizes, the five level sizes
  oracle       OracleFrcnn(sd, cfg, bf16=True)

Every stage is checked on the GPU's own input to that stage, so a tolerance covers one stage's arithmetic.  The
thresholds are those test_frcnn.py has always asserted; each check prints what it measured and returns it.
"""
import numpy as np
import torch


def collect_run(det, sd, cfg, frames, device):
    """One taps-on detect of `frames` (host uint8 [F, H, W, 3]) on `det`, everything moved to the host."""
    from oracle.frcnn import OracleFrcnn
    F_, H, W = (int(v) for v in frames.shape[:3])
    fr = torch.from_numpy(frames).to(device)
    taps = det.make_taps(F_, H, W)
    out = det.detect(fr, taps=taps)
    torch.cuda.synchronize()
    host = lambda v: [x.cpu() for x in v] if isinstance(v, list) else v.cpu()  # noqa: E731
    return dict(cfg=cfg, sd=sd, frames=frames, hw=(H, W), out={k: host(v) for k, v in out.items()},
                taps={k: host(v) for k, v in taps.items()}, shapes=det.shapes(H, W),
                oracle=OracleFrcnn(sd, cfg, bf16=True))


def oracle_forward(run, frames=(0, 1)):
    """The oracle predictor from the frames themselves, on `frames` (indices): (instances, intermediate tensors)."""
    torch.set_num_threads(16)
    return run["oracle"].detect(run["frames"][list(frames)], taps=True)


def nchw(t):  # bf16 [F, h, w, C] -> float [F, C, h, w]
    return t.float().permute(0, 3, 1, 2).contiguous()


def check_resize(run):
    """The PIL bilinear resample, byte for byte, on every frame."""
    from oracle.frcnn import resize_pil
    nh, nw = run["shapes"]["resized"]
    for f in range(run["frames"].shape[0]):
        np.testing.assert_array_equal(run["taps"]["resized"][f].numpy(), resize_pil(run["frames"][f], nh, nw))


def check_backbone_fpn(run, aux, frames=(0, 1)):
    """P2..P6 vs the oracle run from the frames (`aux` of oracle_forward on the same `frames`)."""
    got = []
    for l in range(5):
        g, o = nchw(run["taps"]["fpn"][l][list(frames)]), aux["P"][l]
        assert g.shape == o.shape, (l, g.shape, o.shape)
        rel = float((g - o).norm() / o.norm())
        mx = float((g - o).abs().max() / o.abs().max())
        print(f"P{l + 2}: rel L2 {rel:.2e}, max |d| / max |ref| {mx:.2e}")
        assert rel < 3e-2 and mx < 0.15, (l, rel, mx)
        got.append((rel, mx))
    return got


def check_rpn_head(run, frames=(0, 1)):
    """Logits / deltas from the GPU's P levels (one bf16 conv + f32 1x1)."""
    o = run["oracle"]
    fi, nf = list(frames), len(frames)
    got = []
    for l in range(5):
        P = nchw(run["taps"]["fpn"][l][fi])
        lo, de = o.rpn_head(P)
        g = run["taps"]["rpn"][l][fi]
        h, w = g.shape[1:3]
        assert (h, w) == tuple(run["shapes"]["levels"][l])
        gl = g[..., :3].reshape(nf, -1)
        gd = g[..., 3:15].reshape(nf, h * w * 3, 4)
        el, ed = float((gl - lo).abs().max()), float((gd - de).abs().max())
        print(f"RPN P{l + 2}: logits max|d| {el:.2e} (max {float(lo.abs().max()):.2f}), deltas {ed:.2e}")
        assert el < 3e-2 * max(1.0, float(lo.abs().max())) and ed < 3e-2 * max(0.1, float(de.abs().max()))
        got.append((el, ed))
    return got


def gpu_head_inputs(run, f):
    t = run["taps"]
    logits = [t["rpn"][l][f, ..., :3].reshape(-1) for l in range(5)]
    deltas = [t["rpn"][l][f, ..., 3:15].reshape(-1, 4) for l in range(5)]
    return logits, deltas


def check_proposals(run, taps=None, shapes=None):
    """Top-k / decode / clip / batched NMS / merge from the GPU's logits, on every frame: identical order and scores.
    `taps` / `shapes`: another run's (a test of the test feeds one geometry's taps to another's check)."""
    o = run["oracle"]
    t = run["taps"] if taps is None else taps
    sh = run["shapes"] if shapes is None else shapes
    levels = [tuple(s) for s in sh["levels"]]
    size = tuple(sh["resized"])
    got = []
    for f in range(t["n_proposals"].shape[0]):
        lo, de = gpu_head_inputs(dict(taps=t), f)
        pb, ps = o.proposals(lo, de, size, levels)
        n = int(t["n_proposals"][f])
        gp = t["proposals"][f, :n]
        assert n == pb.shape[0], (f, n, pb.shape[0])
        assert torch.equal(gp[:, 4], ps), f"frame {f}: proposal order / scores differ"
        err = float((gp[:, :4] - pb).abs().max()) if n else 0.0
        print(f"frame {f}: {n} proposals, max |box d| {err:.2e}")
        assert err < 2e-3
        got.append((n, err))
    return got


def check_box_features(run, frames=(0, 1)):
    """ROIAlign from the GPU's P levels and proposals: torchvision's float order, identical but for rare 1-ulp bf16."""
    o, t = run["oracle"], run["taps"]
    got = []
    for f in frames:
        n = int(t["n_proposals"][f])
        assert n > 0, f
        pf = [nchw(t["fpn"][l][f:f + 1])[0] for l in range(4)]
        ref = o.box_features(pf, t["proposals"][f, :n, :4])                    # [n, 256, 7, 7] (bf16 values)
        got_ = t["box_features"][f, :n].float().view(n, 7, 7, 256).permute(0, 3, 1, 2)
        d = (got_ - ref).abs()
        same = float((d == 0).float().mean())
        ulp = float((d / ref.abs().clamp_min(1e-30)).max())
        print(f"frame {f}: ROIAlign bins identical {same:.6f}, max rel diff {ulp:.2e}")
        assert same > 0.999 and float((d - ref.abs() * 2 ** -7).max()) <= 1e-6
        got.append((n, same))
    return got


def check_box_head(run, frames=(0, 1)):
    """fc1 / fc2 / predictor from the GPU's box features."""
    o, t, K = run["oracle"], run["taps"], run["cfg"].num_classes
    got = []
    for f in frames:
        n = int(t["n_proposals"][f])
        cl, de = o.box_head(t["box_features"][f, :n].float().view(n, 7, 7, 256).permute(0, 3, 1, 2))
        g = t["head"][f, :n]
        ec, ed = float((g[:, :K + 1] - cl).abs().max()), float((g[:, K + 1:5 * K + 1] - de).abs().max())
        print(f"frame {f}: cls logits max|d| {ec:.2e} (max {float(cl.abs().max()):.2f}), deltas {ed:.2e}")
        assert ec < 3e-2 * max(1.0, float(cl.abs().max())) and ed < 3e-2 * max(0.1, float(de.abs().max()))
        got.append((ec, ed))
    return got


def check_inference_postprocess(run, min_checked):
    """Softmax / per-class decode / NMS / top 100 / postprocess / gate count from the GPU's head: identical instances.
    A frame with a class probability within 1e-5 of the threshold is skipped; at least `min_checked` frames are not."""
    from oracle.frcnn import OracleFrcnn, gate_persons
    o, t, out, K = run["oracle"], run["taps"], run["out"], run["cfg"].num_classes
    size = tuple(run["shapes"]["resized"])
    H, W = run["hw"]
    checked = 0
    for f in range(run["frames"].shape[0]):
        n = int(t["n_proposals"][f])
        cl, de = t["head"][f, :n, :K + 1], t["head"][f, :n, K + 1:5 * K + 1]
        e = torch.exp(cl - cl.max(1, keepdim=True).values)
        p = e / e.sum(1, keepdim=True)
        if bool(((p[:, :K] - run["cfg"].score_thresh).abs() < 1e-5).any()):
            print(f"frame {f}: a class probability within 1e-5 of the threshold: skipped")
            continue
        b, s, k = o.inference(cl, de, t["proposals"][f, :n, :4], size)
        m = int(t["n_pre_dets"][f])
        g = t["pre_dets"][f, :m]
        assert m == b.shape[0], (f, m, b.shape[0])
        assert torch.equal(g[:, 5].long(), k), f"frame {f}: classes / order differ"
        np.testing.assert_allclose(g[:, 4].numpy(), s.numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(g[:, :4].numpy(), b.numpy(), rtol=1e-5, atol=2e-3)
        fb, fs, fk = OracleFrcnn.postprocess(b, s, k, size, H, W)
        nd = int(out["n_dets"][f])
        assert nd == fb.shape[0]
        np.testing.assert_allclose(out["dets"][f, :nd, :4].numpy(), fb.numpy(), rtol=1e-5, atol=1e-3)
        assert torch.equal(out["dets"][f, :nd, 5].long(), fk)
        assert int(out["n_person"][f]) == gate_persons({"classes": fk, "scores": fs})
        pers = fk == 0
        for j in range(min(2, int(pers.sum()))):
            np.testing.assert_allclose(out["person"][f, j, :4].numpy(), fb[pers][j].numpy(), rtol=1e-5, atol=1e-3)
        checked += 1
        print(f"frame {f}: {m} instances, {int(out['n_person'][f])} persons > 0.5, classes {k[:8].tolist()}")
    assert checked >= min_checked, (checked, min_checked)
    return checked


def check_end_to_end(run, res, frames=(0, 1)):
    """The whole predictor from the frames: the oracle's instances (`res` of oracle_forward on the same `frames`) are
    found among the GPU's (same class, IoU > 0.9, score within 0.05) and the gate's person count agrees unless an
    oracle person score is within 0.05 of 0.5."""
    from oracle.frcnn import gate_persons
    out = run["out"]
    got = []
    for f, r in zip(frames, res):
        nd = int(out["n_dets"][f])
        g = out["dets"][f, :nd]
        top = min(20, len(r["scores"]))
        hit = 0
        for j in range(top):
            bo = r["boxes"][j]
            same = g[g[:, 5].long() == int(r["classes"][j])]
            if same.shape[0] == 0:
                continue
            x1 = torch.maximum(same[:, 0], bo[0]); y1 = torch.maximum(same[:, 1], bo[1])
            x2 = torch.minimum(same[:, 2], bo[2]); y2 = torch.minimum(same[:, 3], bo[3])
            inter = (x2 - x1).clamp_min(0) * (y2 - y1).clamp_min(0)
            iou = inter / ((same[:, 2] - same[:, 0]) * (same[:, 3] - same[:, 1]) + (bo[2] - bo[0]) * (bo[3] - bo[1]) - inter)
            ok = (iou > 0.9) & ((same[:, 4] - r["scores"][j]).abs() < 0.05)
            hit += int(bool(ok.any()))
        print(f"frame {f}: {hit}/{top} oracle instances matched; persons gpu {int(out['n_person'][f])} "
              f"oracle {gate_persons(r)}")
        assert hit >= 0.8 * top
        ps = r["scores"][r["classes"] == 0]
        if not bool(((ps - 0.5).abs() < 0.05).any()):
            assert int(out["n_person"][f]) == gate_persons(r)
        got.append((hit, top))
    return got


def check_roi_modes(sd, cfg, frames, device, chunk):
    """The default ROIAlign (separable per-bin cell weights, roi_align_sep_kernel) against torchvision's sample order
    (roi_align_kernel, vge_debug_set_roi_direct 1) and the separable kernel's own sample loop (2) on the same levels
    and proposals: mode 2 == mode 1 bit for bit, mode 0 identical but for rare 1-ulp bf16 differences."""
    import ctypes as C
    from vge import lib as L
    from vge.frcnn import FrcnnDetector
    F_, H, W = (int(v) for v in frames.shape[:3])
    fr = torch.from_numpy(frames).to(device)
    lib = L.load()
    lib.vge_debug_set_roi_direct.argtypes = [C.c_int]
    got = {}
    det = FrcnnDetector(sd, cfg, device=device, chunk=chunk, frame_hw=(H, W))
    try:
        for direct in (0, 1, 2):  # 2: the separable kernel's own sample loop (its branch for very wide bins)
            lib.vge_debug_set_roi_direct(direct)
            taps = det.make_taps(F_, H, W)
            det.detect(fr, taps=taps)
            torch.cuda.synchronize()
            got[direct] = (taps["box_features"].cpu(), taps["n_proposals"].cpu())
    finally:
        lib.vge_debug_set_roi_direct(0)
        det.close()
    assert torch.equal(got[0][1], got[1][1])
    assert torch.equal(got[2][0], got[1][0]), "the separable kernel's sample loop differs from roi_align_kernel"
    for f in range(F_):
        n = int(got[0][1][f])
        a, b = got[0][0][f, :n].float(), got[1][0][f, :n].float()
        d = (a - b).abs()
        same = float((d == 0).float().mean())
        print(f"frame {f}: {n} ROIs, bins identical {same:.6f}")
        assert n > 0 and same > 0.999 and float((d - b.abs() * 2 ** -7).max()) <= 1e-6


def check_stem_fused_vs_split(sd, cfg, frames, device, chunk):
    """The fused stem conv + ReLU + max pool (frcnn_stem_pool_kernel, default) against the stem conv kernel followed by
    the max-pool kernel (vge_debug_set_stem_split): P2..P6 agree to the conv kernel's own summation differences and the
    gate's person counts are the same."""
    import ctypes as C
    from vge import lib as L
    from vge.frcnn import FrcnnDetector
    F_, H, W = (int(v) for v in frames.shape[:3])
    fr = torch.from_numpy(frames).to(device)
    lib = L.load()
    lib.vge_debug_set_stem_split.argtypes = [C.c_int]
    got = {}
    det = FrcnnDetector(sd, cfg, device=device, chunk=chunk, frame_hw=(H, W))
    try:
        for split in (0, 1):
            lib.vge_debug_set_stem_split(split)
            taps = det.make_taps(F_, H, W)
            o = det.detect(fr, taps=taps)
            torch.cuda.synchronize()
            got[split] = ([p.float().cpu() for p in taps["fpn"]], o["n_person"].cpu())
    finally:
        lib.vge_debug_set_stem_split(0)
        det.close()
    for l, (a, b) in enumerate(zip(got[0][0], got[1][0])):
        rel = float((a - b).norm() / b.norm())
        print(f"P{l + 2}: fused vs split rel L2 {rel:.2e}, identical {float((a == b).float().mean()):.4f}")
        assert rel < 1e-2, (l, rel)
    assert torch.equal(got[0][1], got[1][1])
