"""The device WebP decoder (csrc/vge_webp.hip: vge_webp_decode_device) and the Python layer on it against the host
decoder vge_webp_decode_mem: exact equality of the per-frame statuses and, for accepted frames, of pixels, with canaries
around the output, the statuses, the workspace and every frame slot.  Files come from tests/webp_cases.py (the CPU
suite pins the host decoder to Pillow on the same files) and tests/golden/webp_golden.npz (Pillow-written files with
Pillow's frames)."""
import numpy as np
import pytest
import torch

from tests import webp_cases as WC
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 256   # canary bytes / elements around every device buffer


def lib():
    from vge import lib as L
    return L.load()


def device_decode(data, off, size, canvas, ws=None, fill=0x5A, tamper=None, spread=0, n_files=None):
    """Plan on the host, decode on the device -> (return code, status [frames], uint8 [frames, H, W, 3], whether every
    canary and the inputs survived, the workspace tensor, the descriptors).  tamper(descs, workspace bytes) may spoil
    the plan.  spread: bytes of canary put between the slots (the plan is re-laid with that gap)."""
    w, h = canvas
    _, descs, n, plan_st, _, ws_bytes = WC.host_plan_mem(data, off, size, canvas)
    slots = []
    if spread:
        pos = 0
        for k in range(n):
            d = descs[k]
            if d.plan_status:
                continue
            pos += spread
            d.slot_off = pos
            pos += lib().vge_webp_slot_bytes(d.w, d.h)
            slots.append((d.slot_off, pos))
        ws_bytes = max(16, pos + spread)
    if tamper is not None:
        tamper(descs, ws_bytes)
    d = torch.from_numpy(data).to(DEV)
    dd = torch.from_numpy(np.frombuffer(bytes(descs), np.uint8).copy()).to(DEV)
    frame = h * w * 3
    out = torch.full((n * frame + 2 * PAD,), fill, dtype=torch.uint8, device=DEV)
    st = torch.full((n + 2 * PAD,), -77, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.full((ws_bytes + 2 * PAD,), 0x5A, dtype=torch.uint8, device=DEV)
    assert ws.numel() == ws_bytes + 2 * PAD
    rc = lib().vge_webp_decode_device(d.data_ptr(), data.size, dd.data_ptr(), n, n,
                                      len(off) if n_files is None else n_files, w, h, ws[PAD:].data_ptr(), ws_bytes,
                                      out[PAD:].data_ptr(), st[PAD:].data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    intact = all(bool((t[:PAD] == v).all()) and bool((t[t.numel() - PAD:] == v).all())
                 for t, v in ((out, fill), (st, -77), (ws, 0x5A)))
    intact = intact and np.array_equal(d.cpu().numpy(), data) and bytes(dd.cpu().numpy()) == bytes(descs)
    if spread and tamper is None:   # whatever is no slot is still canary
        used = torch.zeros(ws_bytes, dtype=torch.bool, device=DEV)
        for a, b in slots:
            used[a:b] = True
        assert int((~used).sum()) >= spread
        intact = intact and bool((ws[PAD:PAD + ws_bytes][~used] == 0x5A).all())
    dev_st = st[PAD:PAD + n].cpu().numpy()
    rgb = out[PAD:PAD + n * frame].cpu().numpy().reshape(n, h, w, 3)
    return rc, dev_st, rgb, intact, ws, (descs, n, plan_st)


def assert_equals_host(files, canvas, what, gap=16, order=None, ws=None, spread=0):
    data, off, size = WC.pack(files, gap=gap, order=order)
    _, rows = WC.host_probe_mem(data, off, size)
    total = int(rows[:, 2].sum())
    _, hrgb, hst, _, _ = WC.host_decode_mem(data, off, size, canvas, total)
    rc, st, rgb, intact, ws, (descs, n, plan_st) = device_decode(data, off, size, canvas, ws=ws, spread=spread)
    assert rc == 0 and intact and n == total, what
    assert st.tolist() == hst.tolist(), (what, st.tolist(), hst.tolist())   # the device's own statuses are complete
    assert (st[plan_st != 0] == plan_st[plan_st != 0]).all()
    for i in range(total):
        if st[i] == 0:
            assert np.array_equal(rgb[i], hrgb[i]), (what, i, int((rgb[i] != hrgb[i]).any(-1).sum()))
    return st, rgb, ws, rows


@pytest.mark.parametrize("canvas", list(WC.by_canvas()), ids=lambda s: "%dx%d" % s)
def test_every_case_equals_the_host(canvas):
    """All cases of one canvas in one call, good and refused files side by side, every slot between canaries; the
    statuses are the ones the cases were built for.  A refused frame's pixels keep the fill: nobody writes them."""
    group = WC.by_canvas()[canvas]
    st, rgb, _, rows = assert_equals_host([c.data for c in group], canvas, canvas, spread=48)
    first = np.concatenate([[0], np.cumsum(rows[:, 2])])
    for i, c in enumerate(group):
        s = st[first[i]:first[i + 1]]
        if c.canvas != canvas:
            continue   # a file whose header gives no canvas rides along: the host's verdict, checked above
        bad = len(s) if c.accept else (c.bad_frame or 0)
        assert (s[:bad] == 0).all() and (s[bad:] == c.expect).all(), (c.name, s.tolist())
        assert (rgb[first[i] + bad:first[i + 1]] == 0x5A).all(), c.name


def test_golden_files_equal_their_stored_pixels():
    gold = np.load(GOLDEN / "webp_golden.npz")
    names = sorted(k[5:] for k in gold.files if k.startswith("webp/"))
    assert len(names) >= 6
    for name in names:
        want = gold[f"rgb/{name}"]
        canvas = (want.shape[2], want.shape[1])
        st, rgb, _, _ = assert_equals_host([gold[f"webp/{name}"].tobytes()], canvas, name, gap=3)
        assert st.tolist() == [0] * len(want) and np.array_equal(rgb, want), name


def test_batch_packing_order_and_a_reused_workspace():
    """Files of 8, 0, 6, 1 and 3 frames, one of another size and one cut short, packed with odd gaps and out of order;
    the same workspace, as the first call left it, gives the same result on the second."""
    by_name = {c.name: c for c in WC.cases()}
    files = [by_name[n].data for n in ("anim_hand", "cut_2", "anim_alpha_rules", "shape_64x66", "bounds")]
    order = [4, 2, 0, 3, 1]
    st1, rgb1, ws, rows = assert_equals_host(files, (40, 30), "first", gap=5, order=order)
    st2, rgb2, _, _ = assert_equals_host(files, (40, 30), "reused", gap=5, order=order, ws=ws)
    assert rows[:, 2].tolist() == [8, 0, 6, 1, 3]
    assert st1.tolist() == st2.tolist() == [0] * 14 + [WC.ERR_SHAPE] + [0] + [WC.ERR_BOUNDS] * 2
    ok = st1 == 0
    assert np.array_equal(rgb1[ok], rgb2[ok])


def test_descriptors_that_do_not_fit_are_refused_by_the_kernels():
    """Every way a descriptor can point outside what the host passed: the frame gets VGE_WEBP_ERR_ARG (or, with nobody
    to report to, is left alone), nothing outside the buffers is touched and the neighbours decode."""
    canvas = (17, 9)
    good = next(c.data for c in WC.cases() if c.name == "pred_11")
    n = 16
    data, off, size = WC.pack([good] * n, gap=8)
    _, hrgb, hst, _, _ = WC.host_decode_mem(data, off, size, canvas, n)
    assert hst.tolist() == [0] * n

    def tamper(descs, ws_bytes):
        descs[0].slot_off = ws_bytes - 16
        descs[1].slot_off += 4
        descs[2].slot_off = ws_bytes
        descs[3].w += 1
        descs[4].file_off = -1
        descs[5].pay_off = descs[5].file_bytes - 5
        descs[6].x = 1
        descs[7].pay_bytes = -1
        descs[8].file_bytes = 1 << 28
        descs[9].slot_off = -16
        descs[10].h = 0
        descs[11].frame = n       # nobody's frame: no status to set, no pixels to write
        descs[12].pay_off = -1
        descs[13].pay_bytes = 20  # a payload cut short: the stream ends early
        descs[14].w, descs[14].h = 9, 17   # fits the workspace, not the stream's header

    rc, st, rgb, intact, _, _ = device_decode(data, off, size, canvas, tamper=tamper)
    assert rc == 0 and intact
    assert st.tolist() == [1] * 11 + [0, 1, WC.ERR_IO, 1, 0]
    assert (rgb[:15] == 0x5A).all() and np.array_equal(rgb[15:], hrgb[15:])


def test_descriptor_orders_the_plan_does_not_emit_are_refused_by_the_kernels():
    """The compose kernel finds a file's frames by the order of the descriptors.  A run that does not start at index 0,
    an owner outside the call's files, owners out of order and an unused slot in front of a file's frames: every frame
    that cannot be composed gets VGE_WEBP_ERR_ARG, none keeps status 0 without pixels, and the other files decode."""
    by_name = {c.name: c for c in WC.cases()}
    files = [by_name[n].data for n in ("anim_hand", "anim_alpha_rules", "bounds")]
    data, off, size = WC.pack(files, gap=8)
    _, hrgb, hst, _, _ = WC.host_decode_mem(data, off, size, (40, 30), 17)
    assert hst.tolist() == [0] * 15 + [WC.ERR_BOUNDS] * 2

    def headless(descs, ws_bytes):
        assert [descs[k].index for k in range(8, 12)] == [0, 1, 2, 3]
        descs[8].index = 1       # the second file's run starts at index 1: 8 is no head, 9 starts a run of its own
        descs[14].file = 7       # an owner the call does not have

    def out_of_order(descs, ws_bytes):
        for k in range(17):
            descs[k].file = (1, 0, 2)[descs[k].file]   # the search for file 0 lands on the first run, which is file 1's

    def unused_head(descs, ws_bytes):
        descs[8].frame = -1      # nobody to report to; the later frames of the file are deltas on it

    def too_few_files(descs, ws_bytes):
        pass

    B = WC.ERR_BOUNDS
    for tamper, n_files, want in ((headless, 3, [0] * 8 + [1] * 6 + [1] + [B, B]),
                                  (out_of_order, 3, [1] * 14 + [0, B, B]),   # neither search lands on its run's head
                                  (unused_head, 3, [0] * 9 + [1] * 5 + [0, B, B]),
                                  (too_few_files, 2, [0] * 14 + [1, B, B])):
        rc, st, rgb, intact, _, _ = device_decode(data, off, size, (40, 30), tamper=tamper, n_files=n_files)
        assert rc == 0 and intact, tamper.__name__
        assert st.tolist() == want, (tamper.__name__, st.tolist())
        for k in range(17):
            if tamper is unused_head and k == 8:
                assert (rgb[k] == 0x5A).all()
            elif want[k] == 0:
                assert np.array_equal(rgb[k], hrgb[k]), (tamper.__name__, k)
            else:
                assert (rgb[k] == 0x5A).all(), (tamper.__name__, k)


def test_bad_arguments_are_refused_before_any_launch():
    L = lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    st = torch.full((4,), -5, dtype=torch.int32, device=DEV)
    p, s = buf.data_ptr(), st.data_ptr()
    ok = dict(data=p, data_bytes=1024, descs=p + 1024, n_descs=1, n_frames=1, n_files=1, w=4, h=4, ws=p + 3072,
              ws_bytes=512, rgb=p + 3600, status=s, stream=None)
    for change in (dict(n_descs=-1), dict(n_files=-1), dict(n_frames=-1), dict(data_bytes=-1), dict(ws_bytes=-1),
                   dict(w=0), dict(h=0), dict(w=16385), dict(status=None), dict(status=s + 2), dict(data=None),
                   dict(descs=None), dict(descs=p + 1028), dict(ws=None), dict(ws=p + 3080), dict(rgb=None)):
        a = dict(ok, **change)
        rc = L.vge_webp_decode_device(a["data"], a["data_bytes"], a["descs"], a["n_descs"], a["n_frames"], a["n_files"],
                                      a["w"], a["h"], a["ws"], a["ws_bytes"], a["rgb"], a["status"], a["stream"])
        assert rc == 1 and b"vge_webp_decode_device" in L.vge_last_error(), change
    torch.cuda.synchronize()
    assert (st == -5).all() and not buf.any()


def test_mutations_on_the_device_equal_the_host():
    """The seeded byte mutations of tests/webp_cases.py, grouped by the canvas the probe reads: the kernels end on every
    one of them with the host decoder's statuses and, where a frame is accepted, its pixels."""
    muts = WC.mutations(300)
    groups = {}
    for name, blob in muts:
        data, off, size = WC.pack([blob])
        _, rows = WC.host_probe_mem(data, off, size)
        w, h = int(rows[0, 0]), int(rows[0, 1])
        if int(rows[0, 2]) > 0 and 0 < w <= 256 and 0 < h <= 256:
            groups.setdefault((w, h), []).append(blob)
    assert sum(len(g) for g in groups.values()) >= 150
    accepted = 0
    for canvas, blobs in groups.items():
        st, _, _, _ = assert_equals_host(blobs, canvas, canvas, gap=4)
        accepted += int((st == 0).sum())
    assert accepted >= 30


@pytest.fixture(scope="module")
def webp_tree(tmp_path_factory):
    """Two WebP videos written by this suite's writer from 128 x 128 frames: one whole (5 frames), one whose fourth
    frame's stream is cut short (3 frames stand), and a file that is no WebP at all."""
    root = tmp_path_factory.mktemp("webp_tree")
    d = root / "frames" / "Soccer"
    d.mkdir(parents=True)
    vids = []
    for v in range(2):
        frames = []
        for f in range(5):
            rect = (0, 0, 128, 128) if f == 0 else (8 * f, 4 * f, 96, 100)
            rgb = WC.picture(rect[2], rect[3], 10 * v + f)
            alpha = 255 if f == 0 else np.where(np.add.outer(np.arange(rect[3]), np.arange(rect[2])) % 7 < 3, 0, 255)
            pay = WC.vp8l(WC.rgb_to_argb(rgb, alpha), [(WC.PREDICTOR, 4, 11), (WC.GREEN,)], lz=True, cache_bits=6)
            if v == 1 and f == 3:
                pay = pay[:len(pay) // 2]
            frames.append(WC.anmf(rect[0], rect[1], rect[2], rect[3], pay, blend=f != 2, dispose=f == 1))
        p = d / f"v_w_{v:02d}.webp"
        p.write_bytes(WC.animation((128, 128), frames))
        vids.append(p)
    (d / "notes.txt").write_bytes(b"not a video")
    return root, vids


def test_loaders_agree_between_host_and_device(webp_tree, tmp_path):
    from vge import frames as FR
    _, vids = webp_tree
    host = FR.load_videos(vids, device=DEV, entropy="host")
    dev = FR.load_videos(vids, device=DEV, entropy="device")
    assert [k.tolist() for _, k in host] == [[0, 1, 2, 3, 4], [0, 1, 2]]
    for (hf, hk), (df, dk) in zip(host, dev):
        assert hk.tolist() == dk.tolist() and hf.device.type == "cuda" and torch.equal(hf, df)
        assert tuple(hf.shape[1:]) == (128, 128, 3)
    one_h, kept_h = FR.load_frames(vids[1], device=DEV, entropy="host")
    one_d, kept_d = FR.load_frames(vids[1], device=DEV, entropy="device")
    assert kept_h.tolist() == kept_d.tolist() == [0, 1, 2] and torch.equal(one_h, one_d)
    cpu, kept_c = FR.load_frames(vids[1], device="cpu")
    assert kept_c.tolist() == [0, 1, 2] and torch.equal(cpu, one_d.cpu())
    raw = [v.read_bytes() for v in vids]
    data, off, size = WC.pack(raw)
    offsets = np.concatenate([off, [off[-1] + size[-1]]])
    packed = FR.decode_webps(torch.from_numpy(data), offsets, device=DEV)
    for (pf, pk), (hf, hk) in zip(packed, host):
        assert pk.tolist() == hk.tolist() and torch.equal(pf, hf)
    with pytest.raises(ValueError, match="host memory"):
        FR.decode_webps(torch.from_numpy(data).to(DEV), offsets)
    # a folder of still frames, both routes
    folder = tmp_path / "stills"
    folder.mkdir()
    want = [WC.picture(33, 21, 70 + k) for k in range(3)]
    for k, rgb in enumerate(want):
        (folder / f"{k:03d}.webp").write_bytes(WC.still(WC.all_features(rgb, seed=k)))
    for entropy in ("host", "device"):
        fr, kept = FR.load_frames(folder, device=DEV, entropy=entropy)
        assert kept.tolist() == [0, 1, 2] and np.array_equal(fr.cpu().numpy(), np.stack(want)), entropy
    by_name = {c.name: c for c in WC.cases()}
    (tmp_path / "groups.webp").write_bytes(by_name["groups_257"].data)
    for entropy in ("host", "device"):   # what only the decoders see is still refused by name
        with pytest.raises(FR.UnsupportedWebpError, match="groups"):
            FR.load_frames(tmp_path / "groups.webp", device=DEV, entropy=entropy)


class FullFrameDetector:
    """The gate detector's interface with one person box over the whole frame (the detector has its own tests)."""
    def detect(self, fr):
        F, H, W = (int(v) for v in fr.shape[:3])
        person = torch.zeros(F, 1, 5, device=fr.device)
        person[:, 0, :4] = torch.tensor([0.0, 0.0, W, H], device=fr.device)
        return {"person": person, "n_person": torch.ones(F, dtype=torch.int32, device=fr.device)}


@pytest.mark.parametrize("quality", [None, 95])
def test_tree_driver_on_webp_videos(webp_tree, tmp_path, quality):
    """extract_frame_tree(frame_format="webp") writes what extract_videos writes for the same decoded frames, with and
    without the JPEG round trip in front of the models."""
    from vge import dwpose as D, hmr as H, synth
    from vge.extract import extract_frame_tree, extract_videos
    from vge.frames import load_frames
    root, vids = webp_tree
    hcfg = H.HmrConfig(embed_dim=256, depth=1, heads=4, mlp_dim=256, dec_dim=256, dec_depth=1, dec_heads=4,
                       dec_mlp=256, tok_num=4, tok_classes=256, tok_code_dim=256)
    hmr = H.HmrExtractor(synth.make_hmr_state_dict(hcfg), hcfg, device=DEV, max_frames=8)
    ycfg = D.YoloxConfig(in_size=128, width=16, depth=1, head_ch=64)
    pcfg = D.RtmposeConfig(in_h=128, in_w=96, stem_ch=16, stage_ch=(32, 64, 128, 256), stage_blocks=(1, 1, 1, 1))
    wb = D.Wholebody(D.YoloxDetector(synth.make_yolox_state_dict(ycfg), ycfg, device=DEV, chunk=8),
                     D.DwposeExtractor(synth.make_rtmpose_state_dict(pcfg), pcfg, device=DEV, max_instances=16))
    s = extract_frame_tree(hmr, wb, FullFrameDetector(), root / "frames", tmp_path / "meshes", tmp_path / "kps",
                           tmp_path / "logs", device=DEV, frame_format="webp", jpeg_quality=quality, entropy="device")
    assert s["Soccer"]["single"] == ["v_w_00", "v_w_01"] and not s["Soccer"]["errors"]
    loaded = [load_frames(p, device=DEV) for p in vids]
    assert [k.tolist() for _, k in loaded] == [[0, 1, 2, 3, 4], [0, 1, 2]]
    ref = extract_videos(hmr, wb, FullFrameDetector(), [(p.stem, fr) for p, (fr, _) in zip(vids, loaded)],
                         tmp_path / "ref_meshes", tmp_path / "ref_kps", jpeg_quality=quality)
    for p, (fr, kept) in zip(vids, loaded):
        z = np.load(tmp_path / "meshes" / "Soccer" / f"{p.stem}.npz")
        r = np.load(ref[p.stem])
        np.testing.assert_array_equal(z["frame_idx"], kept[r["frame_idx"]])   # indices into the file's frames
        for k in ("pose", "betas", "global_orient", "vit"):
            np.testing.assert_array_equal(z[k], r[k])
        np.testing.assert_array_equal(np.load(tmp_path / "kps" / "Soccer" / p.stem / "keypoints.npy"),
                                      np.load(tmp_path / "ref_kps" / p.stem / "keypoints.npy"))
