"""The device APNG decoder (csrc/vge_apng.hip: vge_apng_decode_device) and the Python layer on it against the host
decoder vge_apng_decode_mem: exact equality of the per-frame statuses and, for accepted frames, of pixels, with canaries
around the output, the statuses, the workspace and every run and slot.  Files come from tests/apng_cases.py (the CPU
suite pins the host decoder to Pillow's pixels on the same files) and tests/golden/apng_golden.npz (Pillow-written files
with Pillow's frames)."""
import numpy as np
import pytest
import torch

from tests import apng_cases as AC
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 256   # canary bytes / elements around every device buffer
COMPOSE_LANES = 256   # csrc/vge_gather.h WIDE: canvas pixels per compose workgroup


def lib():
    from vge import lib as L
    return L.load()


def records(n):
    """Bytes at the start of the workspace that the inflate kernel keeps for the Adler kernel."""
    return (n * 8 + 15) & ~15


def device_decode(data, off, size, layout, ws=None, fill=0x5A, tamper=None, spread=0, n_files=None):
    """Plan on the host, decode on the device -> (return code, status [frames], uint8 [frames, H, W, 3], whether every
    canary and the inputs survived, the workspace tensor, (descs, n, plan statuses)).  tamper(descs, segs, workspace
    bytes) may spoil the plan.  spread: bytes of canary put between all the plan's runs and slots (the plan is re-laid
    with that gap), so that every run and slot has a canary on both sides."""
    w, h, ct = layout
    _, descs, n, segs, n_segs, plan_st, _, ws_bytes = AC.host_plan_mem(data, off, size, layout)
    if spread:
        pos = records(n)
        for k in range(n):
            d = descs[k]
            if d.plan_status:
                continue
            pos += spread
            for j in range(n_segs):
                if segs[j].desc == k:
                    segs[j].dst_off += pos - d.gat_off
            d.gat_off = pos
            pos = (pos + d.gat_bytes + spread + 15) & ~15
            d.slot_off = pos
            pos += (d.raw_bytes + 3) & ~3
        ws_bytes = max(16, (pos + spread + 15) & ~15)
    if tamper is not None:
        tamper(descs, segs, ws_bytes)
    d = torch.from_numpy(data).to(DEV)
    dd = torch.from_numpy(np.frombuffer(bytes(descs), np.uint8).copy()).to(DEV)
    sd = torch.from_numpy(np.frombuffer(bytes(segs), np.uint8).copy()).to(DEV)
    frame = h * w * 3
    out = torch.full((n * frame + 2 * PAD,), fill, dtype=torch.uint8, device=DEV)
    st = torch.full((n + 2 * PAD,), -77, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.full((ws_bytes + 2 * PAD,), 0x5A, dtype=torch.uint8, device=DEV)
    assert ws.numel() == ws_bytes + 2 * PAD
    rc = lib().vge_apng_decode_device(d.data_ptr(), data.size, dd.data_ptr(), n, sd.data_ptr(), n_segs, n,
                                      len(off) if n_files is None else n_files, w, h, ct, ws[PAD:].data_ptr(), ws_bytes,
                                      out[PAD:].data_ptr(), st[PAD:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    intact = all(bool((t[:PAD] == v).all()) and bool((t[t.numel() - PAD:] == v).all())
                 for t, v in ((out, fill), (st, -77), (ws, 0x5A)))
    intact = intact and np.array_equal(d.cpu().numpy(), data) and bytes(dd.cpu().numpy()) == bytes(descs)
    if spread and tamper is None:   # whatever is neither a record, a gathered run nor a slot is still canary
        used = np.zeros(ws_bytes, bool)
        used[:records(n)] = True
        for k in range(n):
            if not descs[k].plan_status:
                used[descs[k].gat_off:descs[k].gat_off + descs[k].gat_bytes] = True
                used[descs[k].slot_off:descs[k].slot_off + ((descs[k].raw_bytes + 3) & ~3)] = True
        assert (~used).sum() >= spread
        intact = intact and bool((ws[PAD:PAD + ws_bytes].cpu().numpy()[~used] == 0x5A).all())
    dev_st = st[PAD:PAD + n].cpu().numpy()
    rgb = out[PAD:PAD + n * frame].cpu().numpy().reshape(n, h, w, 3)
    return rc, dev_st, rgb, intact, ws, (descs, n, plan_st)


def assert_equals_host(files, layout, what, gap=16, order=None, ws=None, spread=0):
    data, off, size = AC.pack(files, gap=gap, order=order)
    _, rows = AC.host_probe_mem(data, off, size)
    total = int(rows[:, 5].sum())
    _, hrgb, hst, _, _ = AC.host_decode_mem(data, off, size, layout, total)
    rc, st, rgb, intact, ws, (descs, n, plan_st) = device_decode(data, off, size, layout, ws=ws, spread=spread)
    assert rc == 0 and intact and n == total, what
    assert st.tolist() == hst.tolist(), (what, st.tolist(), hst.tolist())   # the device's own statuses are complete
    assert (st[plan_st != 0] == plan_st[plan_st != 0]).all()
    for i in range(total):
        if st[i] == 0:
            assert np.array_equal(rgb[i], hrgb[i]), (what, i)
    return st, rgb, ws, rows


@pytest.mark.parametrize("layout", list(AC.by_layout()), ids=lambda s: "%dx%d_ct%d" % s)
def test_every_case_equals_the_host(layout):
    """All cases of one layout in one call, good and refused files side by side, every run and slot between canaries;
    the statuses are the ones the cases were built for and the pixels are the model's (which the CPU suite pins to
    Pillow's).  A refused frame's pixels keep the fill: nobody writes them."""
    group = AC.by_layout()[layout]
    st, rgb, _, rows = assert_equals_host([c.data for c in group], layout, layout, spread=48)
    first = np.concatenate([[0], np.cumsum(rows[:, 5])])
    for i, c in enumerate(group):
        s = st[first[i]:first[i + 1]]
        assert len(s) == c.n_frames, c.name
        bad = len(s) if c.accept else c.bad_frame
        assert (s[:bad] == 0).all() and (s[bad:] == c.expect).all(), (c.name, s.tolist())
        assert (rgb[first[i] + bad:first[i + 1]] == 0x5A).all(), c.name
        if bad:
            assert np.array_equal(rgb[first[i]:first[i] + bad], c.want[:bad]), c.name


def test_cases_cover_the_kernels_ground():
    band = lib().vge_png_decode_device_band_rows()
    accepted = [c for c in AC.cases() if c.accept]
    rects = {}
    for c in accepted:
        data, off, size = AC.pack([c.data])
        _, descs, nd, _, _, _, _, _ = AC.host_plan_mem(data, off, size, c.layout)
        rects[c.name] = [(descs[k].x, descs[k].y, descs[k].w, descs[k].h, descs[k].dispose_op, descs[k].blend_op)
                         for k in range(nd)]
    # a rectangle that is no whole frame and spans more than one unfilter band, with a ragged last band
    assert any(band < h < 2 * band and (w, h) != c.layout[:2] for c in accepted for (_, _, w, h, _, _) in rects[c.name])
    assert (9, 70) in {(w, h) for (_, _, w, h, _, _) in rects["bands"]}
    # canvases of more than one compose workgroup with a ragged tail, and of a single lane
    pixels = {c.layout[0] * c.layout[1] for c in accepted}
    assert any(p > 2 * COMPOSE_LANES and p % COMPOSE_LANES for p in pixels) and 1 in pixels
    assert 256 * 256 in pixels   # the blend table: every alpha against every value
    # rectangles at the corner, flush with the far edges, 1 x 1, one column wide, the whole canvas
    r37 = [r for c in accepted if c.layout[:2] == (37, 29) for r in rects[c.name]]
    assert any(r[:2] == (0, 0) and r[2:4] != (37, 29) for r in r37)
    assert any(r[0] + r[2] == 37 and r[1] + r[3] == 29 and r[:2] != (0, 0) for r in r37)
    assert any(r[2:4] == (1, 1) for r in r37) and any(r[2] == 1 and r[3] > 1 for r in r37)
    assert any(r[:4] == (0, 0, 37, 29) for r in r37)
    # each disposal followed by each blend, for every colour type; PREVIOUS on frame 0; two PREVIOUS in a row
    for ct in (0, 2, 4, 6):
        rs = rects[f"ops_ct{ct}"]
        assert {(a[4], b[5]) for a, b in zip(rs, rs[1:])} >= {(d, b) for d in (0, 1, 2) for b in (0, 1)}
    assert rects["prev_first"][0][4] == 2
    assert any(a[4] == 2 and b[4] == 2 for a, b in zip(rects["prev_twice"], rects["prev_twice"][1:]))
    assert {c.layout[2] for c in accepted} == {0, 2, 4, 6}
    # every filter type in sub-rectangle frames; chunks cut into pieces, an fdAT of its sequence number alone
    filters = set()
    for f in AC.ops_frames(6)[1:]:
        filters |= set(f.filters)
    assert filters == {0, 1, 2, 3, 4}
    raw = AC.by_name()["split_chunks"].data
    assert raw.count(b"fdAT") > 10 and b"\x00\x00\x00\x04fdAT" in raw and b"\x00\x00\x00\x00IDAT" in raw
    refused = {c.name: c.expect for c in AC.cases() if not c.accept}
    assert {"seq_fdat", "seq_fctl", "fctl_no_data", "rect_outside", "first_smaller", "corrupt_deflate", "wrong_adler",
            "filter_5", "truncated", "other_canvas", "interlaced", "depth16", "palette"} <= set(refused)
    assert all(len(c.data) < (1 << 18) for c in AC.cases())


def test_golden_files_equal_their_stored_pixels():
    gold = np.load(GOLDEN / "apng_golden.npz")
    names = sorted(k[5:] for k in gold.files if k.startswith("apng/"))
    assert len(names) >= 5
    for name in names:
        want = gold[f"rgb/{name}"]
        layout = (want.shape[2], want.shape[1], 6 if name.startswith("rgba") else 2)
        st, rgb, _, _ = assert_equals_host([gold[f"apng/{name}"].tobytes()], layout, name, gap=3)
        assert st.tolist() == [0] * len(want) and np.array_equal(rgb, want), name


def test_batch_packing_order_and_a_reused_workspace():
    """Four files of 3, 4, 4 and 3 frames, a file of another canvas and one that is no PNG in one call, packed with odd
    gaps and in reverse order; the same workspace, as the first call left it, gives the same result on the second."""
    by_name = AC.by_name()
    names = ("prev_first", "seq_fdat", "default_image", "other_canvas", "not_png", "bg_over_alpha0")
    files = [by_name[n].data for n in names]
    order = list(range(len(files)))[::-1]
    st1, rgb1, ws, rows = assert_equals_host(files, (37, 29, 6), "first", gap=5, order=order)
    st2, rgb2, _, _ = assert_equals_host(files, (37, 29, 6), "reused", gap=5, order=order, ws=ws)
    assert rows[:, 5].tolist() == [3, 4, 4, 2, 0, 3]
    assert st1.tolist() == st2.tolist() == [0] * 3 + [0, 0, AC.ERR_IO, AC.ERR_IO] + [0] * 4 + [AC.ERR_SHAPE] * 2 + [0] * 3
    ok = st1 == 0
    assert np.array_equal(rgb1[ok], rgb2[ok])


def test_descriptors_and_segments_that_do_not_fit_are_refused_by_the_kernels():
    """Every way a descriptor or a segment can point outside what the host passed: the frame gets VGE_APNG_ERR_ARG (or,
    with nobody to report to, is left alone), nothing outside the buffers is touched and the neighbours decode."""
    layout = (37, 29, 2)
    good = AC.by_name()["still"].data
    n = 16
    data, off, size = AC.pack([good] * n, gap=8)
    _, hrgb, hst, _, _ = AC.host_decode_mem(data, off, size, layout, n)
    assert hst.tolist() == [0] * n

    def tamper(descs, segs, ws_bytes):
        descs[0].gat_off = ws_bytes - 1
        descs[1].slot_off += 4
        descs[2].slot_off = ws_bytes
        descs[3].w += 1
        descs[4].file_off = -1
        descs[5].raw_bytes += 1
        descs[6].x = 1
        descs[7].color_type = 6
        descs[8].h = 0
        descs[9].gat_off = 0       # inside the records at the start of the workspace
        descs[10].gat_bytes = 1 << 28
        descs[11].frame = n        # nobody's frame: no status to set, no pixels to write
        descs[12].y = -1

    def tamper_segs(descs, segs, ws_bytes):
        def first(k):   # the first segment of frame k
            return next(s for s in segs if s.desc == k)
        first(0).src_off = descs[0].file_off - 1
        first(1).bytes = 1 << 40
        first(2).dst_off = descs[2].gat_off + descs[2].gat_bytes
        first(4).dst_off = descs[4].gat_off - 1
        first(3).desc = n          # nobody's segment: frame 3 inflates a run that begins with the 0x5A fill

    rc, st, rgb, intact, _, _ = device_decode(data, off, size, layout, tamper=tamper)
    assert rc == 0 and intact
    assert st.tolist() == [1] * 11 + [0, 1] + [0] * 3
    assert (rgb[:13] == 0x5A).all() and np.array_equal(rgb[13:], hrgb[13:])
    rc, st, rgb, intact, _, _ = device_decode(data, off, size, layout, tamper=tamper_segs)
    assert rc == 0 and intact
    assert st.tolist() == [1, 1, 1, AC.ERR_IO, 1] + [0] * 11
    assert (rgb[:5] == 0x5A).all() and np.array_equal(rgb[5:], hrgb[5:])


def test_descriptor_orders_the_plan_does_not_emit_are_refused_by_the_kernels():
    """The compose kernel finds a file's frames by the order of the descriptors.  A run that does not start at index 0,
    an owner outside the call's files, owners out of order and an unused slot in front of a file's frames: every frame
    that cannot be composed gets VGE_APNG_ERR_ARG, none keeps status 0 without pixels, and the other files decode."""
    by_name = AC.by_name()
    files = [by_name[n].data for n in ("prev_twice", "prev_first", "partial_trailer")]
    layout = (37, 29, 6)
    data, off, size = AC.pack(files, gap=8)
    _, hrgb, hst, _, _ = AC.host_decode_mem(data, off, size, layout, 9)
    assert hst.tolist() == [0] * 9

    def headless(descs, segs, ws_bytes):
        assert [descs[k].index for k in range(4, 7)] == [0, 1, 2]
        descs[4].index = 1       # the second file's run starts at index 1: 4 is no head, 5 starts a run of its own
        descs[7].file = 7        # an owner the call does not have; 8 is then a run that starts at index 1

    def out_of_order(descs, segs, ws_bytes):
        for k in range(9):
            descs[k].file = (1, 0, 2)[descs[k].file]   # neither search lands on the head of the first two runs

    def unused_head(descs, segs, ws_bytes):
        descs[4].frame = -1      # nobody to report to; the later frames of the file are deltas on it

    def too_few_files(descs, segs, ws_bytes):
        pass

    for tamper, n_files, want in ((headless, 3, [0] * 4 + [1] * 5), (out_of_order, 3, [1] * 7 + [0] * 2),
                                  (unused_head, 3, [0] * 5 + [1] * 2 + [0] * 2), (too_few_files, 2, [0] * 7 + [1] * 2)):
        rc, st, rgb, intact, _, _ = device_decode(data, off, size, layout, tamper=tamper, n_files=n_files)
        assert rc == 0 and intact, tamper.__name__
        assert st.tolist() == want, (tamper.__name__, st.tolist())
        for k in range(9):
            if tamper is unused_head and k == 4:
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
    ok = dict(data=p, data_bytes=1024, descs=p + 1024, n_descs=1, segs=p + 2048, n_segs=1, n_frames=1, n_files=1,
              w=4, h=4, ct=6, ws=p + 3072, ws_bytes=512, rgb=p + 3600, status=s, stream=None)
    for change in (dict(n_descs=-1), dict(n_files=-1), dict(n_segs=-1), dict(n_segs=1 << 31), dict(n_frames=-1),
                   dict(data_bytes=-1), dict(ws_bytes=-1), dict(w=0), dict(h=0), dict(ct=3), dict(ct=1), dict(ct=-1),
                   dict(status=None), dict(status=s + 2), dict(data=None), dict(descs=None), dict(descs=p + 1028),
                   dict(segs=None), dict(segs=p + 2052), dict(ws=None), dict(ws=p + 3080), dict(rgb=None)):
        a = dict(ok, **change)
        rc = L.vge_apng_decode_device(a["data"], a["data_bytes"], a["descs"], a["n_descs"], a["segs"], a["n_segs"],
                                      a["n_frames"], a["n_files"], a["w"], a["h"], a["ct"], a["ws"], a["ws_bytes"],
                                      a["rgb"], a["status"], a["stream"])
        assert rc == 1 and b"vge_apng_decode_device" in L.vge_last_error(), change
    torch.cuda.synchronize()
    assert (st == -5).all() and not buf.any()


@pytest.fixture(scope="module")
def apng_tree(tmp_path_factory):
    """Two APNG videos written by this suite's writer from 128 x 128 RGBA frames: one whole (5 frames), one cut inside
    its fourth frame (3 frames stand), under <root>/frames/Soccer as v_p_00.png and v_p_01.apng."""
    root = tmp_path_factory.mktemp("apng_tree")
    d = root / "frames" / "Soccer"
    d.mkdir(parents=True)
    vids = []
    for v in range(2):
        frames = []
        for f in range(5):
            rect = (0, 0, 128, 128) if f == 0 else (8 * f, 4 * f, 96, 100)
            frames.append(AC.sub(300 + 10 * v + f, rect, 6, dispose=(0, 1, 2, 0, 1)[f], blend=(0, 1, 1, 0, 1)[f],
                                 split=4096))
        chs = AC.chunks((128, 128), 6, frames)
        data = AC.assemble(chs)
        if v == 1:
            data = data[:len(AC.assemble(chs[:AC.nth(chs, b"fcTL", 3) + 1])) + 8 + 100]
        path = d / ("v_p_00.png", "v_p_01.apng")[v]
        path.write_bytes(data)
        vids.append(path)
    return root, vids


def test_loaders_agree_between_host_and_device(apng_tree):
    from vge import frames as FR
    _, vids = apng_tree
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
    data, off, size = AC.pack(raw)
    offsets = np.concatenate([off, [off[-1] + size[-1]]])
    for entropy in ("host", "device", None):
        packed = FR.decode_apngs(torch.from_numpy(data), offsets, device=DEV, entropy=entropy)
        for (pf, pk), (hf, hk) in zip(packed, host):
            assert pk.tolist() == hk.tolist() and torch.equal(pf, hf)
    with pytest.raises(ValueError, match="host memory"):
        FR.decode_apngs(torch.from_numpy(data).to(DEV), offsets)


class FullFrameDetector:
    """The gate detector's interface with one person box over the whole frame (the detector has its own tests)."""
    def detect(self, fr):
        F, H, W = (int(v) for v in fr.shape[:3])
        person = torch.zeros(F, 1, 5, device=fr.device)
        person[:, 0, :4] = torch.tensor([0.0, 0.0, W, H], device=fr.device)
        return {"person": person, "n_person": torch.ones(F, dtype=torch.int32, device=fr.device)}


def test_tree_driver_on_apng_videos(apng_tree, tmp_path):
    """extract_frame_tree(frame_format="apng") on the device route writes what extract_videos writes for the same
    decoded frames."""
    from vge import dwpose as D, hmr as H, synth
    from vge.extract import extract_frame_tree, extract_videos
    from vge.frames import load_frames
    root, vids = apng_tree
    hcfg = H.HmrConfig(embed_dim=256, depth=1, heads=4, mlp_dim=256, dec_dim=256, dec_depth=1, dec_heads=4,
                       dec_mlp=256, tok_num=4, tok_classes=256, tok_code_dim=256)
    hmr = H.HmrExtractor(synth.make_hmr_state_dict(hcfg), hcfg, device=DEV, max_frames=8)
    ycfg = D.YoloxConfig(in_size=128, width=16, depth=1, head_ch=64)
    pcfg = D.RtmposeConfig(in_h=128, in_w=96, stem_ch=16, stage_ch=(32, 64, 128, 256), stage_blocks=(1, 1, 1, 1))
    wb = D.Wholebody(D.YoloxDetector(synth.make_yolox_state_dict(ycfg), ycfg, device=DEV, chunk=8),
                     D.DwposeExtractor(synth.make_rtmpose_state_dict(pcfg), pcfg, device=DEV, max_instances=16))
    s = extract_frame_tree(hmr, wb, FullFrameDetector(), root / "frames", tmp_path / "meshes", tmp_path / "kps",
                           tmp_path / "logs", device=DEV, frame_format="apng", entropy="device")
    assert s["Soccer"]["single"] == ["v_p_00", "v_p_01"] and not s["Soccer"]["errors"]
    loaded = [load_frames(p, device=DEV) for p in vids]
    assert [k.tolist() for _, k in loaded] == [[0, 1, 2, 3, 4], [0, 1, 2]]
    ref = extract_videos(hmr, wb, FullFrameDetector(), [(p.stem, fr) for p, (fr, _) in zip(vids, loaded)],
                         tmp_path / "ref_meshes", tmp_path / "ref_kps")
    for p, (fr, kept) in zip(vids, loaded):
        z = np.load(tmp_path / "meshes" / "Soccer" / f"{p.stem}.npz")
        r = np.load(ref[p.stem])
        np.testing.assert_array_equal(z["frame_idx"], kept[r["frame_idx"]])   # indices into the APNG's frames
        for k in ("pose", "betas", "global_orient", "vit"):
            np.testing.assert_array_equal(z[k], r[k])
        np.testing.assert_array_equal(np.load(tmp_path / "kps" / "Soccer" / p.stem / "keypoints.npy"),
                                      np.load(tmp_path / "ref_kps" / p.stem / "keypoints.npy"))
