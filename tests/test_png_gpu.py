"""The device PNG decoder (csrc/vge_png.hip: vge_png_decode_device) and the Python layer on it against the host decoder
vge_png_decode_mem: exact equality of statuses and, for accepted frames, of pixels, with canaries around the output, the
statuses and the workspace.  Files come from tests/png_cases.py (the CPU suite pins the host decoder to Pillow on the
same files) and tests/golden/png_golden.npz (Pillow-written files with Pillow's pixels)."""
import numpy as np
import pytest
import torch

from tests import png_cases as PC
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 256   # canary bytes / elements around every device buffer


def lib():
    from vge import lib as L
    return L.load()


def device_decode(data, off, size, layout, ws=None, fill=0x5A, tamper=None):
    """Plan on the host, decode on the device -> (return code, combined status [n], uint8 [n, H, W, 3], whether every
    canary and the inputs survived, the workspace tensor).  tamper(descs, segs, workspace bytes) may spoil the plan."""
    w, h, ct = layout
    n = len(off)
    _, descs, segs, n_segs, plan_st, ws_bytes = PC.host_plan_mem(data, off, size, layout)
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
    rc = lib().vge_png_decode_device(d.data_ptr(), data.size, dd.data_ptr(), n, sd.data_ptr(), n_segs, n, w, h, ct,
                                     ws[PAD:].data_ptr(), ws_bytes, out[PAD:].data_ptr(), st[PAD:].data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    intact = all(bool((t[:PAD] == v).all()) and bool((t[t.numel() - PAD:] == v).all())
                 for t, v in ((out, fill), (st, -77), (ws, 0x5A)))
    intact = intact and np.array_equal(d.cpu().numpy(), data) and bytes(dd.cpu().numpy()) == bytes(descs)
    dev_st = st[PAD:PAD + n].cpu().numpy()
    assert not (plan_st != 0)[dev_st != 0].any()   # a frame the plan refused has no work to fail
    rgb = out[PAD:PAD + n * frame].cpu().numpy().reshape(n, h, w, 3)
    return rc, np.where(plan_st != 0, plan_st, dev_st), rgb, intact, ws


def assert_equals_host(files, layout, what, gap=16, order=None, ws=None):
    data, off, size = PC.pack(files, gap=gap, order=order)
    _, hrgb, hst = PC.host_decode_mem(data, off, size, layout)
    rc, st, rgb, intact, ws = device_decode(data, off, size, layout, ws=ws)
    assert rc == 0 and intact, what
    assert st.tolist() == hst.tolist(), (what, st.tolist(), hst.tolist())
    for i in range(len(files)):
        if st[i] == 0:
            assert np.array_equal(rgb[i], hrgb[i]), (what, i)
    return st, rgb, ws


@pytest.mark.parametrize("layout", list(PC.by_layout()), ids=lambda l: "%dx%d_ct%d" % l)
def test_every_case_equals_the_host(layout):
    """All cases of one layout in one call, good and refused frames side by side; the statuses are the ones the cases
    were built for.  A refused frame's rows keep the fill: nobody else writes them (the frame itself writes nothing
    when it is refused before the unfilter, as every refused case here but the filter-byte ones is)."""
    group = PC.by_layout()[layout]
    st, rgb, _ = assert_equals_host([c.data for c in group], layout, layout)
    for i, c in enumerate(group):
        want = c.expect if c.expect is not None else (0 if c.accept else PC.ERR_IO)
        assert st[i] == want, c.name
        if st[i] != 0 and not c.name.startswith("filter5"):
            assert (rgb[i] == 0x5A).all(), c.name


def test_cases_cover_the_kernels_ground():
    band = lib().vge_png_decode_device_band_rows()
    heights = {c.layout[1] for c in PC.cases() if c.accept}
    assert {band - 1, band, band + 1, 2 * band + 1} <= heights
    tails = {(h * (1 + w * PC.CHANNELS[ct])) % 4 for w, h, ct in PC.by_layout()}
    assert tails == {0, 1, 2, 3}
    ring = lib().vge_ingest_decode_device_ring_bytes()
    w, h, ct = next(c.layout for c in PC.cases() if c.name == "ring_wrap")
    assert h * (1 + w * PC.CHANNELS[ct]) > ring


def test_golden_files_equal_their_stored_pixels():
    gold = np.load(GOLDEN / "png_golden.npz")
    names = sorted(k[4:] for k in gold.files if k.startswith("png/"))
    assert len(names) >= 6
    for name in names:
        want = gold[f"rgb/{name}"]
        ct = {"rgba": 6, "grey": 0}.get(name.split("_")[0], 2)
        layout = (want.shape[1], want.shape[0], ct)
        st, rgb, _ = assert_equals_host([gold[f"png/{name}"].tobytes()], layout, name, gap=3)
        assert st.tolist() == [0] and np.array_equal(rgb[0], want), name


def test_packing_order_and_a_reused_workspace():
    """Files packed with odd gaps and in reverse order; the same workspace, as the first call left it, gives the same
    result on the second."""
    layout = (13, 7, 2)
    group = PC.by_layout()[layout]
    files = [c.data for c in group]
    st1, rgb1, ws = assert_equals_host(files, layout, "first", gap=5, order=list(range(len(files)))[::-1])
    st2, rgb2, _ = assert_equals_host(files, layout, "reused", gap=5, order=list(range(len(files)))[::-1], ws=ws)
    assert st1.tolist() == st2.tolist() and np.array_equal(rgb1, rgb2)
    assert 0 in st1 and PC.ERR_IO in st1 and PC.ERR_SHAPE in st1


def test_descriptors_and_segments_that_do_not_fit_are_refused_by_the_kernels():
    """Every way a descriptor or a segment can point outside what the host passed: the frame gets VGE_PNG_ERR_ARG (or,
    with nobody to report to, is left alone), nothing outside the buffers is touched and the neighbours decode."""
    layout = (13, 7, 2)
    good = next(c.data for c in PC.cases() if c.name == "idat_one")
    n = 12
    data, off, size = PC.pack([good] * n, gap=8)
    _, hrgb, _ = PC.host_decode_mem(data, off, size, layout)

    def tamper(descs, segs, ws_bytes):
        assert [g.desc for g in segs[:n]] == list(range(n))   # one chunk per file: segment k belongs to frame k
        descs[0].gat_off = ws_bytes - 1
        descs[1].slot_off += 4
        descs[2].slot_off = ws_bytes
        descs[3].raw_bytes += 1
        descs[4].file_off = -1
        descs[5].color_type = 6
        segs[6].src_off = descs[6].file_off - 1
        segs[7].bytes = 1 << 40
        segs[8].dst_off = descs[8].gat_off + descs[8].gat_bytes
        segs[9].desc = n          # nobody's segment: frame 9 inflates its untouched (0x5A-filled) run
        descs[10].frame = n       # nobody's frame: no status to set, no rows to write

    rc, st, rgb, intact, _ = device_decode(data, off, size, layout, tamper=tamper)
    assert rc == 0 and intact
    assert st.tolist() == [1] * 9 + [PC.ERR_IO, 0, 0]
    assert (rgb[:11] == 0x5A).all() and np.array_equal(rgb[11], hrgb[11])


def test_bad_arguments_are_refused_before_any_launch():
    L = lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    st = torch.full((4,), -5, dtype=torch.int32, device=DEV)
    p, s = buf.data_ptr(), st.data_ptr()
    ok = dict(data=p, data_bytes=1024, descs=p + 1024, n_descs=1, segs=p + 2048, n_segs=1, n_frames=1, w=4, h=4, ct=2,
              ws=p + 3072, ws_bytes=512, rgb=p + 3600, status=s, stream=None)
    for change in (dict(n_descs=-1), dict(n_segs=-1), dict(n_segs=1 << 31), dict(n_frames=-1), dict(data_bytes=-1),
                   dict(ws_bytes=-1), dict(w=0), dict(h=0), dict(ct=3), dict(ct=1), dict(status=None),
                   dict(status=s + 2), dict(data=None), dict(descs=None), dict(descs=p + 1028), dict(segs=None),
                   dict(segs=p + 2052), dict(ws=None), dict(ws=p + 3080), dict(rgb=None)):
        a = dict(ok, **change)
        rc = L.vge_png_decode_device(a["data"], a["data_bytes"], a["descs"], a["n_descs"], a["segs"], a["n_segs"],
                                     a["n_frames"], a["w"], a["h"], a["ct"], a["ws"], a["ws_bytes"], a["rgb"],
                                     a["status"], a["stream"])
        assert rc == 1 and b"vge_png_decode_device" in L.vge_last_error(), change
    torch.cuda.synchronize()
    assert (st == -5).all() and not buf.any()


@pytest.fixture(scope="module")
def png_tree(tmp_path_factory):
    """Two PNG videos of three good frames each around one broken and one JPEG file, from the golden files' pixels."""
    from vge.frames import encode_frames
    root = tmp_path_factory.mktemp("png_tree")
    vids = []
    for v, ct in enumerate((2, 6)):
        d = root / "frames" / "Soccer" / f"v_p_{v:02d}"
        d.mkdir(parents=True)
        for f in range(5):
            px = PC.pixels(50 + 10 * v + f, 128, 128, ct, smooth=True)
            data = PC.simple(px, ct, (0, 1, 2, 3, 4), level=6, idat=4096)
            if v == 0 and f == 1:
                data = data[:len(data) // 2]
            if v == 0 and f == 3:
                jd, jo = encode_frames(torch.from_numpy(np.ascontiguousarray(px[None, ..., :3])), entropy="host")
                data = jd.numpy().tobytes()
            (d / f"frame_{f:06d}.png").write_bytes(data)
        vids.append(d)
    return root, vids


def test_loaders_agree_between_host_and_device(png_tree):
    from vge import frames as FR
    _, vids = png_tree
    host = FR.load_videos(vids, device=DEV, entropy="host")
    dev = FR.load_videos(vids, device=DEV, entropy="device")
    assert [k.tolist() for _, k in host] == [[0, 2, 4], [0, 1, 2, 3, 4]]
    for (hf, hk), (df, dk) in zip(host, dev):
        assert hk.tolist() == dk.tolist() and hf.device.type == "cuda" and torch.equal(hf, df)
        assert tuple(hf.shape[1:]) == (128, 128, 3)
    one_h, kept_h = FR.load_frames(vids[0], device=DEV, entropy="host")
    one_d, kept_d = FR.load_frames(vids[0], device=DEV, entropy="device")
    assert kept_h.tolist() == kept_d.tolist() == [0, 2, 4] and torch.equal(one_h, one_d) and torch.equal(one_h, host[0][0])
    cpu, kept_c = FR.load_frames(vids[0], device="cpu")
    assert kept_c.tolist() == [0, 2, 4] and torch.equal(cpu, one_d.cpu())


def test_decode_frames_on_a_device_resident_buffer():
    from vge import frames as FR
    layout = (13, 7, 2)
    group = [c for c in PC.by_layout()[layout] if c.expect is None]
    data, off, size = PC.pack([c.data for c in group])
    offsets = np.concatenate([off, [off[-1] + size[-1]]])
    _, hrgb, hst = PC.host_decode_mem(data, off, size, layout)
    frames, kept = FR.decode_frames(torch.from_numpy(data).to(DEV), offsets)
    assert kept.tolist() == np.flatnonzero(hst == 0).tolist() and frames.device.type == "cuda"
    assert np.array_equal(frames.cpu().numpy(), hrgb[kept])
    frames_h, kept_h = FR.decode_frames(torch.from_numpy(data), offsets, device=DEV)
    assert kept_h.tolist() == kept.tolist() and torch.equal(frames_h, frames)


class FullFrameDetector:
    """The gate detector's interface with one person box over the whole frame (the detector has its own tests)."""
    def detect(self, fr):
        F, H, W = (int(v) for v in fr.shape[:3])
        person = torch.zeros(F, 1, 5, device=fr.device)
        person[:, 0, :4] = torch.tensor([0.0, 0.0, W, H], device=fr.device)
        return {"person": person, "n_person": torch.ones(F, dtype=torch.int32, device=fr.device)}


@pytest.mark.parametrize("quality", [None, 95])
def test_tree_driver_on_png_folders(png_tree, tmp_path, quality):
    """extract_frame_tree(frame_format="png") writes what extract_videos writes for the same decoded frames, with and
    without the JPEG round trip in front of the models."""
    from vge import dwpose as D, hmr as H, synth
    from vge.extract import extract_frame_tree, extract_videos
    from vge.frames import load_frames
    root, vids = png_tree
    hcfg = H.HmrConfig(embed_dim=256, depth=1, heads=4, mlp_dim=256, dec_dim=256, dec_depth=1, dec_heads=4,
                       dec_mlp=256, tok_num=4, tok_classes=256, tok_code_dim=256)
    hmr = H.HmrExtractor(synth.make_hmr_state_dict(hcfg), hcfg, device=DEV, max_frames=8)
    ycfg = D.YoloxConfig(in_size=128, width=16, depth=1, head_ch=64)
    pcfg = D.RtmposeConfig(in_h=128, in_w=96, stem_ch=16, stage_ch=(32, 64, 128, 256), stage_blocks=(1, 1, 1, 1))
    wb = D.Wholebody(D.YoloxDetector(synth.make_yolox_state_dict(ycfg), ycfg, device=DEV, chunk=8),
                     D.DwposeExtractor(synth.make_rtmpose_state_dict(pcfg), pcfg, device=DEV, max_instances=16))
    s = extract_frame_tree(hmr, wb, FullFrameDetector(), root / "frames", tmp_path / "meshes", tmp_path / "kps",
                           tmp_path / "logs", device=DEV, frame_format="png", jpeg_quality=quality, entropy="device")
    assert s["Soccer"]["single"] == ["v_p_00", "v_p_01"] and not s["Soccer"]["errors"]
    loaded = [load_frames(d, device=DEV) for d in vids]
    ref = extract_videos(hmr, wb, FullFrameDetector(), [(d.name, fr) for d, (fr, _) in zip(vids, loaded)],
                         tmp_path / "ref_meshes", tmp_path / "ref_kps", jpeg_quality=quality)
    for d, (fr, kept) in zip(vids, loaded):
        z = np.load(tmp_path / "meshes" / "Soccer" / f"{d.name}.npz")
        r = np.load(ref[d.name])
        np.testing.assert_array_equal(z["frame_idx"], kept[r["frame_idx"]])   # indices into the sorted *.png list
        for k in ("pose", "betas", "global_orient", "vit"):
            np.testing.assert_array_equal(z[k], r[k])
        np.testing.assert_array_equal(np.load(tmp_path / "kps" / "Soccer" / d.name / "keypoints.npy"),
                                      np.load(tmp_path / "ref_kps" / d.name / "keypoints.npy"))
    with pytest.raises(ValueError):
        extract_frame_tree(hmr, wb, FullFrameDetector(), root / "frames", tmp_path / "m", tmp_path / "k",
                           tmp_path / "l", device=DEV, frame_format="bmp")
