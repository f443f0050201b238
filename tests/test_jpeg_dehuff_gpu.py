"""The device entropy decoder (csrc/vge_jpeg_dehuff.hip: vge_jpeg_entropy_decode_device) and the Python layer on it
(decode_frames, load_frames(entropy="device"), extract_frame_tree) against the host decoder: exact equality of
coefficients, tables, statuses and pixels.  Reads the three JPEG fixtures (no Pillow needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import jpeg_dehuff_cases as DC
from tests import jpeg_enc_cases as JC
from tests import jpeg_entropy_cases as EC
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64   # canary elements in front of and behind every output buffer


@pytest.fixture(scope="module")
def files():
    return DC.all_files()


@pytest.fixture(scope="module")
def paths(files, tmp_path_factory):
    root = tmp_path_factory.mktemp("jpeg_dehuff_gpu")
    out = {}
    for name, blob in files.items():
        p = root / f"{name}.jpg"
        p.write_bytes(blob)
        out[name] = str(p)
    return out


def workspace_for(lay, n, nbytes):
    from vge import lib as L
    size = int(L.load().vge_jpeg_entropy_decode_workspace_bytes(C.byref(lay), n, nbytes))
    assert size > 0
    return torch.empty(size, dtype=torch.uint8, device=DEV)


def device_decode(data, off, size, lay, ws=None):
    """vge_jpeg_entropy_decode_device on the current stream -> (return code, status [n], coef, qtab, rounds [n], and
    whether every canary around the outputs and in the gaps between the files survived)."""
    from vge import lib as L
    n, per = len(off), lay.blocks_per_frame * 64
    d = torch.from_numpy(data).to(DEV)
    table = torch.from_numpy(np.stack([off, size]).astype(np.int64)).to(DEV)
    ws = workspace_for(lay, n, data.size) if ws is None else ws
    coef = torch.full((n * per + 2 * PAD,), 0x5A5A, dtype=torch.int16, device=DEV)
    qtab = torch.full((n * 192 + 2 * PAD,), 0x5A5A, dtype=torch.int16, device=DEV)
    st = torch.full((n + 2 * PAD,), -77, dtype=torch.int32, device=DEV)
    rounds = torch.full((n + 2 * PAD,), -77, dtype=torch.int32, device=DEV)
    rc = L.load().vge_jpeg_entropy_decode_device(
        d.data_ptr(), data.size, table[0].data_ptr(), table[1].data_ptr(), n, C.byref(lay), ws.data_ptr(),
        coef[PAD:].data_ptr(), qtab[PAD:].data_ptr(), st[PAD:].data_ptr(), rounds[PAD:].data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    intact = all(bool((t[:PAD] == v).all()) and bool((t[t.numel() - PAD:] == v).all())
                 for t, v in ((coef, 0x5A5A), (qtab, 0x5A5A), (st, -77), (rounds, -77)))
    intact = intact and np.array_equal(d.cpu().numpy(), data)
    return (rc, st[PAD:PAD + n].cpu().numpy(), coef[PAD:PAD + n * per].cpu().numpy().reshape(n, -1, 64),
            qtab[PAD:PAD + n * 192].cpu().numpy().view(np.uint16).reshape(n, 3, 64),
            rounds[PAD:PAD + n].cpu().numpy(), intact)


def assert_equals_host(blobs, lay, what, gap=0, order=None):
    data, off, size = DC.pack(blobs, gap=gap, order=order)
    _, hst, hcoef, hqtab = DC.host_decode_mem(data, off, size, lay)
    rc, st, coef, qtab, rounds, intact = device_decode(data, off, size, lay)
    assert rc == 0 and intact, what
    assert st.tolist() == hst.tolist(), (what, st.tolist(), hst.tolist())
    assert np.array_equal(coef, hcoef) and np.array_equal(qtab, hqtab), what
    assert (rounds >= 0).all(), what
    return st, coef, qtab, rounds


def encoded(coef, lay, quality=95):
    rc, _, st, out = EC.encode_mem(coef[None], lay, quality=quality)
    assert rc == 0 and st[0] == 0
    return out[0]


def test_every_fixture_file_equals_the_host_decoder(files):
    """One frame per call: 1 x 1 (a scan shorter than one subsequence), restart intervals of 1 MCU (15 of them: the
    marker index wraps), 2 MCUs, 3 MCUs and one MCU row, optimised tables, grayscale (one block per MCU), long codes."""
    from vge.frames import make_layout
    seen = set()
    for name, blob in files.items():
        row = DC.probe_one(blob)
        lay = make_layout(*[int(x) for x in row[:5]]) if int(row[5]) == 0 else make_layout(16, 16, 3, 2, 2)
        st, _, _, rounds = assert_equals_host([blob], lay, name)
        seen.add(int(st[0]))
        if st[0] == 0:
            assert rounds[0] >= 1, name
    assert seen == {0, DC.ERR_IO, DC.ERR_PROGRESSIVE}


def test_fixture_pixels_through_load_frames(paths):
    from vge.frames import load_frames
    for fixture in ("jpeg_golden.npz", "jpeg_enc_golden.npz"):
        gold = np.load(GOLDEN / fixture)
        for name in list(gold["names"]) + list(gold["batch_names"]):
            fr, kept = load_frames([paths[str(name)]], device=DEV, entropy="device")
            assert kept.tolist() == [0] and fr.device.type == "cuda", name
            assert torch.equal(fr[0].cpu(), torch.from_numpy(gold[f"rgb/{name}"])), name


@pytest.fixture(scope="module")
def synthetic():
    """{name: (layout, coefficients, file bytes)} of the coder's synthetic set, coded by the host coder."""
    out = {}
    for name, shape, coef in EC.synthetic_set():
        lay = EC.layout(*shape)
        out[name] = (lay, coef, encoded(coef, lay))
    return out


def test_synthetic_set_round_trip(synthetic):
    """max_block and dense put subsequence starts inside 1,658-bit blocks (whole subsequences hold no block start);
    their blocks are beyond VGE_JPEG_BLOCK_L1_MAX, so after decoding them both sides answer ERR_IO (dense blocks the
    decoder accepts: test_several_tiles).  ff_tail ends the scan on a stuffed FF, zero is nothing but EOBs,
    sparse_520x280 spans many subsequences."""
    from vge import lib as L
    sub = L.load().vge_jpeg_entropy_decode_subsequence_bytes()
    assert 1658 // 8 > 2 * sub   # a maximal block covers whole subsequences
    for name, (lay, coef, blob) in synthetic.items():
        st, got, _, rounds = assert_equals_host([blob], lay, name)
        if name in DC.L1_REFUSED:
            assert st[0] == DC.ERR_IO and not got.any() and rounds[0] > 2, name
        else:
            assert st[0] == 0 and np.array_equal(got[0], coef), name
    assert synthetic["ff_tail"][2].endswith(b"\xff\x00\xff\xd9")
    assert len(synthetic["sparse_520x280"][2]) > 100 * sub


def test_several_tiles():
    from vge import lib as L
    tile = L.load().vge_jpeg_entropy_decode_tile_bytes()
    lay, coef = DC.dense_frame(tile)
    blob = encoded(coef, lay, DC.DENSE_QUALITY)
    scan = len(blob) - DC.scan_start(blob) - 2 - blob[DC.scan_start(blob):].count(b"\xff\x00")
    assert scan >= 3 * tile and scan % tile != 0
    st, got, _, rounds = assert_equals_host([blob], lay, "dense tiles")
    assert st[0] == 0 and np.array_equal(got[0], coef) and rounds[0] > 2


def test_more_than_two_rounds(synthetic):
    """A lane that starts inside a dense block stays out of step until a block boundary: its guess needs repairing over
    several subsequences.  ROUNDS_CASE was found by DC.find_rounds_case."""
    def rounds_of(name, shape, coef):
        lay, _, blob = synthetic[name]
        return int(assert_equals_host([blob], lay, name)[3][0])
    assert DC.find_rounds_case(rounds_of) == DC.ROUNDS_CASE
    lay, coef, blob = synthetic[DC.ROUNDS_CASE]
    assert rounds_of(DC.ROUNDS_CASE, None, None) > 2
    assert np.array_equal(DC.host_decode_files([blob], lay)[2][0], coef)


def test_error_streams_equal_the_host(files):
    lay = DC.layout_of(files["batch_0"])
    st = assert_equals_host([files["truncated"], files["progressive"], files["16x16_420_smooth"]], lay, "bad files")[0]
    assert st.tolist() == [DC.ERR_IO, DC.ERR_PROGRESSIVE, DC.ERR_SHAPE]
    blob = files["37x53_420_noise"]
    cut = DC.cuts(blob)
    st = assert_equals_host(list(cut.values()), DC.layout_of(blob), "cuts")[0]
    assert dict(zip(cut, st.tolist()))["ff_00"] == DC.ERR_IO
    rst = files["rst1_80x48_420"]
    st = assert_equals_host([rst, DC.wrong_marker_index(rst), DC.removed_marker(rst)], DC.layout_of(rst), "rst")[0]
    assert st.tolist() == [0, DC.ERR_IO, DC.ERR_IO]
    flips = DC.flip_set()
    st = assert_equals_host(flips, DC.layout_of(files[DC.FLIP_FILE]), "flips")[0]
    assert (st == 0).any() and (st == DC.ERR_IO).any()


def test_surplus_byte_before_a_marker_is_refused(files):
    """The one class outside the equality with the host (include/vge_frames.h): the device answers ERR_IO."""
    rst = files["rst1_80x48_420"]
    lay = DC.layout_of(rst)
    data, off, size = DC.pack([rst, DC.surplus_before_marker(rst)])
    rc, st, coef, qtab, _, intact = device_decode(data, off, size, lay)
    assert rc == 0 and intact and st.tolist() == [0, DC.ERR_IO]
    assert not coef[1].any() and (qtab[1] == 1).all()


def test_batch_with_failed_frames_gaps_and_canaries(files, paths):
    from vge.frames import load_frames
    names = ["batch_0", "truncated", "batch_1", "16x16_420_smooth", "batch_2"]
    blobs = [files[n] for n in names]
    lay = DC.layout_of(blobs[0])
    st, coef, qtab, _ = assert_equals_host(blobs, lay, "batch", gap=7, order=[3, 0, 4, 2, 1])
    assert np.flatnonzero(st == 0).tolist() == [0, 2, 4]
    for i, blob in enumerate(blobs):   # neighbours equal their single-frame results, rows between canaries
        s1, c1, q1, _ = assert_equals_host([blob], lay, names[i])
        assert s1[0] == st[i] and np.array_equal(c1[0], coef[i]) and np.array_equal(q1[0], qtab[i]), i
    fr, kept = load_frames([paths[n] for n in names], device=DEV, entropy="device")
    ref, rkept = load_frames([paths[n] for n in names], device=DEV)
    assert kept.tolist() == rkept.tolist() == [0, 2, 4] and torch.equal(fr, ref)


def test_argument_refusals(files):
    from vge import lib as L
    so = L.load()
    blob = files["batch_0"]
    lay = DC.layout_of(blob)
    data, off, size = DC.pack([blob, blob, blob], gap=4)
    bad = size.copy()
    bad[0], bad[2] = -1, data.size   # a negative size; an offset / size pair that leaves the buffer
    rc, st, coef, qtab, _, intact = device_decode(data, off, bad, lay)
    assert rc == 0 and intact and st.tolist() == [DC.ERR_ARG, 0, DC.ERR_ARG]
    assert not coef[0].any() and (qtab[0] == 1).all() and coef[1].any() and not coef[2].any()
    assert so.vge_jpeg_entropy_decode_device(None, 0, None, None, 0, C.byref(lay), None, None, None, None, None,
                                             None) == 0
    assert so.vge_jpeg_entropy_decode_device(None, 8, None, None, 1, C.byref(lay), None, None, None, None, None,
                                             None) == DC.ERR_ARG
    assert b"vge_jpeg_entropy_decode_device" in so.vge_last_error()
    assert so.vge_jpeg_entropy_decode_workspace_bytes(C.byref(lay), -1, 8) == 0


def test_workspace_reuse():
    from vge import lib as L
    lay, dense = DC.dense_frame(L.load().vge_jpeg_entropy_decode_tile_bytes())
    dense_blob = encoded(dense, lay, DC.DENSE_QUALITY)
    zero_blob = encoded(np.zeros_like(dense), lay, DC.DENSE_QUALITY)
    ws = workspace_for(lay, 1, len(dense_blob) + 16)
    got = []
    for blob in (dense_blob, zero_blob, dense_blob):
        data, off, size = DC.pack([blob])
        data = np.concatenate([data, np.full(len(dense_blob) + 16 - data.size, DC.CANARY, np.uint8)])
        rc, st, coef, _, _, intact = device_decode(data, off, size, lay, ws=ws)
        assert rc == 0 and intact and st[0] == 0
        got.append(coef[0])
    assert np.array_equal(got[0], dense) and np.array_equal(got[2], dense) and not got[1].any()


def test_non_default_stream_equals_default_stream(files, paths):
    from vge.frames import load_frames
    names = [f"batch_{i}" for i in range(5)] + ["rst1_80x48_420"]
    blobs = [files[n] for n in names[:5]]
    lay = DC.layout_of(blobs[0])
    data, off, size = DC.pack(blobs)
    ref = device_decode(data, off, size, lay)
    ref_fr, _ = load_frames([paths[n] for n in names[:5]], device=DEV, entropy="device")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        got = device_decode(data, off, size, lay)
        fr, _ = load_frames([paths[n] for n in names[:5]], device=DEV, entropy="device")
    s.synchronize()
    assert got[0] == 0 and got[5] and all(np.array_equal(a, b) for a, b in zip(got[1:5], ref[1:5]))
    assert torch.equal(fr, ref_fr)


def test_on_device_loop_inverts_encode_frames():
    from vge.frames import decode_frames, encode_frames, jpeg_roundtrip
    gold = JC.load_gold()
    fr = torch.cat([torch.from_numpy(gold[f"src/{JC.parts(n)[0]}"])[None] for n in gold["batch_names"]]).to(DEV)
    out, kept = decode_frames(*encode_frames(fr, keep_on_device=True))
    assert out.device.type == "cuda" and kept.tolist() == [0, 1, 2, 3, 4]
    assert torch.equal(out, jpeg_roundtrip(fr))
    tile = torch.from_numpy(gold["src/tile260x140"])[None].to(DEV)
    for sub in ("420", "422", "444"):
        data, offsets = encode_frames(tile, subsampling=sub, keep_on_device=True)
        assert data.device.type == "cuda"
        out, kept = decode_frames(data, offsets)
        assert out.device.type == "cuda" and kept.tolist() == [0], sub
        assert torch.equal(out, jpeg_roundtrip(tile, subsampling=sub)), sub
    # files in host memory, decoded on the device after one upload
    data, offsets = encode_frames(fr)
    assert data.device.type == "cpu"
    out, kept = decode_frames(data, offsets, device=DEV, entropy="device")
    assert out.device.type == "cuda" and torch.equal(out, jpeg_roundtrip(fr))


def test_device_path_equals_host_path(paths):
    from vge.frames import UnsupportedJpegError, load_frames, load_videos
    gold = np.load(GOLDEN / "jpeg_golden.npz")
    tree = [paths[str(n)] for n in gold["tree_names"]]
    dev, kd = load_frames(tree, device=DEV, entropy="device")
    host, kh = load_frames(tree, device=DEV, entropy="host")
    assert tuple(dev.shape) == (12, 128, 128, 3) and kd.tolist() == kh.tolist() and torch.equal(dev, host)
    for n in gold["tile_names"]:
        dev, kd = load_frames([paths[str(n)]], device=DEV, entropy="device")
        host, kh = load_frames([paths[str(n)]], device=DEV, entropy="host")
        assert kd.tolist() == kh.tolist() == [0] and torch.equal(dev, host), n
    # videos of two layouts, an unreadable video and a missing file in one call
    vids = [tree[:6], [paths["tile_260x140_gray"]], [paths["truncated"]], tree[6:8] + [tree[0] + ".missing"]]
    a = load_videos(vids, device=DEV, entropy="device")
    b = load_videos(vids, device=DEV, entropy="host")
    for (fa, ka), (fb, kb) in zip(a, b):
        assert ka.tolist() == kb.tolist() and fa.shape == fb.shape and torch.equal(fa, fb)
    assert a[2][1].size == 0 and a[3][1].tolist() == [0, 1]
    with pytest.raises(UnsupportedJpegError, match="progressive"):
        load_frames([tree[0], paths["progressive"]], device=DEV, entropy="device")
    with pytest.raises(ValueError):
        load_frames(tree, device="cpu", entropy="device")


def test_extraction_driver_with_the_device_decoder(tmp_path):
    from tests.test_extract_tree_gpu import FullFrameDetector
    from vge import dwpose as D, hmr as H, synth
    from vge.extract import extract_frame_tree
    gold = np.load(GOLDEN / "jpeg_golden.npz")
    hcfg = H.HmrConfig(embed_dim=256, depth=1, heads=4, mlp_dim=256, dec_dim=256, dec_depth=1, dec_heads=4,
                       dec_mlp=256, tok_num=4, tok_classes=256, tok_code_dim=256)
    hmr = H.HmrExtractor(synth.make_hmr_state_dict(hcfg), hcfg, device=DEV, max_frames=8)
    ycfg = D.YoloxConfig(in_size=128, width=16, depth=1, head_ch=64)
    pcfg = D.RtmposeConfig(in_h=128, in_w=96, stem_ch=16, stage_ch=(32, 64, 128, 256), stage_blocks=(1, 1, 1, 1))
    wb = D.Wholebody(D.YoloxDetector(synth.make_yolox_state_dict(ycfg), ycfg, device=DEV, chunk=8),
                     D.DwposeExtractor(synth.make_rtmpose_state_dict(pcfg), pcfg, device=DEV, max_instances=16))
    for v in range(2):
        d = tmp_path / "frames" / "Soccer" / f"v_s_{v:02d}"
        d.mkdir(parents=True)
        for f in range(6):
            (d / f"frame_{f:06d}.jpg").write_bytes(gold[f"jpeg/tree_v{v}_f{f}"].tobytes())
    out = {}
    for entropy in ("host", "device"):
        root = tmp_path / entropy
        s = extract_frame_tree(hmr, wb, FullFrameDetector(), tmp_path / "frames", root / "meshes", root / "kps",
                               root / "logs", device=DEV, entropy=entropy)
        assert s["Soccer"]["single"] == ["v_s_00", "v_s_01"] and not s["Soccer"]["errors"]
        out[entropy] = root
    for v in range(2):
        a = np.load(out["host"] / "meshes" / "Soccer" / f"v_s_{v:02d}.npz")
        b = np.load(out["device"] / "meshes" / "Soccer" / f"v_s_{v:02d}.npz")
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            if k != "meta":
                np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        np.testing.assert_array_equal(np.load(out["host"] / "kps" / "Soccer" / f"v_s_{v:02d}" / "keypoints.npy"),
                                      np.load(out["device"] / "kps" / "Soccer" / f"v_s_{v:02d}" / "keypoints.npy"))
