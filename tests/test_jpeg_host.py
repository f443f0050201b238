"""The JPEG frame front end on the host (include/vge_frames.h, vge/frames.py): the entropy decoder and the plain-C++
reconstruct reproduce Pillow / libjpeg-turbo (the islow IDCT and fancy upsampling cv2.imread uses too) byte for byte on
the committed fixture (tests/golden/make_jpeg_golden.py); the error statuses; no GPU needed."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN, REPO


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN / "jpeg_golden.npz"))


@pytest.fixture(scope="module")
def files(gold, tmp_path_factory):
    """Every fixture JPEG written to disk once: {name: path}."""
    root = tmp_path_factory.mktemp("jpeg")
    out = {}
    for k, v in gold.items():
        if k.startswith("jpeg/") or k.startswith("bad/"):
            p = root / (k.replace("/", "_") + ".jpg")
            p.write_bytes(v.tobytes())
            out[k.split("/", 1)[1]] = str(p)
    return out


def test_host_decode_equals_pillow_on_every_fixture(gold, files):
    from vge.frames import load_frames
    for name in list(gold["names"]) + list(gold["batch_names"]):
        fr, kept = load_frames([files[name]], device="cpu")
        assert kept.tolist() == [0], name
        assert np.array_equal(fr[0].numpy(), gold[f"rgb/{name}"]), name


def test_probe_reports_size_and_sampling(gold, files):
    from vge.frames import probe
    info = probe([files["37x53_420_smooth"], files["37x53_422_noise"], files["17x33_444_smooth"],
                  files["19x21_gray_noise"]])
    assert info.tolist() == [[37, 53, 3, 2, 2, 0], [37, 53, 3, 2, 1, 0], [17, 33, 3, 1, 1, 0], [19, 21, 1, 1, 1, 0]]


def test_progressive_reports_its_own_status(files):
    from vge import lib as L
    from vge.frames import UnsupportedJpegError, load_frames, probe
    info = probe([files["progressive"]])
    assert info[0, 5] == 20 and L.JPEG_STATUS[20] == "ERR_PROGRESSIVE"
    assert info[0, :2].tolist() == [37, 53]
    with pytest.raises(UnsupportedJpegError, match="progressive") as e:
        load_frames([files["batch_0"], files["progressive"]], device="cpu")
    assert files["progressive"] in str(e.value)


def test_layout_refuses_unsupported_sampling_and_components():
    from vge import lib as L
    so = L.load()
    lay = L.JpegLayout()
    assert so.vge_jpeg_make_layout(16, 16, 3, 1, 2, C.byref(lay)) == 24
    assert so.vge_jpeg_make_layout(16, 16, 3, 4, 1, C.byref(lay)) == 24
    assert so.vge_jpeg_make_layout(16, 16, 4, 1, 1, C.byref(lay)) == 23
    assert so.vge_jpeg_make_layout(0, 16, 3, 1, 1, C.byref(lay)) == 1
    assert b"vge_jpeg_make_layout" in so.vge_last_error()
    assert so.vge_jpeg_make_layout(37, 53, 3, 2, 2, C.byref(lay)) == 0
    assert (lay.mcus_x, lay.mcus_y, list(lay.bw), list(lay.bh), list(lay.off), lay.blocks_per_frame) == \
        (3, 4, [6, 3, 3], [8, 4, 4], [0, 48, 60], 72)


def test_truncated_frame_fails_alone_in_a_batch(gold, files):
    from vge import lib as L
    from vge.frames import load_frames
    names = list(gold["batch_names"])
    paths = [files[n] for n in names[:2]] + [files["truncated"]] + [files[n] for n in names[2:]]
    fr, kept = load_frames(paths, device="cpu")
    assert kept.tolist() == [0, 1, 3, 4, 5]
    for j, n in enumerate(names):
        assert np.array_equal(fr[j].numpy(), gold[f"rgb/{n}"]), n
    # the per-frame status is the IO one, and vge_last_error names the file
    so = L.load()
    lay = L.JpegLayout()
    assert so.vge_jpeg_make_layout(64, 48, 3, 2, 2, C.byref(lay)) == 0
    coef = np.full((len(paths), lay.blocks_per_frame, 64), 7, np.int16)
    qt = np.zeros((len(paths), 3, 64), np.uint16)
    st = np.full(len(paths), -1, np.int32)
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    rc = so.vge_jpeg_entropy_decode(arr, len(paths), 2, C.byref(lay), coef.ctypes.data, qt.ctypes.data, st.ctypes.data)
    assert rc == 7 and st.tolist() == [0, 0, 7, 0, 0, 0]
    assert os.fsencode(files["truncated"]) in so.vge_last_error()
    assert not coef[2].any() and (qt[2] == 1).all()


def test_second_size_in_one_call_gets_the_shape_status(files):
    from vge import lib as L
    from vge.frames import load_frames
    paths = [files["batch_0"], files["16x16_420_smooth"], files["batch_1"], files["19x21_gray_noise"]]
    so = L.load()
    lay = L.JpegLayout()
    assert so.vge_jpeg_make_layout(64, 48, 3, 2, 2, C.byref(lay)) == 0
    coef = np.zeros((4, lay.blocks_per_frame, 64), np.int16)
    qt = np.zeros((4, 3, 64), np.uint16)
    st = np.zeros(4, np.int32)
    arr = (C.c_char_p * 4)(*[os.fsencode(p) for p in paths])
    assert so.vge_jpeg_entropy_decode(arr, 4, 0, C.byref(lay), coef.ctypes.data, qt.ctypes.data, st.ctypes.data) == 8
    assert st.tolist() == [0, 8, 0, 8]
    fr, kept = load_frames(paths, device="cpu")
    assert kept.tolist() == [0, 2] and tuple(fr.shape) == (2, 48, 64, 3)


def test_missing_and_garbage_files_get_the_io_status(files, tmp_path):
    from vge.frames import load_frames, probe
    junk = tmp_path / "junk.jpg"
    junk.write_bytes(b"\xff\xd8 not a jpeg at all" * 8)
    info = probe([str(tmp_path / "absent.jpg"), str(junk)])
    assert info[:, 5].tolist() == [7, 7]
    fr, kept = load_frames([str(tmp_path / "absent.jpg"), files["batch_0"], str(junk)], device="cpu")
    assert kept.tolist() == [1] and fr.shape[0] == 1
    fr, kept = load_frames([str(junk)], device="cpu")
    assert kept.size == 0 and fr.shape[0] == 0


def test_block_beyond_the_32_bit_bound_is_refused(gold, tmp_path):
    """A frame whose dequantised block exceeds VGE_JPEG_BLOCK_L1_MAX (the reconstructs' 32-bit IDCT bound) is corrupt:
    the same stream with its quantisation table raised to 255 everywhere.  Host and device then agree on every frame
    they accept."""
    from vge.frames import load_frames
    data = bytearray(gold["jpeg/37x53_444_smooth"].tobytes())
    i = data.find(b"\xff\xdb")
    assert i > 0 and data[i + 4] == 0          # DQT, 8-bit table 0
    data[i + 5:i + 5 + 64] = b"\xff" * 64
    p = tmp_path / "loud.jpg"
    p.write_bytes(bytes(data))
    fr, kept = load_frames([str(p)], device="cpu")
    assert kept.size == 0


def test_idct_gain_behind_the_32_bit_bound():
    """The constants behind VGE_JPEG_BLOCK_L1_MAX (csrc/vge_jpeg_math.h): the largest multiplier of one input in one
    output of an 8-point pass is M = 11,363, and M (M S / 2048 + 12) + 2^17 < 2^31 at S = 32,767."""
    def one_pass(i):
        i0, i1, i2, i3, i4, i5, i6, i7 = i
        z1 = (i2 + i6) * 4433; t2 = z1 - i6 * 15137; t3 = z1 + i2 * 6270
        t0 = (i0 + i4) << 13; t1 = (i0 - i4) << 13
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        a, b, c, d = i7, i5, i3, i1
        z1, z2, z3, z4 = a + d, b + c, a + c, b + d
        z5 = (z3 + z4) * 9633
        a *= 2446; b *= 16819; c *= 25172; d *= 12299
        z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5
        a += z1 + z3; b += z2 + z4; c += z2 + z3; d += z1 + z4
        return [t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d]
    M = max(abs(v) for k in range(8) for v in one_pass([int(j == k) for j in range(8)]))
    assert M == 11363
    assert M * (M * 32767 // 2048 + 12) + (1 << 17) < (1 << 31)


def test_fresh_encodings_match_pillow(tmp_path):
    """Re-encode fresh random images and compare again: catches a stale fixture / another Pillow."""
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    from vge.frames import load_frames
    rng = np.random.default_rng(int.from_bytes(os.urandom(4), "little"))
    cases = [(2, 95, None), (1, 75, None), (0, 60, None), (2, 30, None), (None, 85, None)]
    cases += [(2, 90, (w, 7)) for w in (2, 3, 4, 5, 6)] + [(1, 90, (w, 5)) for w in (2, 3, 4, 5)]   # narrow chroma planes
    cases += [(2, 80, (200, 150)), (1, 80, (131, 70))]                                              # several kernel tiles
    for k, (sub, quality, size) in enumerate(cases):
        w, h = size or (int(rng.integers(1, 70)), int(rng.integers(1, 70)))
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        if k % 2 == 0:   # smoother content
            img = (img // 8 + np.linspace(0, 200, w, dtype=np.int64)[None, :, None]).astype(np.uint8)
        im = Image.fromarray(img)
        kw = {}
        if sub is None:
            im = im.convert("L")
        else:
            kw["subsampling"] = sub
        p = tmp_path / f"fresh_{k}.jpg"
        im.save(p, format="JPEG", quality=quality, **kw)
        ref = np.asarray(Image.open(p).convert("RGB"))
        fr, kept = load_frames([str(p)], device="cpu")
        assert kept.tolist() == [0]
        assert np.array_equal(fr[0].numpy(), ref), (w, h, sub, quality)


def test_tile_fixture_matches_pillow(gold, files):
    """The multi-tile fixture images carry no stored Pillow array; where Pillow imports they are checked here."""
    pytest.importorskip("PIL")
    from PIL import Image
    from vge.frames import load_frames
    for name in gold["tile_names"]:
        fr, _ = load_frames([files[name]], device="cpu")
        assert np.array_equal(fr[0].numpy(), np.asarray(Image.open(files[name]).convert("RGB"))), name


def test_list_frames_sorted_jpg_only(tmp_path):
    from vge.frames import list_frames
    for n in ("frame_000010.jpg", "frame_000002.jpg", "notes.txt", "frame_000001.JPG", "frame_000003.jpeg"):
        (tmp_path / n).write_bytes(b"x")
    assert [os.path.basename(p) for p in list_frames(tmp_path)] == ["frame_000002.jpg", "frame_000010.jpg"]


def test_load_videos_groups_sizes_and_keeps_order(gold, files):
    """Several videos in one call: videos of one size share a decode; results come back per video, in order."""
    from vge.frames import load_videos
    b = list(gold["batch_names"])
    vids = [[files[b[0]], files[b[1]]], [files["17x33_422_smooth"]], [files[b[2]], files["truncated"], files[b[3]]], []]
    res = load_videos(vids, device="cpu")
    assert [r[1].tolist() for r in res] == [[0, 1], [0], [0, 2], []]
    assert np.array_equal(res[0][0][1].numpy(), gold[f"rgb/{b[1]}"])
    assert np.array_equal(res[1][0][0].numpy(), gold["rgb/17x33_422_smooth"])
    assert np.array_equal(res[2][0][1].numpy(), gold[f"rgb/{b[3]}"])


def test_jpeg_kernel_has_no_scratch_and_no_flat_access():
    """The reconstruct kernel as built: no scratch, no FLAT memory instructions (tools/isa_guard.py, as
    tests/test_isa_guard.py reads the other hot kernels)."""
    import shutil
    lib = os.path.join(REPO, "video-gen-evals_amd", "vge", "libvge.so")
    if not shutil.which("objcopy") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("objcopy / ROCm llvm-objdump not available")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_guard
    hits = {k: v for k, v in isa_guard.kernels(lib).items() if "jpeg_reconstruct_kernel" in k}
    assert hits
    for name, r in hits.items():
        assert r["flat"] == 0, f"{name}: {r['flat']} FLAT memory instructions"
        assert r["scratch"] == 0 and r["scratch_ops"] == 0, f"{name}: {r['scratch']} B/lane scratch"
