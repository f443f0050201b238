"""The host half of the APNG front end (include/vge_apng.h, csrc/vge_apng.cpp) against what Pillow decodes from the
same files (tests/golden/apng_golden.npz, written by tests/golden/make_apng_golden.py) and against the numpy model of
the composition rule in tests/apng_cases.py: every accepted case byte for byte; for every refused case the expected
code on the expected frame, the later frames with it and the earlier frames standing with Pillow's pixels.  Then the
probe, the plan, the argument refusals, the Python loaders, the extraction driver on a tree of APNGs with stub models,
and the parser and decoder in a stand-alone program under the address and undefined-behaviour sanitizers.  No GPU and
no Pillow needed."""
import json
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import apng_cases as AC
from tests.conftest import GOLDEN, REPO


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "apng_golden.npz")


def decode_case(c):
    data, off, size = AC.pack([c.data], gap=4)
    _, rows = AC.host_probe_mem(data, off, size)
    n = int(rows[0, 5])
    rc, rgb, st, fst, total = AC.host_decode_mem(data, off, size, c.layout, n)
    assert total == n
    return rc, rgb, st, int(fst[0]), rows[0]


@pytest.fixture(scope="module")
def verdicts():
    """name -> (return code, frames, statuses, file status, probe row), every case decoded once."""
    return {c.name: decode_case(c) for c in AC.cases()}


def test_accepted_cases_equal_pillow_and_the_model(verdicts, gold):
    compared = 0
    for c in AC.cases():
        if not c.accept:
            continue
        rc, rgb, st, fst, row = verdicts[c.name]
        assert rc == 0 and fst == 0 and len(st) == c.n_frames > 0 and not st.any(), (c.name, st.tolist())
        assert int(gold[f"n/{c.name}"]) == c.n_frames, c.name
        pil = gold[f"rgb/{c.name}"]
        assert pil.shape == rgb.shape == c.want.shape, c.name
        for k in range(c.n_frames):
            assert np.array_equal(pil[k], rgb[k]), (c.name, k)
            assert np.array_equal(c.want[k], pil[k]), (c.name, k)
        compared += 1
    assert compared == sum(c.accept for c in AC.cases()) == 20


def test_refused_cases_fail_on_the_expected_frame(verdicts, gold):
    """The refused frame and every later one carry the code; the frames before it stand, with Pillow's pixels and the
    model's; inside the equality Pillow yields exactly those frames."""
    compared = 0
    for c in AC.cases():
        if c.accept:
            continue
        rc, rgb, st, fst, row = verdicts[c.name]
        assert rc == c.expect and fst == c.expect and len(st) == c.n_frames, (c.name, rc, fst, st.tolist())
        assert (st[:c.bad_frame] == 0).all() and (st[c.bad_frame:] == c.expect).all(), (c.name, st.tolist())
        if c.pillow:
            assert int(gold[f"n/{c.name}"]) == c.bad_frame, c.name
        for k in range(c.bad_frame):
            assert np.array_equal(gold[f"rgb/{c.name}"][k], rgb[k]) and np.array_equal(c.want[k], rgb[k]), (c.name, k)
        compared += 1
    assert compared == 16
    outside = sorted(c.name for c in AC.cases() if not c.accept and not c.pillow)
    assert outside == sorted(AC.OUTSIDE_PILLOW)


def test_the_blend_table_covers_every_alpha_against_every_value(gold):
    first, second = AC.blend_table()
    assert sorted(set(map(tuple, second.px[..., 2:].reshape(-1, 2)))) == [(v, a) for v in range(256) for a in range(256)]
    src, a, dst = second.px[..., :3].astype(np.int64), second.px[..., 3:].astype(np.int64), first.px[..., :3]
    t = src * a + dst * (255 - a) + 128
    assert np.array_equal(gold["rgb/blend_table"][1], ((t + (t >> 8)) >> 8).astype(np.uint8))
    assert not np.array_equal(gold["rgb/blend_table"][1], ((src * a + dst * (255 - a)) // 255).astype(np.uint8))


def test_probe_values():
    names = ["ops_ct2", "default_image", "split_chunks", "declares_more", "declares_fewer", "actl_after_idat", "still",
             "truncated", "rect_outside", "first_smaller", "interlaced", "depth16", "palette", "not_png", "empty_file",
             "other_canvas"]
    by_name = AC.by_name()
    data, off, size = AC.pack([by_name[n].data for n in names], gap=3)
    rc, rows = AC.host_probe_mem(data, off, size)
    assert rc == AC.ERR_IO   # the first failing file's code: the truncated one
    assert rows[0].tolist()[:7] == [37, 29, 2, 8, 0, 13, 0] and rows[0, -1] == 0
    assert rows[1].tolist()[:7] == [37, 29, 6, 8, 0, 4, 1] and rows[1, -1] == 0
    # chunks written: 7, 6, one per byte and 3, of which 2, 3, 0 and 0 are empty; the bytes are the four zlib streams
    streams = [AC.zstream(f) for f in _split_frames()]
    assert rows[2, 7] == 5 + 3 + len(streams[2]) + 3 and rows[2, 8] == sum(len(z) for z in streams)
    assert rows[3:7, 5].tolist() == [3, 2, 1, 1] and rows[3:7, -1].tolist() == [0] * 4
    assert rows[3:7, 6].tolist() == [0] * 4
    assert rows[7, 5] == 3 and rows[7, -1] == AC.ERR_IO
    assert rows[8, 5] == 4 and rows[8, -1] == AC.ERR_BOUNDS and rows[9, 5] == 2 and rows[9, -1] == AC.ERR_BOUNDS
    assert rows[10:15, 5].tolist() == [0] * 5
    assert rows[10:15, -1].tolist() == [AC.ERR_INTERLACED, AC.ERR_BITDEPTH, AC.ERR_PALETTE, AC.ERR_IO, AC.ERR_IO]
    assert rows[10].tolist()[:5] == [37, 29, 6, 8, 1] and rows[11, 3] == 16 and rows[12, 2] == 3
    assert rows[15].tolist()[:3] == [21, 16, 6] and rows[15, 5] == 2 and rows[15, -1] == 0   # the call's matter
    from vge import frames as FR
    assert np.array_equal(FR.apng_probe_mem(data, off, size), rows)


def _split_frames():
    C37 = (37, 29)
    return [AC.full(22, C37, 6), AC.sub(23, AC.BIG_37, 6), AC.sub(24, (5, 5, 1, 1), 6), AC.sub(25, AC.BIG_37, 6)]


def test_probe_and_decode_from_paths(tmp_path):
    from vge import frames as FR
    by_name = AC.by_name()
    paths = []
    for n in ("prev_twice", "default_image", "empty_file"):
        (tmp_path / f"{n}.png").write_bytes(by_name[n].data)
        paths.append(tmp_path / f"{n}.png")
    rows = FR.apng_probe(paths + [tmp_path / "missing.png"])
    assert rows[:, 5].tolist() == [4, 4, 0, 0] and rows[:, -1].tolist() == [0, 0, AC.ERR_IO, AC.ERR_IO]


def test_plan_descriptors_and_segments():
    by_name = AC.by_name()
    files = [by_name[n].data for n in ("split_chunks", "rgb_trns_over", "rect_outside", "not_png", "default_image")]
    data, off, size = AC.pack(files[:4], gap=5, order=[2, 0, 3, 1])
    rc, descs, nd, segs, ns, st, fst, ws = AC.host_plan_mem(data, off, size, (37, 29, 6))
    assert rc == AC.ERR_SHAPE and fst.tolist() == [0, AC.ERR_SHAPE, AC.ERR_BOUNDS, AC.ERR_IO]
    assert nd == 4 + 3 + 4 + 0 and st.tolist() == [0] * 4 + [AC.ERR_SHAPE] * 3 + [0, 0, AC.ERR_BOUNDS, AC.ERR_BOUNDS]
    assert [descs[k].file for k in range(nd)] == [0] * 4 + [1] * 3 + [2] * 4
    assert [descs[k].index for k in range(nd)] == [0, 1, 2, 3, 0, 1, 2, 0, 1, 2, 3]
    assert [descs[k].frame for k in range(nd)] == list(range(11))
    assert [descs[k].plan_status for k in range(nd)] == st.tolist()
    d = descs[1]
    assert (d.x, d.y, d.w, d.h, d.color_type, d.dispose_op, d.blend_op, d.trns) == (2, 1, 33, 27, 6, 0, 1, -1)
    assert d.file_off == off[0] and d.file_bytes == size[0] and d.raw_bytes == 27 * (1 + 33 * 4)
    # one segment per non-empty payload, back to back in the gathered run, an fdAT's source behind its sequence number
    mine = [segs[j] for j in range(ns) if segs[j].desc == 1]
    stream = AC.zstream(_split_frames()[1])
    assert [s.bytes for s in mine] == [3, 500, len(stream) - 503] and d.gat_bytes == len(stream)
    assert [s.dst_off for s in mine] == [d.gat_off, d.gat_off + 3, d.gat_off + 503]
    whole = bytes(data)
    got = b"".join(whole[s.src_off:s.src_off + s.bytes] for s in mine)
    assert got == stream
    assert whole[mine[0].src_off - 8:mine[0].src_off - 4] == b"fdAT"
    assert ns == 5 + 3 + len(AC.zstream(_split_frames()[2])) + 3 + 2
    assert descs[9].gat_bytes == 0 and descs[10].gat_bytes == 0   # refused frames own no segment
    lo = (nd * 8 + 15) & ~15
    for k in (0, 1, 2, 3, 7, 8):
        d = descs[k]
        assert d.gat_off >= lo and d.slot_off % 16 == 0 and d.gat_off + d.gat_bytes <= d.slot_off
        assert d.slot_off + d.raw_bytes <= ws
    # the tRNS colour travels in the descriptor; a default image is frame 0 with no operations
    data, off, size = AC.pack([files[1]])
    rc, descs, nd, segs, ns, st, fst, ws = AC.host_plan_mem(data, off, size, (37, 29, 2))
    assert rc == 0 and [descs[k].trns for k in range(nd)] == [17 | 34 << 8 | 51 << 16] * 3
    data, off, size = AC.pack([files[4]])
    rc, descs, nd, segs, ns, st, fst, ws = AC.host_plan_mem(data, off, size, (37, 29, 6))
    assert rc == 0 and nd == 4
    assert [(descs[k].dispose_op, descs[k].blend_op) for k in range(nd)] == [(0, 0), (2, 1), (0, 1), (0, 0)]
    assert (descs[0].x, descs[0].y, descs[0].w, descs[0].h) == (0, 0, 37, 29)
    from vge import lib as L
    assert L.load().vge_apng_decode_device_workspace_bytes(descs, nd) == ws


def test_packing_with_gaps_and_in_any_order(gold):
    by_name = AC.by_name()
    names = ["prev_first", "seq_fdat", "default_image", "other_canvas", "not_png", "bg_over_alpha0"]
    files = [by_name[n].data for n in names]
    want = None
    for gap, order in ((0, None), (7, [5, 3, 1, 0, 2, 4]), (33, [2, 4, 0, 5, 1, 3])):
        data, off, size = AC.pack(files, gap=gap, order=order)
        rc, rgb, st, fst, total = AC.host_decode_mem(data, off, size, (37, 29, 6), 3 + 4 + 4 + 2 + 0 + 3, threads=3)
        assert rc == AC.ERR_IO and total == 16
        assert fst.tolist() == [0, AC.ERR_IO, 0, AC.ERR_SHAPE, AC.ERR_IO, 0]
        assert st.tolist() == [0] * 3 + [0, 0, AC.ERR_IO, AC.ERR_IO] + [0] * 4 + [AC.ERR_SHAPE] * 2 + [0] * 3
        ok = st == 0
        if want is None:
            want = rgb[ok].copy()
            assert np.array_equal(rgb[:3], gold["rgb/prev_first"])
            assert np.array_equal(rgb[7:11], gold["rgb/default_image"])
            assert np.array_equal(rgb[13:], gold["rgb/bg_over_alpha0"])
        assert np.array_equal(rgb[ok], want)


def test_argument_refusals():
    import ctypes as C

    from vge import lib as L
    lib = L.load()
    c = AC.by_name()["prev_twice"]
    data, off, size = AC.pack([c.data, c.data], gap=4)
    # files outside the buffer and negative offsets: the file's own code, the other file decodes
    for bad_off, bad_size in ((-1, size[0]), (off[0], data.size), (data.size + 1, 0), (off[0], -1)):
        o, s = off.copy(), size.copy()
        o[0], s[0] = bad_off, bad_size
        rc, rows = AC.host_probe_mem(data, o, s)
        assert rc == AC.ERR_ARG and rows[:, -1].tolist() == [AC.ERR_ARG, 0]
        rc, rgb, st, fst, total = AC.host_decode_mem(data, o, s, c.layout, 4)
        assert rc == AC.ERR_ARG and fst.tolist() == [AC.ERR_ARG, 0] and total == 4 and st.tolist() == [0] * 4
        assert np.array_equal(rgb, c.want)
        rc, descs, nd, segs, ns, pst, pf, ws = AC.host_plan_mem(data, o, s, c.layout)
        assert rc == AC.ERR_ARG and pf.tolist() == [AC.ERR_ARG, 0] and nd == 4
    # capacities that are too small
    rc, _, _, _, total = AC.host_decode_mem(data, off, size, c.layout, 7)
    assert rc == AC.ERR_ARG and total == 8 and b"frame_cap" in lib.vge_last_error()
    _, _, nd, _, ns, _, _, _ = AC.host_plan_mem(data, off, size, c.layout)
    assert (nd, ns) == (8, 8)
    assert AC.host_plan_mem(data, off, size, c.layout, seg_cap=ns - 1)[0] == AC.ERR_ARG
    assert b"seg_cap" in lib.vge_last_error()
    assert AC.host_plan_mem(data, off, size, c.layout, desc_cap=nd - 1)[0] == AC.ERR_ARG
    # null pointers and a bad layout
    nd_, ns_ = C.c_int64(), C.c_int64()
    p = data.ctypes.data
    tail = (None, 0, C.byref(nd_), None, 0, C.byref(ns_), None, None, None)
    for w, h, ct in ((0, 29, 6), (37, 0, 6), (37, 29, 3), (37, 29, 5)):
        assert lib.vge_apng_plan_mem(p, data.size, off.ctypes.data, size.ctypes.data, 2, 1, w, h, ct, *tail) == AC.ERR_ARG
        assert lib.vge_apng_decode_mem(p, data.size, off.ctypes.data, size.ctypes.data, 2, 1, w, h, ct, 0, None, None,
                                       None, None) == AC.ERR_ARG
    assert lib.vge_apng_plan_mem(p, data.size, off.ctypes.data, size.ctypes.data, 2, 1, 37, 29, 6, None, 0, None, None,
                                 0, C.byref(ns_), None, None, None) == AC.ERR_ARG
    assert lib.vge_apng_decode_mem(p, data.size, off.ctypes.data, size.ctypes.data, 2, 1, 37, 29, 6, 8, None, None,
                                   None, None) == AC.ERR_ARG
    assert lib.vge_apng_probe_mem(None, 10, off.ctypes.data, size.ctypes.data, 2, 1, None) == AC.ERR_ARG
    assert lib.vge_apng_probe(None, 2, 1, None) == AC.ERR_ARG


def write_other_videos(root):
    jpeg = np.load(GOLDEN / "jpeg_golden.npz")
    png = np.load(GOLDEN / "png_golden.npz")
    gif = np.load(GOLDEN / "gif_golden.npz")
    (root / "jpg").mkdir()
    (root / "png").mkdir()
    (root / "jpg" / "frame_000000.jpg").write_bytes(jpeg[f"jpeg/{jpeg['batch_names'][0]}"].tobytes())
    (root / "png" / "frame_000000.png").write_bytes(png["png/rgb_l6"].tobytes())
    (root / "png" / "frame_000001.png").write_bytes(png["png/rgb_l6"].tobytes())
    (root / "clip.gif").write_bytes(gif["gif/rgb_optimize"].tobytes())
    return png["rgb/rgb_l6"], gif["rgb/rgb_optimize"]


def test_load_videos_on_paths_mixed_with_folders(tmp_path, caplog, gold):
    from vge import frames as FR
    by_name = AC.by_name()
    png_rgb, gif_rgb = write_other_videos(tmp_path)
    files = {"deltas.png": gold["apng/rgba_deltas"].tobytes(), "mixed.apng": gold["apng/rgb_mixed"].tobytes(),
             "ops.png": by_name["ops_ct4"].data, "broken.png": by_name["corrupt_deflate"].data,
             "dead.png": by_name["first_smaller"].data, "still.png": by_name["still"].data}
    for n, b in files.items():
        (tmp_path / n).write_bytes(b)
    vids = [tmp_path / "deltas.png", tmp_path / "jpg", tmp_path / "ops.png", tmp_path / "png", tmp_path / "broken.png",
            str(tmp_path / "mixed.apng"), tmp_path / "dead.png", tmp_path / "clip.gif", tmp_path / "still.png"]
    with caplog.at_level("WARNING", logger="vge.frames"):
        out = FR.load_videos(vids, device="cpu", threads=3)
    assert [k.tolist() for _, k in out] == [list(range(6)), [0], list(range(13)), [0, 1], [0, 1], list(range(6)), [],
                                            list(range(6)), [0]]
    assert np.array_equal(out[0][0].numpy(), gold["rgb/rgba_deltas"])
    assert np.array_equal(out[5][0].numpy(), gold["rgb/rgb_mixed"])
    assert np.array_equal(out[2][0].numpy(), gold["rgb/ops_ct4"])
    assert np.array_equal(out[4][0].numpy(), gold["rgb/corrupt_deflate"])
    assert np.array_equal(out[3][0][1].numpy(), png_rgb) and np.array_equal(out[7][0].numpy(), gif_rgb)
    assert np.array_equal(out[8][0].numpy(), by_name["still"].want)   # a still PNG file: a video of one frame
    assert "broken.png" in caplog.text and "dead.png" in caplog.text and "ERR_BOUNDS" in caplog.text
    one, kept = FR.load_frames(tmp_path / "deltas.png", device="cpu")
    assert kept.tolist() == list(range(6)) and torch.equal(one, out[0][0])
    # inside a folder or a list an APNG stays one still frame, its IDAT picture
    (tmp_path / "folder").mkdir()
    (tmp_path / "folder" / "a.png").write_bytes(by_name["ops_ct2"].data)
    (tmp_path / "folder" / "b.png").write_bytes(by_name["still"].data)
    fr, kept = FR.load_frames(tmp_path / "folder", device="cpu")
    assert kept.tolist() == [0, 1] and np.array_equal(fr[0].numpy(), gold["rgb/ops_ct2"][0])
    fr, kept = FR.load_frames([tmp_path / "folder" / "a.png"], device="cpu")
    assert kept.tolist() == [0] and np.array_equal(fr[0].numpy(), gold["rgb/ops_ct2"][0])
    for n in ("interlaced", "depth16", "palette"):
        (tmp_path / f"{n}.png").write_bytes(by_name[n].data)
        with pytest.raises(FR.UnsupportedPngError, match=f"{n}.png: unsupported PNG: " +
                           {"interlaced": "interlaced", "depth16": "not 8 bits", "palette": "palette"}[n]):
            FR.load_frames(tmp_path / f"{n}.png", device="cpu")
    with pytest.raises(ValueError):
        FR.load_frames(tmp_path / "deltas.png", device="cpu", entropy="device")


def test_decode_apngs_from_packed_host_memory(gold):
    from vge import frames as FR
    by_name = AC.by_name()
    files = [gold["apng/rgba_previous_over"].tobytes(), by_name["bands"].data, by_name["not_png"].data,
             by_name["seq_fdat"].data, gold["apng/rgb_deltas"].tobytes(), by_name["canvas_1x1"].data]
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    data = torch.from_numpy(np.frombuffer(b"".join(files), np.uint8).copy())
    out = FR.decode_apngs(data, offsets, device="cpu")
    assert [k.tolist() for _, k in out] == [list(range(6)), list(range(4)), [], [0, 1], list(range(6)), [0, 1, 2]]
    assert np.array_equal(out[0][0].numpy(), gold["rgb/rgba_previous_over"])
    assert np.array_equal(out[1][0].numpy(), gold["rgb/bands"])
    assert np.array_equal(out[4][0].numpy(), gold["rgb/rgb_deltas"])
    assert np.array_equal(out[5][0].numpy(), gold["rgb/canvas_1x1"])
    assert FR.decode_apngs(data, offsets[:1], device="cpu") == []
    with pytest.raises(ValueError):
        FR.decode_apngs(data, offsets[::-1].copy(), device="cpu")
    with pytest.raises(ValueError):
        FR.decode_apngs(data, offsets, device="cpu", entropy="device")
    both = files[0] + by_name["palette"].data
    with pytest.raises(FR.UnsupportedPngError, match="file 1"):
        FR.decode_apngs(torch.from_numpy(np.frombuffer(both, np.uint8).copy()),
                        np.array([0, len(files[0]), len(both)]), device="cpu")


def test_golden_files_on_the_host(gold):
    names = sorted(k[5:] for k in gold.files if k.startswith("apng/"))
    assert len(names) >= 5
    rects = set()
    for name in names:
        want = gold[f"rgb/{name}"]
        raw = gold[f"apng/{name}"]
        off, size = np.zeros(1, np.int64), np.array([raw.size], np.int64)
        _, rows = AC.host_probe_mem(raw, off, size)
        layout = (want.shape[2], want.shape[1], int(rows[0, 2]))
        rc, rgb, st, fst, total = AC.host_decode_mem(raw, off, size, layout, len(want))
        assert rc == 0 and total == len(want) and not st.any() and np.array_equal(rgb, want), name
        _, descs, nd, _, _, _, _, _ = AC.host_plan_mem(raw, off, size, layout)
        rects |= {(descs[k].w, descs[k].h) for k in range(nd)}
        assert {descs[k].dispose_op for k in range(nd)} <= {0, 1, 2} and {descs[k].blend_op for k in range(nd)} <= {0, 1}
    assert len(rects) > 2   # Pillow's own delta rectangles, not only whole frames


def test_tree_driver_on_apng_videos(tmp_path, gold, capsys):
    """extract_frame_tree(frame_format="apng") with stub models: bookkeeping, frame_idx, the messages that name the
    file, the .png / .apng collision, resume."""
    from tests.test_extract_tree import Calls, StubDetector, StubHmr, StubWholebody, stub_crop
    from vge.extract import extract_frame_tree
    by_name = AC.by_name()
    root = tmp_path / "frames"
    (root / "Archery").mkdir(parents=True)
    (root / "Bowling").mkdir(parents=True)
    (root / "Archery" / "v_a_01.png").write_bytes(gold["apng/rgba_deltas"].tobytes())
    (root / "Archery" / "v_a_02.apng").write_bytes(gold["apng/rgb_mixed"].tobytes())
    (root / "Archery" / "v_a_03.png").write_bytes(by_name["not_png"].data)       # loses against its .apng twin
    (root / "Archery" / "v_a_03.apng").write_bytes(gold["apng/rgb_deltas"].tobytes())
    (root / "Archery" / "notes.txt").write_text("not a video")
    (root / "Bowling" / "v_b_01.png").write_bytes(by_name["corrupt_deflate"].data)   # 2 of 4 frames
    (root / "Bowling" / "v_b_02.png").write_bytes(by_name["not_png"].data)
    (root / "Bowling" / "v_b_03.png").write_bytes(by_name["first_smaller"].data)
    calls = Calls()

    def run(**kw):
        return extract_frame_tree(StubHmr(calls), StubWholebody(calls), StubDetector(calls), root, tmp_path / "meshes",
                                  tmp_path / "kps", tmp_path / "logs", device="cpu", crop=stub_crop,
                                  **dict(dict(frame_format="apng"), **kw))
    s = run()
    assert s == {"Archery": {"single": ["v_a_01", "v_a_02", "v_a_03"], "not_single": [], "errors": [], "skipped": []},
                 "Bowling": {"single": [], "not_single": ["v_b_01"], "errors": ["v_b_02", "v_b_03"], "skipped": []}}
    said = capsys.readouterr().out
    assert "v_a_03.png" in said and "using v_a_03.apng" in said
    z = np.load(tmp_path / "meshes" / "Archery" / "v_a_01.npz")
    rgb = gold["rgb/rgba_deltas"]
    np.testing.assert_array_equal(z["frame_idx"], np.arange(6))
    np.testing.assert_allclose(z["vit"][:, :3], rgb.astype(np.float32).mean(axis=(1, 2)), rtol=1e-6)
    np.testing.assert_array_equal(z["vit"][:, 3:], rgb[:, 0, 0].astype(np.float32))
    meta = json.loads(str(z["meta"]))
    assert meta == {"action": "Archery", "video": "v_a_01", "source_path": str(root / "Archery" / "v_a_01.png")}
    z3 = np.load(tmp_path / "meshes" / "Archery" / "v_a_03.npz")
    assert json.loads(str(z3["meta"]))["source_path"] == str(root / "Archery" / "v_a_03.apng")
    np.testing.assert_array_equal(z3["vit"][:, 3:], gold["rgb/rgb_deltas"][:, 0, 0].astype(np.float32))
    assert np.load(tmp_path / "kps" / "Bowling" / "v_b_01" / "keypoints.npy").shape == (2, 120)
    err = json.loads((tmp_path / "logs" / "errors" / "Bowling.json").read_text())
    assert "v_b_02.png" in err["v_b_02"] and "v_b_03.png" in err["v_b_03"] and "2 frames" in err["v_b_03"]
    before = dict(calls.n)
    s2 = run()
    assert s2["Archery"]["skipped"] == ["v_a_01", "v_a_02", "v_a_03"] and s2["Bowling"]["errors"] == ["v_b_02", "v_b_03"]
    assert calls.n == before   # nothing decodable was left to do
    with pytest.raises(ValueError, match="webp"):
        run(frame_format="bmp")


SANITIZED_MAIN = r"""
// Runs the host APNG parser and decoder over the files listed in argv[1] (lines: path width height colour_type).
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "include/vge_apng.h"
namespace vge { void set_last_error(const std::string&) {} }
extern "C" int vge_ingest_default_threads(void) { return 2; }
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char path[4096];
  int w, h, ct, n = 0, bad = 0;
  while (fscanf(f, "%4095s %d %d %d", path, &w, &h, &ct) == 4) {
    FILE* g = fopen(path, "rb");
    if (!g) return 2;
    std::vector<uint8_t> own;  // the exact file bytes in a heap block of their own: a read past either end is seen
    int c;
    while ((c = fgetc(g)) != EOF) own.push_back((uint8_t)c);
    fclose(g);
    own.shrink_to_fit();
    if (own.empty()) own.reserve(1);
    int64_t zero = 0, size = (int64_t)own.size(), total = 0, nd = 0, ns = 0, ws = 0;
    vge_apng_info info, info2;
    memset(&info, 0, sizeof(info));
    memset(&info2, 0, sizeof(info2));
    const char* p = path;
    vge_apng_probe(&p, 1, 1, &info);
    vge_apng_probe_mem(own.data(), size, &zero, &size, 1, 1, &info2);
    if (memcmp(&info, &info2, sizeof(info)) != 0 && size > 0) ++bad;
    const int64_t cap = info2.n_frames;
    std::vector<uint8_t> rgb((size_t)(cap + 1) * w * h * 3), rgb2(rgb.size());
    std::vector<int32_t> st((size_t)cap + 1, -1), st2((size_t)cap + 1, -1);
    int32_t fst = -1, fst2 = -1, pst = -1;
    vge_apng_decode(&p, 1, 2, w, h, ct, cap, rgb.data(), st.data(), &fst, &total);
    vge_apng_decode_mem(own.data(), size, &zero, &size, 1, 2, w, h, ct, cap, rgb2.data(), st2.data(), &fst2, &total);
    if (total != cap || (fst != fst2 && size > 0)) ++bad;
    for (int64_t k = 0; k < cap; ++k)
      if (st[k] != st2[k] || (st[k] == 0 && memcmp(&rgb[k * w * h * 3], &rgb2[k * w * h * 3], (size_t)w * h * 3) != 0))
        ++bad;
    std::vector<vge_apng_desc> descs((size_t)cap + 1);
    std::vector<vge_apng_segment> segs((size_t)info2.n_chunks + 1);
    std::vector<int32_t> plan((size_t)cap + 1, -1);
    vge_apng_plan_mem(own.data(), size, &zero, &size, 1, 1, w, h, ct, descs.data(), cap, &nd, segs.data(),
                      info2.n_chunks, &ns, plan.data(), &pst, &ws);
    if (nd != cap || ns > info2.n_chunks || vge_apng_decode_device_workspace_bytes(descs.data(), (int)nd) != (size_t)ws)
      ++bad;
    for (int64_t j = 0; j < ns; ++j)  // every segment lies inside the file and inside its frame's gathered run
      if (segs[j].src_off < 0 || segs[j].bytes < 1 || segs[j].src_off + segs[j].bytes > size || segs[j].desc < 0 ||
          segs[j].desc >= nd || segs[j].dst_off < descs[segs[j].desc].gat_off ||
          segs[j].dst_off + segs[j].bytes > descs[segs[j].desc].gat_off + descs[segs[j].desc].gat_bytes)
        ++bad;
    for (int64_t k = 0; k < nd; ++k)  // every planned rectangle lies inside the canvas
      if (descs[k].plan_status == 0 && (descs[k].w < 1 || descs[k].h < 1 || descs[k].x < 0 || descs[k].y < 0 ||
                                        descs[k].x + descs[k].w > w || descs[k].y + descs[k].h > h))
        ++bad;
    ++n;
  }
  fclose(f);
  printf("%d files, %d mismatches\n", n, bad);
  return bad ? 1 : 0;
}
"""


def mutations(count, seed=5):
    """(case name, byte position, new byte): single-byte changes of the small case files, weighted towards the chunk
    headers and the control chunks in front of the pixels."""
    rng = np.random.default_rng(seed)
    small = [c for c in AC.cases() if 0 < len(c.data) < 20000]
    out = []
    for i in range(count):
        c = small[int(rng.integers(len(small)))]
        at = int(rng.integers(min(len(c.data), 120))) if i % 2 else int(rng.integers(len(c.data)))
        out.append((c.name, at, int(rng.integers(256))))
    return out


def test_host_parser_and_decoder_under_sanitizers(tmp_path):
    """A stand-alone program (its own main, nothing loaded into python) links vge_apng.cpp built with
    -fsanitize=address,undefined and runs the probe, the decoder and the plan over every case file and over a few
    hundred single-byte mutations of them (fixed seed), from the path and from an exactly-sized heap copy."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    (tmp_path / "main.cpp").write_text(SANITIZED_MAIN)
    by_name = AC.by_name()
    lines = []
    for c in AC.cases():
        p = tmp_path / f"{c.name}.png"
        p.write_bytes(c.data)
        lines.append(f"{p} {c.layout[0]} {c.layout[1]} {c.layout[2]}")
    muts = mutations(300)
    assert len(muts) == 300 and muts == mutations(300)
    for i, (name, at, byte) in enumerate(muts):
        b = bytearray(by_name[name].data)
        b[at] = byte
        p = tmp_path / f"mut_{i:03d}.png"
        p.write_bytes(bytes(b))
        lay = by_name[name].layout
        lines.append(f"{p} {lay[0]} {lay[1]} {lay[2]}")
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    exe = tmp_path / "apng_asan"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", str(REPO), str(tmp_path / "main.cpp"),
                            str(REPO / "video-gen-evals_amd" / "csrc" / "vge_apng.cpp"), "-o", str(exe), "-lz",
                            "-lpthread"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe), str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert f"{len(lines)} files, 0 mismatches" in run.stdout
