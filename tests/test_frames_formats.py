"""What the three one-file video formats of vge.frames (GIF, lossless WebP, APNG) have in common, on files of a few
pixels written by the builders of tests/gif_cases.py, tests/webp_cases.py and tests/apng_cases.py: grouping by canvas
and the split of a group's frames back to the files, the frames kept in front of a corrupt one, the empty video, the
refusals by name and the order in which a call with several of them raises, the argument checks of decode_gifs /
decode_webps / decode_apngs, the probes from paths and from memory, and the frame counts the extraction driver takes
from the probe.  Two or three frames per file and three to six files per call: the smallest inputs at which grouping and
splitting can go wrong.  No GPU needed."""
import numpy as np
import pytest
import torch

from tests import apng_cases as AC
from tests import gif_cases as GC
from tests import png_cases as PC
from tests import webp_cases as WC

FORMATS = ("gif", "webp", "apng")
SUFFIX = {"gif": ".gif", "webp": ".webp", "apng": ".png"}
A, B = (5, 4), (3, 6)   # two canvases


def gif_file(canvas, seed, n=2, bad=None):
    """n whole-screen frames; frame `bad`'s LZW data ends half way through it."""
    w, h = canvas
    frames = []
    for k in range(n):
        idx = np.random.default_rng(seed + k).integers(0, 4, (h, w))
        if k == bad:
            codes = GC.lzw_encode(idx, 2)
            frames.append(GC.frame((0, 0, w, h), mcs=2, stream=GC.pack_codes(codes[:len(codes) // 2], 2), disposal=1))
        else:
            frames.append(GC.frame((0, 0, w, h), idx, mcs=2, disposal=1))
    return GC.gif(canvas, frames, GC.palette(seed, 4))


def webp_file(canvas, seed, n=2, bad=None):
    """n whole-canvas frames; frame `bad`'s VP8L stream ends half way through it."""
    w, h = canvas
    frames = []
    for k in range(n):
        pay = WC.vp8l(WC.rgb_to_argb(WC.picture(w, h, seed + k)))
        frames.append(WC.anmf(0, 0, w, h, pay[:len(pay) // 2] if k == bad else pay))
    return WC.animation(canvas, frames)


def apng_file(canvas, seed, n=2, bad=None, ct=6, **kw):
    """n whole-canvas frames of colour type ct; frame `bad`'s deflate stream opens with block type 3."""
    frames = [AC.full(seed + k, canvas, ct) for k in range(n)]
    if bad is not None:
        frames[bad] = AC.Spec(frames[bad].rect, frames[bad].px, stream=PC.zwrap(b"\x07" + bytes(40), b""))
    return AC.assemble(AC.chunks(canvas, ct, frames, **kw))


MAKE = {"gif": gif_file, "webp": webp_file, "apng": apng_file}
# a file with its format's signature and no frame
NO_FRAME = {"gif": b"GIF89a", "webp": WC.riff(WC.vp8x(5, 4) + WC.UNKNOWN), "apng": PC.SIG}
LOSSY = bytes([0x10, 0x02, 0x00, 0x9d, 0x01, 0x2a, 5, 0, 4, 0]) + bytes(range(30))   # a VP8 key frame's first bytes


def refused_file(fmt):
    """(file, exception class, the text behind the name) of a file the probe refuses by name."""
    from vge import frames as FR
    if fmt == "gif":
        idx = np.random.default_rng(9).integers(0, 4, (4, 5))
        return (GC.gif(A, [GC.frame((0, 0, 5, 4), idx, mcs=2)]), FR.UnsupportedGifError,
                "unsupported GIF: a frame without any colour table (ERR_NO_PALETTE)")
    if fmt == "webp":
        return (WC.riff(WC.chunk(b"VP8 ", LOSSY)), FR.UnsupportedWebpError,
                "unsupported WebP: a lossy (VP8 / ALPH) frame (ERR_LOSSY)")
    return apng_file(A, 9, lace=1), FR.UnsupportedPngError, "unsupported PNG: interlaced (ERR_INTERLACED)"


def too_many_groups():
    """A still WebP of 257 prefix-code groups: one more than the decoders hold, which the probe does not see."""
    g = np.zeros((1, 2), np.int64)
    g[0, 1] = WC.MAX_GROUPS
    return WC.still(WC.vp8l(WC.rgb_to_argb(WC.picture(9, 5, 3)), meta_bits=3, groups=g))


def write(tmp_path, fmt, blobs, stem="v"):
    paths = []
    for i, b in enumerate(blobs):
        paths.append(tmp_path / f"{stem}{i}{SUFFIX[fmt]}")
        paths[-1].write_bytes(b)
    return paths


def packed(blobs, lead=3, tail=2):
    """(data, offsets[F + 1]) with `lead` bytes in front of the first file and `tail` behind the last."""
    offsets = lead + np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.int64)
    data = np.frombuffer(b"\xa5" * lead + b"".join(blobs) + b"\xa5" * tail, np.uint8).copy()
    return torch.from_numpy(data), offsets


def decode_packed(fmt):
    from vge import frames as FR
    return {"gif": FR.decode_gifs, "webp": FR.decode_webps, "apng": FR.decode_apngs}[fmt]


def probes(fmt):
    from vge import frames as FR
    return {"gif": (FR.gif_probe, FR.gif_probe_mem, 6, 2), "webp": (FR.webp_probe, FR.webp_probe_mem, 6, 2),
            "apng": (FR.apng_probe, FR.apng_probe_mem, 10, 5), "png": (FR.png_probe, FR.png_probe_mem, 8, None)}[fmt]


def interleaved(fmt):
    """[(file, canvas, frames)]: two files of canvas A with one of canvas B between them; for APNG a fourth of canvas A
    and another colour type, which is a group of its own."""
    files = [(MAKE[fmt](A, 10, 2), A, 2), (MAKE[fmt](B, 20, 3), B, 3), (MAKE[fmt](A, 30, 3), A, 3)]
    if fmt == "apng":
        files.append((apng_file(A, 40, 2, ct=2), A, 2))
    return files


@pytest.mark.parametrize("fmt", FORMATS)
def test_interleaved_canvases_land_at_their_input_index(fmt, tmp_path):
    from vge import frames as FR
    files = interleaved(fmt)
    paths = write(tmp_path, fmt, [f for f, _, _ in files])
    out = FR.load_videos(paths, device="cpu", threads=2)
    assert len(out) == len(files)
    for p, (fr, kept), (_, canvas, n) in zip(paths, out, files):
        one, kept1 = FR.load_frames(p, device="cpu")
        assert kept.dtype == np.int64 and kept.tolist() == kept1.tolist() == list(range(n)), p
        assert fr.dtype == torch.uint8 and tuple(fr.shape) == (n, canvas[1], canvas[0], 3), p
        assert torch.equal(fr, one), p
    assert not torch.equal(out[0][0], out[2][0][:2])   # the two files of one canvas hold different pictures


@pytest.mark.parametrize("fmt", FORMATS)
def test_corrupt_frames_and_files_without_frames(fmt, tmp_path, caplog):
    """In one call: a good file, one whose second frame is corrupt, one with the signature and nothing else, one whose
    first frame is corrupt.  The log lines, in order and word for word."""
    from vge import frames as FR
    make = MAKE[fmt]
    paths = write(tmp_path, fmt, [make(A, 1, 2), make(A, 2, 3, bad=1), NO_FRAME[fmt], make(A, 3, 2, bad=0)])
    with caplog.at_level("WARNING", logger="vge.frames"):
        out = FR.load_videos(paths, device="cpu", threads=2)
    assert [r.getMessage() for r in caplog.records] == [
        f"no decodable frame in {paths[2]}: ERR_IO",
        f"dropping frames 1.. of {paths[1]}: ERR_IO",
        f"dropping frames 0.. of {paths[3]}: ERR_IO",
        f"no decodable frame in {paths[3]}"]
    assert [k.tolist() for _, k in out] == [[0, 1], [0], [], []]
    for fr, kept in (out[2], out[3]):
        assert kept.dtype == np.int64 and fr.dtype == torch.uint8
    assert tuple(out[2][0].shape) == (0, 0, 0, 3) and tuple(out[3][0].shape) == (0, 4, 5, 3)
    good, _ = FR.load_frames(paths[0], device="cpu")
    assert torch.equal(out[0][0], good)
    whole, _ = FR.load_frames(write(tmp_path, fmt, [make(A, 2, 3)], stem="whole")[0], device="cpu")
    assert torch.equal(out[1][0], whole[:1])


@pytest.mark.parametrize("fmt", FORMATS)
def test_refused_by_name(fmt, tmp_path):
    from vge import frames as FR
    blob, error, text = refused_file(fmt)
    good = MAKE[fmt](A, 1, 2)
    paths = write(tmp_path, fmt, [good, blob])
    for call in (lambda: FR.load_frames(paths[1], device="cpu"), lambda: FR.load_videos(paths, device="cpu")):
        with pytest.raises(error) as e:
            call()
        assert type(e.value) is error and str(e.value) == f"{paths[1]}: {text}"
    with pytest.raises(error) as e:
        decode_packed(fmt)(*packed([good, blob]), device="cpu")
    assert type(e.value) is error and str(e.value) == f"file 1: {text}"


def test_webp_refusal_that_only_the_decoder_sees(tmp_path):
    from vge import frames as FR
    text = "unsupported WebP: more prefix-code groups than the table arena holds (ERR_GROUPS)"
    paths = write(tmp_path, "webp", [webp_file(A, 1, 2), too_many_groups()])
    assert FR.webp_probe(paths)[:, 5].tolist() == [0, 0]
    with pytest.raises(FR.UnsupportedWebpError) as e:
        FR.load_videos(paths, device="cpu")
    assert str(e.value) == f"{paths[1]}: {text}"
    with pytest.raises(FR.UnsupportedWebpError) as e:
        FR.decode_webps(*packed([webp_file(A, 1, 2), too_many_groups()]), device="cpu")
    assert str(e.value) == f"file 1: {text}"


def test_a_refusable_file_of_each_format_raises_the_apng_files_error(tmp_path):
    """load_videos handles the formats in the order APNG, GIF, WebP; each format's refusals are raised when it is
    probed, so the APNG file's comes first wherever it stands in the call."""
    from vge import frames as FR
    paths = [write(tmp_path, fmt, [refused_file(fmt)[0]], stem="bad")[0] for fmt in ("gif", "webp", "apng")]
    with pytest.raises(FR.UnsupportedPngError) as e:
        FR.load_videos(paths, device="cpu")
    assert str(e.value) == f"{paths[2]}: {refused_file('apng')[2]}"
    with pytest.raises(FR.UnsupportedGifError) as e:
        FR.load_videos(paths[:2], device="cpu")
    assert str(e.value) == f"{paths[0]}: {refused_file('gif')[2]}"


@pytest.mark.parametrize("fmt", FORMATS)
def test_packed_argument_checks(fmt):
    decode = decode_packed(fmt)
    data, offsets = packed([MAKE[fmt](A, 1, 2), MAKE[fmt](B, 2, 2)], lead=0, tail=0)

    def refuses(message, *args, **kw):
        with pytest.raises(ValueError) as e:
            decode(*args, **{"device": "cpu", **kw})
        assert type(e.value) is ValueError and str(e.value) == message

    refuses("data must be a one-dimensional uint8 tensor", data.reshape(1, -1), offsets)
    refuses("data must be a one-dimensional uint8 tensor", data.to(torch.int16), offsets)
    refuses("data must be a one-dimensional uint8 tensor", data.numpy(), offsets)
    refuses("offsets must be int64 [F + 1]", data, offsets[:0])
    refuses("offsets must be int64 [F + 1]", data, offsets.reshape(1, -1))
    refuses("offsets must be non-decreasing and inside data", data, offsets[::-1].copy())
    refuses("offsets must be non-decreasing and inside data", data, offsets + 1)
    refuses("offsets must be non-decreasing and inside data", data, offsets - 1)
    refuses("entropy must be 'host' or 'device', not 'x'", data, offsets, entropy="x")
    refuses("entropy='device' needs a GPU", data, offsets, entropy="device")
    # the entropy words are checked in front of the offsets' values, and an empty call after them
    refuses("entropy must be 'host' or 'device', not 'x'", data, offsets[::-1].copy(), entropy="x")
    refuses("entropy='device' needs a GPU", data, offsets[:1], entropy="device")
    # file bytes that are not in host memory (a meta tensor stands in for a GPU's) are refused, not copied back
    walks = "data sub-block" if fmt == "gif" else "chunk"
    refuses(f"decode_{fmt}s needs the file bytes in host memory: the plan walks every {walks} on the host; pass a CPU "
            "tensor (entropy='device' uploads it once)", data.to("meta"), offsets)
    assert decode(data, offsets[:1], device="cpu") == []
    assert decode(data, torch.from_numpy(offsets[1:2]), device="cpu") == []


@pytest.mark.parametrize("fmt", FORMATS)
def test_packed_files_decode_as_their_paths_do(fmt, tmp_path, caplog):
    from vge import frames as FR
    blobs = [f for f, _, _ in interleaved(fmt)] + [NO_FRAME[fmt], MAKE[fmt](B, 50, 3, bad=2)]
    want = FR.load_videos(write(tmp_path, fmt, blobs), device="cpu", threads=2)
    data, offsets = packed(blobs)
    caplog.clear()
    with caplog.at_level("WARNING", logger="vge.frames"):
        for off in (offsets, torch.from_numpy(offsets)):
            got = decode_packed(fmt)(data, off, device="cpu", threads=2)
            assert len(got) == len(want) == len(blobs)
            for (fr, kept), (fr1, kept1) in zip(got, want):
                assert kept.dtype == np.int64 and kept.tolist() == kept1.tolist()
                assert fr.shape == fr1.shape and torch.equal(fr, fr1)
    n = len(blobs)
    assert [r.getMessage() for r in caplog.records] == 2 * [f"no decodable frame in file {n - 2}: ERR_IO",
                                                            f"dropping frames 2.. of file {n - 1}: ERR_IO"]


@pytest.mark.parametrize("fmt", FORMATS + ("png",))
def test_probe_from_paths_equals_probe_from_memory(fmt, tmp_path):
    probe, probe_mem, columns, count_col = probes(fmt)
    if fmt == "png":
        blobs = [PC.simple(PC.pixels(1, 4, 5, 2), 2), PC.simple(PC.pixels(2, 6, 3, 6), 6), PC.SIG]
        counts = None
    else:
        blobs = [MAKE[fmt](A, 1, 2), MAKE[fmt](B, 2, 3), NO_FRAME[fmt]]
        counts = [2, 3, 0]
    paths = write(tmp_path, "apng" if fmt == "png" else fmt, blobs)
    rows = probe(paths, 2)
    assert rows.dtype == np.int64 and rows.shape == (3, columns)
    assert rows[:, :2].tolist()[:2] == [list(A), list(B)] and rows[:, -1].tolist() == [0, 0, 7]
    if counts is not None:
        assert rows[:, count_col].tolist() == counts
    data, off, size = PC.pack(blobs, gap=3)
    assert np.array_equal(probe_mem(data, off, size, 2), rows)
    assert np.array_equal(probe_mem(data, off.astype(np.int32), size.astype(np.int32)), rows)   # any integer type
    assert np.array_equal(probe([str(p) for p in paths]), rows)
    for empty in (probe([]), probe_mem(data, off[:0], size[:0])):
        assert empty.dtype == np.int64 and empty.shape == (0, columns)


def test_only_a_webp_probe_gives_frames_on_a_canvas_without_size():
    """The group condition asks for frames, a status other than ERR_ARG and a positive width and height.  For GIF and
    APNG the last two follow from the first: no case file's probe row has frames on a canvas without width or height."""
    from vge import lib as L
    for cases, count_col in ((GC, 2), (AC, 5)):
        data, off, size = cases.pack([c.data for c in cases.cases()], gap=1)
        rows = cases.host_probe_mem(data, off, size)[1]
        assert len(rows) > 30 and ((rows[:, 0] <= 0) | (rows[:, 1] <= 0)).sum() >= 2
        assert not ((rows[:, count_col] > 0) & ((rows[:, 0] <= 0) | (rows[:, 1] <= 0))).any()
    # an APNG is refused by name in the words and under the status names of a still PNG
    assert L.APNG_UNSUPPORTED == L.PNG_UNSUPPORTED
    assert all(L.APNG_STATUS[s] == L.PNG_STATUS[s] for s in L.PNG_UNSUPPORTED)


@pytest.mark.parametrize("fmt", FORMATS)
def test_tree_driver_takes_the_frame_counts_from_the_probe(fmt, tmp_path):
    from tests.test_extract_tree import Calls, StubDetector, StubHmr, StubWholebody, stub_crop
    from vge.extract import extract_frame_tree
    root = tmp_path / "frames"
    (root / "Archery").mkdir(parents=True)
    paths = []
    for name, blob in (("v_a_01", MAKE[fmt](A, 1, 2)), ("v_a_02", MAKE[fmt](B, 2, 3)), ("v_a_03", NO_FRAME[fmt])):
        paths.append(root / "Archery" / (name + SUFFIX[fmt]))
        paths[-1].write_bytes(blob)
    counts = probes(fmt)[0](paths)[:, probes(fmt)[3]].tolist()
    assert counts == [2, 3, 0]
    calls = Calls()
    s = extract_frame_tree(StubHmr(calls), StubWholebody(calls), StubDetector(calls), root, tmp_path / "meshes",
                           tmp_path / "kps", tmp_path / "logs", device="cpu", crop=stub_crop, frame_format=fmt)
    # the stub detector sees two people on any frame that is not 64 wide
    assert s == {"Archery": {"single": [], "not_single": ["v_a_01", "v_a_02"], "errors": ["v_a_03"], "skipped": []}}
    for name, n in (("v_a_01", 2), ("v_a_02", 3)):
        assert np.load(tmp_path / "kps" / "Archery" / name / "keypoints.npy").shape == (n, 120)
    import json
    err = json.loads((tmp_path / "logs" / "errors" / "Archery.json").read_text())
    assert err == {"v_a_03": f"no decodable frame in {paths[2]}: not a {fmt.upper()}, truncated, or without an image"}
