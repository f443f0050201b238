"""The host half of the lossless WebP front end (include/vge_webp.h, csrc/vge_webp.cpp) against Pillow, opened at test
time with ImageSequence-style seeking and .convert("RGB"): every accepted case byte for byte; every case Pillow refuses
is refused, on the frame Pillow raises on.  Then the coverage of the format by the cases (the host decoder reports what
each file exercised), the probe, the plan, the argument refusals, the Python loaders, the extraction driver's WebP
branch with stub models, and the parser and decoder in a stand-alone program under the address and
undefined-behaviour sanitizers.  No GPU needed."""
import shutil
import subprocess

import numpy as np
import pytest
import torch

from PIL import Image  # noqa: F401  the independent truth of this file: a missing Pillow is a failure, not a skip

from tests import webp_cases as WC
from tests.conftest import GOLDEN, REPO


def decode_case(c, gap=4, fill=0xA5):
    data, off, size = WC.pack([c.data], gap=gap, fill=fill)
    _, rows = WC.host_probe_mem(data, off, size)
    n = int(rows[0, 2])
    if c.canvas[0] < 1:   # no canvas to decode on: the probe's verdict is the file's
        return 0, None, np.full(n, int(rows[0, 5]), np.int32), int(rows[0, 5]), rows[0]
    rc, rgb, st, fst, total = WC.host_decode_mem(data, off, size, c.canvas, n)
    assert total == n
    return rc, rgb, st, int(fst[0]), rows[0]


@pytest.fixture(scope="module")
def verdicts():
    """name -> (return code, frames, statuses, file status, probe row), every case decoded once."""
    return {c.name: decode_case(c) for c in WC.cases()}


def test_accepted_cases_equal_pillow(verdicts):
    compared = 0
    for c in WC.cases():
        if not c.accept:
            continue
        rc, rgb, st, fst, row = verdicts[c.name]
        assert rc == 0 and fst == 0 and st.tolist() == [0] * c.n_frames, (c.name, st.tolist())
        assert (int(row[0]), int(row[1])) == c.canvas and int(row[5]) == 0, c.name
        frames, raised = WC.pillow_frames(c.data)
        assert raised is None and len(frames) == c.n_frames, (c.name, raised)
        for k, f in enumerate(frames):
            assert np.array_equal(rgb[k], f), (c.name, k, int((rgb[k] != f).any(-1).sum()))
            compared += 1
    assert compared >= 90


def test_refused_cases_are_refused_where_pillow_refuses(verdicts):
    """The statuses are the ones the cases were built for: the frames in front of the refused one stand (and are
    Pillow's where Pillow shows them), the refused one and every later one carry its code.  Outside OUTSIDE_PILLOW,
    Pillow raises on that very frame."""
    seen = set()
    for c in WC.cases():
        if c.accept:
            continue
        rc, rgb, st, fst, row = verdicts[c.name]
        n = int(row[2])
        assert n == c.n_frames, (c.name, n)
        bad = c.bad_frame or 0
        assert st.tolist() == [0] * bad + [c.expect] * (n - bad), (c.name, st.tolist())
        assert fst == c.expect and (rc == c.expect or c.canvas[0] < 1), (c.name, fst, rc)
        frames, raised = WC.pillow_frames(c.data)
        if c.name in WC.OUTSIDE_PILLOW:
            seen.add(c.name)
        else:
            assert raised == bad, (c.name, raised, bad)
        for k in range(min(bad, len(frames))):
            assert np.array_equal(rgb[k], frames[k]), (c.name, k)
    assert seen == set(WC.OUTSIDE_PILLOW)
    for name in ("lossy_frame_2", "bounds", "stream_ends_frame_1"):   # the earlier frames stand
        assert (verdicts[name][2] == 0).sum() >= 1


def test_the_cases_cover_the_format():
    """The host decoder reports what each file made it do.  The union over the accepted cases must hold every
    predictor mode, every transform alone and all four together, both code forms with their corner cases, the colour
    cache in the image and in a sub-image, one and many groups, every distance-map code, plain, clamped, overlapping
    and far copies, every bundling and an index beyond the palette."""
    mask, codes, most = 0, set(), 0
    alone = set()
    for c in WC.cases():
        if not c.accept:
            continue
        rc, f, dc, g = WC.features(c.data)
        assert rc == 0, c.name
        mask |= f
        codes |= dc
        most = max(most, g)
        x = (f >> WC.F_XFORM0) & 15
        if x in (1, 2, 4, 8):
            alone.add(x)
    missing = [k for k in range(44) if not (mask >> k) & 1]
    assert not missing, missing
    assert codes == set(range(1, 121))
    assert alone == {1, 2, 4, 8}
    assert most == WC.MAX_GROUPS   # groups_256 sits exactly at the arena's capacity
    rc, _, _, g = WC.features(next(c.data for c in WC.cases() if c.name == "groups_257"))
    assert rc == WC.ERR_GROUPS and g == WC.MAX_GROUPS + 1


def test_probe_and_plan_counts_are_consistent(verdicts):
    for canvas, group in WC.by_canvas().items():
        data, off, size = WC.pack([c.data for c in group], gap=7)
        rc_p, rows = WC.host_probe_mem(data, off, size)
        total = int(rows[:, 2].sum())
        rc_d, rgb, st, fst, n = WC.host_decode_mem(data, off, size, canvas, total)
        rc, descs, nd, plan_st, plan_fst, ws = WC.host_plan_mem(data, off, size, canvas)
        assert n == nd == total
        from vge import lib as L
        assert L.load().vge_webp_decode_device_workspace_bytes(descs, nd) == ws and ws % 16 == 0
        k = 0
        for i, c in enumerate(group):
            for j in range(int(rows[i, 2])):
                d = descs[k]
                assert (d.file, d.index, d.frame) == (i, j, k)
                assert plan_st[k] == d.plan_status
                if d.plan_status == 0:
                    assert d.file_off == off[i] and d.file_bytes == size[i] and d.slot_off % 16 == 0
                    assert 0 < d.pay_off and d.pay_off + d.pay_bytes <= size[i]
                    assert L.load().vge_webp_slot_bytes(d.w, d.h) > 2 * 4 * d.w * d.h
                else:   # what the plan refuses, the decoder refuses with the same code
                    assert st[k] == d.plan_status, (c.name, j)
                k += 1
            # the plan sees container errors only: a stream error is the decoder's
            assert plan_fst[i] in (0, fst[i]), c.name
        # the single-file verdicts again, in company
        k = 0
        for i, c in enumerate(group):
            n_i = int(rows[i, 2])
            if c.canvas == canvas:
                assert st[k:k + n_i].tolist() == verdicts[c.name][2].tolist(), c.name
            k += n_i


def test_packed_memory_order_gaps_and_capacity():
    by_name = {c.name: c for c in WC.cases()}
    names = ("anim_hand", "cut_2", "anim_alpha_rules", "shape_64x66", "bounds")
    files = [by_name[n].data for n in names]
    canvas = (40, 30)
    data, off, size = WC.pack(files, gap=5, order=[4, 2, 0, 3, 1])
    rc, rgb, st, fst, total = WC.host_decode_mem(data, off, size, canvas, 18)
    assert total == 8 + 0 + 6 + 1 + 3 and rc == WC.ERR_IO
    assert fst.tolist() == [0, WC.ERR_IO, 0, WC.ERR_SHAPE, WC.ERR_BOUNDS]
    assert st.tolist() == [0] * 14 + [WC.ERR_SHAPE] + [0] + [WC.ERR_BOUNDS] * 2
    data2, off2, size2 = WC.pack(files, gap=0)
    _, rgb2, st2, _, _ = WC.host_decode_mem(data2, off2, size2, canvas, 18)
    ok = st == 0
    assert st2.tolist() == st.tolist() and np.array_equal(rgb[ok], rgb2[ok])
    # a capacity one short: nothing is decoded
    rc, rgb3, st3, _, total = WC.host_decode_mem(data, off, size, canvas, 17)
    assert rc == WC.ERR_ARG and total == 18 and (rgb3 == 0x5A).all() and (st3 == -1).all()
    rc, _, nd, _, _, _ = WC.host_plan_mem(data, off, size, canvas, desc_cap=17)
    assert rc == WC.ERR_ARG and nd == 18
    # a file outside the buffer: refused unread
    off_bad = off.copy()
    off_bad[0] = data.size - 3
    rc, _, st4, fst4, _ = WC.host_decode_mem(data, off_bad, size, canvas, 18)
    assert fst4[0] == WC.ERR_ARG and st4[:10].tolist() == [0] * 6 + [WC.ERR_SHAPE] + [0] + [WC.ERR_BOUNDS] * 2


def test_bad_arguments():
    from vge import lib as L
    lib = L.load()
    data, off, size = WC.pack([WC.cases()[0].data])
    out, st = np.zeros((1, 9, 17, 3), np.uint8), np.zeros(1, np.int32)
    p = WC._ptr
    for w, h, cap, rgb in ((0, 9, 1, p(out)), (17, 0, 1, p(out)), (16385, 9, 1, p(out)), (17, 9, -1, p(out)),
                           (17, 9, 1, None)):
        assert lib.vge_webp_decode_mem(p(data), data.size, p(off), p(size), 1, 1, w, h, cap, rgb, p(st), None,
                                       None) == WC.ERR_ARG
        assert b"vge_webp_decode_mem" in lib.vge_last_error()
    assert lib.vge_webp_decode_mem(None, data.size, p(off), p(size), 1, 1, 17, 9, 1, p(out), p(st), None, None) == 1
    assert lib.vge_webp_probe_mem(p(data), data.size, p(off), p(size), 1, 1, None) == WC.ERR_ARG
    assert lib.vge_webp_plan_mem(p(data), data.size, p(off), p(size), 1, 1, 17, 9, None, 0, None, None, None, None) == 1


def test_mutations_terminate_and_read_only_their_file():
    """A few hundred seeded byte mutations of valid files: every one is decoded (or refused) without a crash, with one
    status per frame, and the verdict and pixels do not depend on what lies around the file in memory."""
    muts = WC.mutations(300)
    assert len(muts) == 300 and muts == WC.mutations(300)
    accepted = 0
    for name, blob in muts:
        results = []
        for fill in (0xA5, 0x00):
            data, off, size = WC.pack([blob], gap=64, fill=fill)
            _, rows = WC.host_probe_mem(data, off, size)
            n, w, h = int(rows[0, 2]), int(rows[0, 0]), int(rows[0, 1])
            if n == 0 or not (0 < w <= 256 and 0 < h <= 256):
                results.append((rows[0].tolist(),))
                continue
            rc, rgb, st, fst, total = WC.host_decode_mem(data, off, size, (w, h), n)
            assert total == n and ((st == 0) | (st == st[st != 0][:1].sum())).all(), name
            results.append((rows[0].tolist(), st.tolist(), rgb[st == 0].tobytes()))
            accepted += int((st == 0).any() and fill == 0)
        assert results[0] == results[1], name
    assert accepted >= 30   # the mutations are not all rejected at the door: some reach the pixel loop


# ------------------------------------------------------------------------------------------ loaders

@pytest.fixture(scope="module")
def webp_files(tmp_path_factory):
    root = tmp_path_factory.mktemp("webp")
    by_name = {c.name: c for c in WC.cases()}
    paths = {}
    for name in ("anim_hand", "pil_anim_rgba", "shape_64x66", "stream_ends_frame_1", "lossy_still", "bounds",
                 "groups_257", "cut_1"):
        paths[name] = root / f"{name}.webp"
        paths[name].write_bytes(by_name[name].data)
    return root, paths, by_name


def test_loaders(webp_files):
    from vge import frames as FR
    from vge import lib as L
    root, paths, by_name = webp_files
    want = np.stack(WC.pillow_frames(by_name["anim_hand"].data)[0])
    fr, kept = FR.load_frames(paths["anim_hand"], device="cpu")
    assert kept.tolist() == list(range(8)) and fr.dtype == torch.uint8 and np.array_equal(fr.numpy(), want)
    fr, kept = FR.load_frames(str(paths["stream_ends_frame_1"]), device="cpu")   # frames from the bad one on are dropped
    assert kept.tolist() == [0] and tuple(fr.shape) == (1, 9, 17, 3)
    vids = FR.load_videos([paths["pil_anim_rgba"], paths["anim_hand"], paths["shape_64x66"], paths["cut_1"]],
                          device="cpu", threads=2)
    assert [k.tolist() for _, k in vids] == [[0, 1, 2, 3], list(range(8)), [0], []]
    assert np.array_equal(vids[0][0].numpy(), np.stack(WC.pillow_frames(by_name["pil_anim_rgba"].data)[0]))
    assert np.array_equal(vids[1][0].numpy(), want)
    rows = FR.webp_probe([paths["anim_hand"], paths["lossy_still"]])
    assert rows[:, :3].tolist() == [[40, 30, 8], [17, 9, 1]] and rows[:, 5].tolist() == [0, WC.ERR_LOSSY]
    for name, word in (("lossy_still", "lossy"), ("bounds", "outside the canvas"), ("groups_257", "groups")):
        with pytest.raises(FR.UnsupportedWebpError, match=word) as e:
            FR.load_frames(paths[name], device="cpu")
        assert paths[name].name in str(e.value) and issubclass(FR.UnsupportedWebpError, L.VgeError)
    with pytest.raises(ValueError, match="entropy"):
        FR.load_frames(paths["anim_hand"], device="cpu", entropy="gpu")
    # files packed in memory
    raw = [paths[n].read_bytes() for n in ("anim_hand", "shape_64x66", "cut_1")]
    data, off, size = WC.pack(raw)
    offsets = np.concatenate([off, [off[-1] + size[-1]]])
    packed = FR.decode_webps(torch.from_numpy(data), offsets, device="cpu", threads=2)
    assert [k.tolist() for _, k in packed] == [list(range(8)), [0], []]
    assert np.array_equal(packed[0][0].numpy(), want)
    assert FR.decode_webps(torch.zeros(0, dtype=torch.uint8), np.zeros(1, np.int64), device="cpu") == []
    with pytest.raises(ValueError, match="offsets"):
        FR.decode_webps(torch.from_numpy(data), offsets[::-1].copy(), device="cpu")
    with pytest.raises(ValueError, match="needs a GPU"):
        FR.decode_webps(torch.from_numpy(data), offsets, device="cpu", entropy="device")


def test_a_folder_of_still_frames(tmp_path):
    from vge import frames as FR
    stills, want = [], []
    for k in range(4):
        rgb = WC.picture(20, 13, 40 + k)
        stills.append(WC.still(WC.all_features(rgb, seed=k)))
        want.append(rgb)
    folder = tmp_path / "clip"
    folder.mkdir()
    for k, b in enumerate(stills):
        (folder / f"{k:04d}.webp").write_bytes(b)
    assert [p[-9:] for p in FR.list_frames(folder, ext=".webp")] == [f"{k:04d}.webp" for k in range(4)]
    fr, kept = FR.load_frames(folder, device="cpu")
    assert kept.tolist() == [0, 1, 2, 3] and np.array_equal(fr.numpy(), np.stack(want))
    (folder / "0002.webp").write_bytes(stills[2][:len(stills[2]) // 2])       # unreadable: dropped, as a JPEG would be
    fr, kept = FR.load_frames(sorted(folder.iterdir()), device="cpu")
    assert kept.tolist() == [0, 1, 3] and np.array_equal(fr.numpy(), np.stack(want)[[0, 1, 3]])
    (folder / "0002.webp").write_bytes(WC.still(WC.all_features(WC.picture(21, 13, 1))))
    with pytest.raises(ValueError, match="one size") as e:
        FR.load_frames(folder, device="cpu")
    assert "0002.webp" in str(e.value)


def test_tree_driver_reads_webp_videos(tmp_path, webp_files):
    """extract_frame_tree(frame_format="webp") with stub models: the probe's frame counts pack the passes, the frames
    are the file's frames, an undecodable file is recorded under its name and the job goes on."""
    from tests.test_extract_tree import Calls, StubDetector, StubHmr, StubWholebody, stub_crop
    from vge.extract import extract_frame_tree
    _, paths, by_name = webp_files
    root = tmp_path / "frames"
    (root / "Archery").mkdir(parents=True)
    shutil.copy(paths["anim_hand"], root / "Archery" / "v_a_01.webp")
    shutil.copy(paths["stream_ends_frame_1"], root / "Archery" / "v_a_02.webp")
    shutil.copy(paths["cut_1"], root / "Archery" / "v_a_03.webp")
    (root / "Archery" / "notes.gif").write_bytes(b"GIF89a")     # another format's file is not a video of this tree
    calls = Calls()
    s = extract_frame_tree(StubHmr(calls), StubWholebody(calls), StubDetector(calls), root, tmp_path / "meshes",
                           tmp_path / "kps", tmp_path / "logs", device="cpu", crop=stub_crop, frame_format="webp")
    assert s["Archery"]["errors"] == ["v_a_03"] and sorted(s["Archery"]["single"] + s["Archery"]["not_single"]) == [
        "v_a_01", "v_a_02"]
    with pytest.raises(ValueError, match="webp"):
        extract_frame_tree(None, None, None, root, tmp_path / "m", tmp_path / "k", tmp_path / "l", frame_format="bmp")


def test_golden_files_hold_pillows_pixels():
    """tests/golden/webp_golden.npz (make_webp_golden.py): the host decoder gives the stored pixels, and so does the
    Pillow of this machine."""
    gold = np.load(GOLDEN / "webp_golden.npz")
    names = sorted(k[5:] for k in gold.files if k.startswith("webp/"))
    assert len(names) >= 6
    for name in names:
        blob, want = gold[f"webp/{name}"].tobytes(), gold[f"rgb/{name}"]
        data, off, size = WC.pack([blob], gap=2)
        rc, rgb, st, _, total = WC.host_decode_mem(data, off, size, (want.shape[2], want.shape[1]), len(want))
        assert rc == 0 and total == len(want) and st.tolist() == [0] * len(want) and np.array_equal(rgb, want), name
        frames, raised = WC.pillow_frames(blob)
        assert raised is None and np.array_equal(np.stack(frames), want), name


# ------------------------------------------------------------------------------------------ sanitizers

SANITIZED_MAIN = r"""
// Runs the host WebP parser and decoder over the files listed in argv[1] (lines: path).
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "include/vge_webp.h"
namespace vge { void set_last_error(const std::string&) {} }
extern "C" int vge_ingest_default_threads(void) { return 2; }
extern "C" int vge_debug_webp_features(const uint8_t* data, int64_t bytes, uint64_t* out);
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char path[4096];
  int n = 0, bad = 0, decoded = 0;
  while (fscanf(f, "%4095s", path) == 1) {
    FILE* g = fopen(path, "rb");
    if (!g) return 2;
    std::vector<uint8_t> own;  // the exact file bytes in a heap block of their own: a read past either end is seen
    int c;
    while ((c = fgetc(g)) != EOF) own.push_back((uint8_t)c);
    fclose(g);
    own.shrink_to_fit();
    if (own.empty()) own.reserve(1);
    int64_t zero = 0, size = (int64_t)own.size(), total = 0, nd = 0, ws = 0;
    vge_webp_info info, info2;
    const char* p = path;
    vge_webp_probe(&p, 1, 1, &info);
    vge_webp_probe_mem(own.data(), size, &zero, &size, 1, 1, &info2);
    if (memcmp(&info, &info2, sizeof(info)) != 0 && size > 0) ++bad;
    ++n;
    uint64_t feat[4];
    vge_debug_webp_features(own.data(), size, feat);
    const int w = info2.width, h = info2.height;
    if (w < 1 || h < 1 || w > 512 || h > 512) continue;
    const int64_t cap = info2.n_frames;
    std::vector<uint8_t> rgb((size_t)(cap + 1) * w * h * 3), rgb2(rgb.size());
    std::vector<int32_t> st((size_t)cap + 1, -1), st2((size_t)cap + 1, -1);
    int32_t fst = -1, fst2 = -1, pst = -1;
    vge_webp_decode(&p, 1, 2, w, h, cap, rgb.data(), st.data(), &fst, &total);
    vge_webp_decode_mem(own.data(), size, &zero, &size, 1, 2, w, h, cap, rgb2.data(), st2.data(), &fst2, &total);
    if (total != cap || (fst != fst2 && size > 0)) ++bad;
    for (int64_t k = 0; k < cap; ++k) {
      if (st[k] != st2[k] || (st[k] == 0 && memcmp(&rgb[k * w * h * 3], &rgb2[k * w * h * 3], (size_t)w * h * 3) != 0))
        ++bad;
      decoded += st[k] == 0;
    }
    std::vector<vge_webp_desc> descs((size_t)cap + 1);
    std::vector<int32_t> plan((size_t)cap + 1, -1);
    vge_webp_plan_mem(own.data(), size, &zero, &size, 1, 1, w, h, descs.data(), cap, &nd, plan.data(), &pst, &ws);
    if (nd != cap || vge_webp_decode_device_workspace_bytes(descs.data(), (int)nd) != (size_t)ws) ++bad;
    for (int64_t k = 0; k < nd; ++k)
      if (descs[k].plan_status == 0 && (descs[k].pay_off + descs[k].pay_bytes > size || st2[k] == 1)) ++bad;
  }
  fclose(f);
  printf("%d files, %d mismatches, %d frames decoded\n", n, bad, decoded);
  return bad ? 1 : 0;
}
"""


def test_host_parser_and_decoder_under_sanitizers(tmp_path):
    """A stand-alone program (its own main, nothing loaded into python) links vge_webp.cpp built with
    -fsanitize=address,undefined and runs the probe, the decoder, the coverage export and the plan over every case file
    and over the seeded mutations, from the path and from an exactly-sized heap copy."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    (tmp_path / "main.cpp").write_text(SANITIZED_MAIN)
    lines = []
    for c in WC.cases():
        p = tmp_path / f"{c.name}.webp"
        p.write_bytes(c.data)
        lines.append(str(p))
    for name, blob in WC.mutations(300):
        p = tmp_path / f"{name}.webp"
        p.write_bytes(blob)
        lines.append(str(p))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    exe = tmp_path / "webp_asan"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", str(REPO), str(tmp_path / "main.cpp"),
                            str(REPO / "video-gen-evals_amd" / "csrc" / "vge_webp.cpp"), "-o", str(exe), "-lpthread"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe), str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert f"{len(lines)} files, 0 mismatches" in run.stdout
