"""Writes tests/golden/jpeg_dehuff_golden.npz: the JPEG files the device entropy decoder's tests need beyond
jpeg_golden.npz and jpeg_enc_golden.npz.  Pillow only.  Run from the repository root:

    python -m tests.golden.make_jpeg_dehuff_golden

Keys: jpeg/<name> uint8 file bytes; the names are listed in `names`.  File bytes only: the expected coefficients come
from the host decoder at test time.
  rst1_80x48_420    restart_marker_blocks=1: 15 restart intervals, so the marker index wraps past RST7
  rstrow_64x48_444  restart_marker_rows=1
  rstrow_64x48_gray the same, one component: one block per MCU
  rstopt_64x48_420  optimize=True (the file's own Huffman tables) with restart_marker_blocks=3
  noise_64x64_q100  uniform noise at quality 100: long codes past the 9-bit lookahead
  synth_256x256     one vge.synth.make_frames frame at quality 95, 4:2:0: what cv2.imwrite writes, the workload's kind
"""
import io
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(REPO / "video-gen-evals_amd"))

from tests.golden.make_jpeg_golden import noise_image, smooth_image  # noqa: E402


def encode(img, quality, gray=False, **kw):
    from PIL import Image
    im = Image.fromarray(img)
    if gray:
        im = im.convert("L")
    buf = io.BytesIO()
    im.save(buf, format="JPEG", quality=quality, **kw)
    return np.frombuffer(buf.getvalue(), np.uint8)


def main():
    from vge import synth
    out = {}
    out["jpeg/rst1_80x48_420"] = encode(smooth_image(80, 48, 11), 95, subsampling=2, restart_marker_blocks=1)
    out["jpeg/rstrow_64x48_444"] = encode(smooth_image(64, 48, 12), 95, subsampling=0, restart_marker_rows=1)
    out["jpeg/rstrow_64x48_gray"] = encode(smooth_image(64, 48, 13), 95, gray=True, restart_marker_rows=1)
    out["jpeg/rstopt_64x48_420"] = encode(noise_image(64, 48, 14), 60, subsampling=2, optimize=True,
                                          restart_marker_blocks=3)
    out["jpeg/noise_64x64_q100"] = encode(noise_image(64, 64, 15), 100, subsampling=0)
    out["jpeg/synth_256x256"] = encode(synth.make_frames(1000, 1, h=256, w=256)[0], 95, subsampling=2)
    out["names"] = np.array([k.split("/", 1)[1] for k in out])
    path = REPO / "tests" / "golden" / "jpeg_dehuff_golden.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, {k: int(v.size) for k, v in out.items() if k != "names"})


if __name__ == "__main__":
    main()
