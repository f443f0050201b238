"""Writes tests/golden/webp_golden.npz: lossless WebP files as Pillow writes them and two animations from the suite's own
writer (tests/webp_cases.py), with the frames Pillow decodes from them and the Pillow version, so that the GPU test of
the WebP decoder needs no Pillow.

    python tests/golden/make_webp_golden.py

Keys: webp/<name> (the file, uint8), rgb/<name> (uint8 [F, H, W, 3]: every ImageSequence frame after .convert("RGB")),
pillow_version."""
import io
import sys
from pathlib import Path

import numpy as np
import PIL
from PIL import Image, ImageSequence

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from tests import webp_cases as WC  # noqa: E402


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    rgb = WC._moving(64, 48, 5, 11)
    rgba = WC._moving(64, 48, 4, 12, alpha=True)
    few = [f // 128 * 128 for f in WC._moving(64, 48, 4, 13)]
    by_name = {c.name: c.data for c in WC.cases()}
    files = {"still_default": WC._pillow_bytes(rgb[:1]),
             "still_m6_q100": WC._pillow_bytes(rgb[1:2], method=6, quality=100),
             "still_rgba": WC._pillow_bytes(rgba[1:2]),
             "anim_default": WC._pillow_bytes(rgb),
             "anim_m6_q100": WC._pillow_bytes(rgb, method=6, quality=100),
             "anim_minimize_size": WC._pillow_bytes(rgb, minimize_size=True),
             "anim_rgba": WC._pillow_bytes(rgba),
             "anim_16_colours": WC._pillow_bytes(few),
             "hand_anim": by_name["anim_hand"],
             "hand_alpha_rules": by_name["anim_alpha_rules"]}
    for name, data in files.items():
        out[f"webp/{name}"] = np.frombuffer(data, np.uint8)
        out[f"rgb/{name}"] = np.stack([np.asarray(f.convert("RGB")) for f in
                                       ImageSequence.Iterator(Image.open(io.BytesIO(data)))])
    path = Path(__file__).resolve().parent / "webp_golden.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
