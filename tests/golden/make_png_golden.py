"""Writes tests/golden/png_golden.npz: a handful of PNG files as Pillow writes them, with the pixels Pillow decodes
from them and the Pillow version, so that the GPU test of the PNG decoder needs no Pillow.

    python tests/golden/make_png_golden.py

Keys: png/<name> (the file, uint8), rgb/<name> (uint8 [H, W, 3]: Image.open(file).convert("RGB")), pillow_version."""
import io
from pathlib import Path

import numpy as np
import PIL
from PIL import Image


def frame(seed, h, w, c):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(2 * x + y) % 256, (x + 3 * y) % 256, (x * y // 5) % 256, (200 + x - y) % 256], -1)[..., :c]
    return ((base + rng.integers(0, 8, (h, w, c))) % 256).astype(np.uint8)


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    specs = [("rgb_l1", "RGB", 3, 96, 80, dict(compress_level=1)), ("rgb_l6", "RGB", 3, 96, 80, dict(compress_level=6)),
             ("rgb_l9", "RGB", 3, 96, 80, dict(compress_level=9)), ("rgb_opt", "RGB", 3, 130, 67, dict(optimize=True)),
             ("rgba_l6", "RGBA", 4, 70, 90, dict(compress_level=6)), ("grey_l6", "L", 1, 75, 131, dict(compress_level=6))]
    for i, (name, mode, c, h, w, kw) in enumerate(specs):
        px = frame(40 + i, h, w, c)
        buf = io.BytesIO()
        Image.fromarray(px[..., 0] if c == 1 else px, mode).save(buf, "PNG", **kw)
        out[f"png/{name}"] = np.frombuffer(buf.getvalue(), np.uint8)
        out[f"rgb/{name}"] = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    path = Path(__file__).resolve().parent / "png_golden.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
