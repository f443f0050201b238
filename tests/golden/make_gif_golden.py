"""Writes tests/golden/gif_golden.npz: a handful of animated GIFs as Pillow writes them, with the frames Pillow decodes
from them and the Pillow version, so that the GPU test of the GIF decoder needs no Pillow.

    python tests/golden/make_gif_golden.py

Keys: gif/<name> (the file, uint8), rgb/<name> (uint8 [F, H, W, 3]: every ImageSequence frame after .convert("RGB")),
pillow_version."""
import io
from pathlib import Path

import numpy as np
import PIL
from PIL import Image, ImageSequence


def clip(seed, n, h, w):
    """A moving square over a slowly changing banded background: parts of a frame repeat the one before."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for f in range(n):
        base = np.stack([(x // 6 * 24 + f) % 256, (y // 5 * 20) % 256, ((x + y) // 8 * 16) % 256], -1).astype(np.uint8)
        base[5 + 2 * f:17 + 2 * f, 8 + 3 * f:22 + 3 * f] = rng.integers(0, 256, 3, dtype=np.uint8)
        out.append(base)
    return out


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    rgb = [Image.fromarray(a, "RGB") for a in clip(1, 6, 48, 64)]
    pal = [im.quantize(32) for im in rgb]
    specs = [("rgb_plain", rgb, dict(optimize=False)),        # RGB frames: a local table per frame
             ("rgb_optimize", rgb, dict(optimize=True)),      # transparent "unchanged" pixels, cropped rectangles
             ("p_plain", pal, dict(optimize=False)),
             ("p_dispose2", pal, dict(optimize=True, disposal=2)),
             ("p_interlaced", pal[:1], dict(interlace=True))]   # Pillow interlaces single images only
    for name, frames, kw in specs:
        buf = io.BytesIO()
        if len(frames) == 1:
            frames[0].save(buf, "GIF", **kw)
        else:
            frames[0].save(buf, "GIF", save_all=True, append_images=frames[1:], duration=40, loop=0, **kw)
        data = buf.getvalue()
        out[f"gif/{name}"] = np.frombuffer(data, np.uint8)
        out[f"rgb/{name}"] = np.stack([np.asarray(f.convert("RGB")) for f in
                                       ImageSequence.Iterator(Image.open(io.BytesIO(data)))])
    path = Path(__file__).resolve().parent / "gif_golden.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
