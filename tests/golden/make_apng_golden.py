"""Writes tests/golden/apng_golden.npz: what Pillow decodes from every file of tests/apng_cases.py, and a handful of
animated PNGs as Pillow writes them with the frames Pillow decodes from them, so that the tests of the APNG decoder
need no Pillow.  Needs neither a GPU nor the network.

    python tests/golden/make_apng_golden.py

Keys: n/<case> (the frames PIL.ImageSequence yields before it stops or raises), rgb/<case> (uint8 [n, H, W, 3]: those
frames after .convert("RGB"); absent when n is 0), apng/<name> (a Pillow-written file, uint8), rgb/<name> (its frames),
pillow_version.  The maker also confirms, point by point, the composition rule that include/vge_apng.h states: the
model of tests/apng_cases.py must give Pillow's pixels for every frame that stands, and Pillow must yield exactly the
frames that stand for every case inside the equality."""
import io
import sys
import warnings
from pathlib import Path

import numpy as np
import PIL
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from tests import apng_cases as AC  # noqa: E402


def pillow_frames(data: bytes):
    """The frames Pillow yields, seeking as PIL.ImageSequence.Iterator does, until it stops or raises."""
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            im = Image.open(io.BytesIO(data))
            k = 0
            while True:
                try:
                    im.seek(k)
                except EOFError:
                    break
                out.append(np.asarray(im.convert("RGB")).copy())
                k += 1
        except Exception:   # the frame that raises, and every later one, is not yielded
            pass
    return out


def clip(seed, n, h, w, alpha):
    """A moving square over a fixed banded background: frames differ only in a corner, so Pillow writes deltas."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x // 6 * 24) % 256, (y // 5 * 20) % 256, ((x + y) // 8 * 16) % 256, (x * 5 + y * 3) % 256], -1)
    out = []
    for f in range(n):
        a = base.astype(np.uint8).copy()
        a[4 + 2 * f:14 + 2 * f, 6 + 3 * f:18 + 3 * f] = rng.integers(0, 256, 4, dtype=np.uint8)
        out.append(a if alpha else a[..., :3].copy())
    return out


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for c in AC.cases():
        frames = pillow_frames(c.data)
        stand = c.n_frames if c.accept else c.bad_frame
        if c.pillow:
            assert len(frames) == stand, (c.name, len(frames), stand)
        for k in range(min(stand, len(frames)) if c.want is not None else 0):
            assert np.array_equal(frames[k], c.want[k]), (c.name, k)
        out[f"n/{c.name}"] = np.array(len(frames))
        if frames and c.expect != AC.ERR_SHAPE:
            out[f"rgb/{c.name}"] = np.stack(frames)
        print(f"{c.name}: Pillow yields {len(frames)}, {stand} stand here")
    specs = [("rgb_deltas", False, {}), ("rgba_deltas", True, {}),
             ("rgba_background_over", True, dict(disposal=1, blend=1)),
             ("rgba_previous_over", True, dict(disposal=2, blend=1)),
             ("rgb_mixed", False, dict(disposal=[0, 1, 2, 0, 1, 2], blend=[0, 1, 0, 1, 0, 1])),
             ("rgba_mixed", True, dict(disposal=[2, 1, 0, 2, 1, 0], blend=[1, 1, 0, 1, 0, 1]))]
    for name, alpha, kw in specs:
        ims = [Image.fromarray(a, "RGBA" if alpha else "RGB") for a in clip(3, 6, 48, 64, alpha)]
        buf = io.BytesIO()
        ims[0].save(buf, "PNG", save_all=True, append_images=ims[1:], duration=40, loop=0, **kw)
        data = buf.getvalue()
        frames = pillow_frames(data)
        assert len(frames) == 6, name
        out[f"apng/{name}"] = np.frombuffer(data, np.uint8)
        out[f"rgb/{name}"] = np.stack(frames)
    path = Path(__file__).resolve().parent / "apng_golden.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
