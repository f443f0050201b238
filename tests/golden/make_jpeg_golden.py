"""Writes tests/golden/jpeg_golden.npz: JPEG byte strings and the arrays Pillow (libjpeg-turbo: the islow IDCT and
fancy upsampling that cv2.imread uses too) decodes from them.  Run from the repository root:

    python -m tests.golden.make_jpeg_golden

Keys: jpeg/<name> uint8 bytes, rgb/<name> uint8 [H, W, 3] (Pillow's decode, grayscale converted to RGB; none for tree_* and
tile_*: decoded JPEG noise does not compress, and the file stays small);
bad/<name> bytes only (error-path files); names are listed in `names`, `batch_names`, `tree_names`, `tile_names`.
Images: ten sizes (width or height no multiple of the MCU, odd chroma planes, one-sample planes) x 4:2:0, 4:2:2, 4:4:4,
grayscale, 4:2:0 with restart markers, 4:2:0 with optimised Huffman tables x {a smooth image at quality 95, uniform
noise at quality 60}; five 64x48 frames for the batched path; 2 videos x 6 frames of vge.synth.make_frames (128x128,
quality 95, 4:2:0: what cv2.imwrite writes) for the extraction-tree test; 260x140 and 150x131 images in the four
samplings (several tiles of the device kernel); a progressive file and a truncated file.
"""
import io
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(REPO / "video-gen-evals_amd"))

# (width, height); the last four: chroma planes of one and two columns, which libjpeg replicates instead of
# interpolating (its fancy upsamplers need a downsampled width > 2), and the first widths past that
SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (19, 21), (37, 53), (2, 37), (3, 5), (4, 9), (5, 6)]
ENCODINGS = {
    "420": dict(subsampling=2),
    "422": dict(subsampling=1),
    "444": dict(subsampling=0),
    "gray": dict(),
    "420rst": dict(subsampling=2, restart_marker_blocks=2),
    "420opt": dict(subsampling=2, optimize=True),
}


def smooth_image(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 6.28, size=(3, 2))
    img = np.stack([127.5 + 110 * np.sin(x / 5.0 + ph[c, 0]) * np.cos(y / 7.0 + ph[c, 1]) for c in range(3)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


def noise_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def encode(img, quality, mode="RGB", **kw):
    from PIL import Image
    im = Image.fromarray(img)
    if mode == "L":
        im = im.convert("L")
    buf = io.BytesIO()
    im.save(buf, format="JPEG", quality=quality, **kw)
    return buf.getvalue()


def decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    from vge import synth
    out, names, batch, tree, tiles = {}, [], [], [], []

    def add(name, data, lst):
        out[f"jpeg/{name}"] = np.frombuffer(data, np.uint8)
        if lst is not tree and lst is not tiles:   # those are compared with the host path on the same bytes
            out[f"rgb/{name}"] = decode(data)
        lst.append(name)

    seed = 100
    for (w, h) in SIZES:
        for enc, kw in ENCODINGS.items():
            for kind, quality, gen in (("smooth", 95, smooth_image), ("noise", 60, noise_image)):
                seed += 1
                add(f"{w}x{h}_{enc}_{kind}", encode(gen(w, h, seed), quality, "L" if enc == "gray" else "RGB", **kw),
                    names)
    for i in range(5):
        img = smooth_image(64, 48, 900 + i) // 2 + noise_image(64, 48, 950 + i) // 2
        add(f"batch_{i}", encode(img, 95, subsampling=2), batch)
    for v in range(2):
        fr = synth.make_frames(40 + v, 6, h=128, w=128)
        for f in range(6):
            add(f"tree_v{v}_f{f}", encode(fr[f], 95, subsampling=2), tree)
    # several 128 x 64 kernel tiles in both directions, frame edges inside a tile: dword-store and byte-store widths
    for (w, h) in ((260, 140), (150, 131)):
        for enc in ("420", "422", "444", "gray"):
            coarse = np.kron(noise_image(w // 8 + 2, h // 8 + 2, 301 + w), np.ones((8, 8, 1), np.uint8))[3:h + 3, 5:w + 5]
            img = (smooth_image(w, h, 300 + w).astype(np.int32) * 3 // 4 + coarse // 4).astype(np.uint8)
            add(f"tile_{w}x{h}_{enc}", encode(img, 75, "L" if enc == "gray" else "RGB", **ENCODINGS[enc]), tiles)
    img = smooth_image(37, 53, 7)
    out["bad/progressive"] = np.frombuffer(encode(img, 90, progressive=True), np.uint8)
    good = encode(smooth_image(64, 48, 8) // 2 + noise_image(64, 48, 9) // 2, 95, subsampling=2)
    out["bad/truncated"] = np.frombuffer(good[:len(good) // 2], np.uint8)
    out["names"] = np.array(names)
    out["batch_names"] = np.array(batch)
    out["tree_names"] = np.array(tree)
    out["tile_names"] = np.array(tiles)
    import PIL
    out["pillow_version"] = np.array(PIL.__version__)
    dst = Path(__file__).resolve().parent / "jpeg_golden.npz"
    np.savez_compressed(dst, **out)
    print(f"{dst}: {dst.stat().st_size} bytes, {len(names)} + {len(batch)} + {len(tree)} + {len(tiles)} images")


if __name__ == "__main__":
    main()
