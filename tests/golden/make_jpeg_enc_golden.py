"""Writes tests/golden/jpeg_enc_golden.npz: source images, the JPEG files Pillow (libjpeg-turbo: the encoder
cv2.imwrite uses too) writes from them, and what Pillow decodes from those files.  Run from the repository root:

    python -m tests.golden.make_jpeg_enc_golden

Keys
  src/<image>        uint8 [H, W, 3] RGB source
  jpeg/<case>        uint8 bytes of Image.save(quality=q, subsampling=s); <case> is <image>_<420|422|444>_q<quality>
  rgb/<case>         uint8 [H, W, 3]: Pillow's decode of those bytes (none for the tile_* cases: the host reconstruct is
                     already pinned to Pillow's decoder by jpeg_golden.npz, and their files and coefficients are compared)
  names, batch_names, tile_names   the cases (the image of a case: its name without the last two fields)
  qtables            uint8 [100, 2, 64]: the luminance and chrominance tables of Pillow's files for quality 1..100, natural
                     order, read out of the files' DQT segments

Images, as width x height: the basic block and MCU (1x1, 8x8, 16x16); odd sizes (17x33, 37x53); an even height that is
no multiple of 16, where libjpeg's vertical edge rule shows (5x6, 16x12, 32x44); right-hand dummy luma blocks (8x14); a
whole dummy luma row (16x6); narrow planes (2x37, 3x5) -- each as uniform noise and as a smooth image, in the three
samplings at quality 95, and 17x33 / 32x44 noise also at 30, 75 and 100; five 64x48 frames for the batched path; 260x140
and 150x131 (several 128 x 64 kernel tiles, dword and byte paths) as a smooth image mixed with blocky noise, which stays
small in the archive.
"""
import io
from pathlib import Path

import numpy as np

from tests.golden.make_jpeg_golden import noise_image, smooth_image

SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (37, 53), (5, 6), (16, 12), (32, 44), (8, 14), (16, 6), (2, 37), (3, 5)]
SUBSAMPLING = {"420": 2, "422": 1, "444": 0}
EXTRA_QUALITY_SIZES = [(17, 33), (32, 44)]
TILE_SIZES = [(260, 140), (150, 131)]
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
          61, 54, 47, 55, 62, 63]


def encode(img, quality, sub):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=quality, subsampling=SUBSAMPLING[sub])
    return buf.getvalue()


def decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def dqt_tables(data):
    """{table id: uint8 [64] natural order} from a file's DQT segments."""
    out, i = {}, 2
    while data[i + 1] != 0xDA:
        n = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xDB:
            seg = data[i + 4:i + 2 + n]
            for o in range(0, len(seg), 65):
                assert seg[o] >> 4 == 0
                t = np.zeros(64, np.uint8)
                t[ZIGZAG] = np.frombuffer(seg[o + 1:o + 65], np.uint8)
                out[seg[o] & 15] = t
        i += 2 + n
    return out


def main():
    out, names, batch, tiles = {}, [], [], []

    def add(image, img, quality, sub, lst, with_decode=True):
        out[f"src/{image}"] = img
        case = f"{image}_{sub}_q{quality}"
        data = encode(img, quality, sub)
        out[f"jpeg/{case}"] = np.frombuffer(data, np.uint8)
        if with_decode:
            out[f"rgb/{case}"] = decode(data)
        lst.append(case)

    seed = 500
    for (w, h) in SIZES:
        for kind, gen in (("noise", noise_image), ("smooth", smooth_image)):
            seed += 1
            img = gen(w, h, seed)
            for sub in SUBSAMPLING:
                add(f"{w}x{h}_{kind}", img, 95, sub, names)
                if kind == "noise" and (w, h) in EXTRA_QUALITY_SIZES:
                    for q in (30, 75, 100):
                        add(f"{w}x{h}_{kind}", img, q, sub, names)
    for i in range(5):
        img = smooth_image(64, 48, 1900 + i) // 2 + noise_image(64, 48, 1950 + i) // 2
        add(f"batch{i}", img, 95, "420", batch)
    for (w, h) in TILE_SIZES:
        coarse = np.kron(noise_image(w // 8 + 2, h // 8 + 2, 701 + w), np.ones((8, 8, 1), np.uint8))[3:h + 3, 5:w + 5]
        img = (smooth_image(w, h, 700 + w).astype(np.int32) * 3 // 4 + coarse // 4).astype(np.uint8)
        for sub in SUBSAMPLING:
            add(f"tile{w}x{h}", img, 95, sub, tiles, with_decode=False)
    qt = np.zeros((100, 2, 64), np.uint8)
    for q in range(1, 101):
        t = dqt_tables(encode(np.zeros((8, 8, 3), np.uint8), q, "420"))
        qt[q - 1, 0], qt[q - 1, 1] = t[0], t[1]
    out["qtables"] = qt
    out["names"] = np.array(names)
    out["batch_names"] = np.array(batch)
    out["tile_names"] = np.array(tiles)
    import PIL
    out["pillow_version"] = np.array(PIL.__version__)
    dst = Path(__file__).resolve().parent / "jpeg_enc_golden.npz"
    np.savez_compressed(dst, **out)
    print(f"{dst}: {dst.stat().st_size} bytes, {len(names)} + {len(batch)} + {len(tiles)} cases")


if __name__ == "__main__":
    main()
