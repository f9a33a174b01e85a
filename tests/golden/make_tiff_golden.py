"""Writes tests/golden/tiff_golden.npz: TIFF files written by Pillow's libtiff -- an encoder that shares nothing with the
writer of tests/tiff_cases.py -- and the arrays Pillow reads back from them.

Needs Pillow built with libtiff; the tests need neither Pillow nor this script.

    python tests/golden/make_tiff_golden.py

Per case i the file holds tif_<i> (the file's bytes) and img_<i> (what Pillow reads back: uint8 / uint16 [H, W] or uint8
[H, W, 3 or 4]), and the label array name.  Modes L, I;16, RGB, RGBA; no compression, PackBits, LZW, Deflate; LZW also with
predictor 2 and four rows per strip (tiffinfo={317: 2, 278: 4})."""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tiff_cases  # noqa: E402

MODES = {"L": (1, 8), "I;16": (1, 16), "RGB": (3, 8), "RGBA": (4, 8)}
COMPRESSIONS = [None, "packbits", "tiff_lzw", "tiff_adobe_deflate"]


def save(img, mode, **kw):
    buf = io.BytesIO()
    im = Image.fromarray(img)
    assert im.mode == mode, (im.mode, mode)
    im.save(buf, "TIFF", **kw)
    return buf.getvalue()


def main():
    cases = []
    k = 0
    for mode, (samples, bits) in MODES.items():
        for comp in COMPRESSIONS:
            w, h = [(23, 19), (31, 9), (16, 33), (37, 11)][k % 4]
            img = tiff_cases.random_image(w, h, samples, bits, seed=40 + k)
            cases.append((f"{mode}_{comp or 'none'}_{w}x{h}", save(img, mode, compression=comp)))
            k += 1
        img = tiff_cases.random_image(33, 21, samples, bits, seed=80 + k)
        cases.append((f"{mode}_lzw_predictor2_rps4_33x21", save(img, mode, compression="tiff_lzw", tiffinfo={317: 2, 278: 4})))
    # every code width and a ClearCode in mid-stream, from libtiff's encoder
    cases.append(("L_lzw_noise_67x131", save(tiff_cases.noise(), "L", compression="tiff_lzw")))
    out = {"name": np.array([c[0] for c in cases])}
    for i, (name, data) in enumerate(cases):
        back = np.asarray(Image.open(io.BytesIO(data)))
        out[f"tif_{i}"] = np.frombuffer(data, np.uint8)
        out[f"img_{i}"] = back.astype(np.uint16) if back.dtype.itemsize == 2 else back
    path = os.path.join(ROOT, "tests", "golden", "tiff_golden.npz")
    np.savez_compressed(path, **out)
    print(len(cases), "cases,", os.path.getsize(path), "bytes ->", path)


if __name__ == "__main__":
    main()
