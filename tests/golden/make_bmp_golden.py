"""Writes tests/golden/bmp_golden.npz: Windows Bitmap files written by Pillow -- an encoder that shares nothing with the
writer of tests/bmp_cases.py -- and the arrays they were written from.

Needs Pillow; the tests need neither Pillow nor this script.

    python tests/golden/make_bmp_golden.py

Per case i the file holds bmp_<i> (the file's bytes) and img_<i> (the image as R G B samples, uint8 [H, W, 3]: a mode 1 or L
pixel three times, a mode P pixel's palette entry, the first three of an RGBA pixel), and the label array name.  Modes 1, L,
P, RGB and RGBA at 13x5 and 37x9."""
import io
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = [(13, 5), (37, 9)]


def image(mode, w, h, seed):
    rng = np.random.default_rng(seed)
    if mode == "1":
        return Image.fromarray(rng.integers(0, 2, (h, w)).astype(bool))
    if mode == "L":
        return Image.fromarray(rng.integers(0, 256, (h, w)).astype(np.uint8))
    if mode == "P":
        im = Image.fromarray(rng.integers(0, 256, (h, w)).astype(np.uint8), "P")
        im.putpalette(rng.integers(0, 256, 768).astype(np.uint8).tobytes())
        return im
    return Image.fromarray(rng.integers(0, 256, (h, w, len(mode))).astype(np.uint8), mode)


def main():
    out, names = {}, []
    for k, (mode, (w, h)) in enumerate((m, s) for m in ("1", "L", "P", "RGB", "RGBA") for s in SIZES):
        im = image(mode, w, h, 60 + k)
        buf = io.BytesIO()
        im.save(buf, "BMP")
        names.append(f"{mode}_{w}x{h}")
        out[f"bmp_{k}"] = np.frombuffer(buf.getvalue(), np.uint8)
        out[f"img_{k}"] = np.asarray(im.convert("RGB"))
    out["name"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "bmp_golden.npz")
    np.savez_compressed(path, **out)
    print(len(names), "cases,", os.path.getsize(path), "bytes ->", path)


if __name__ == "__main__":
    main()
