"""Writes tests/golden/pnm_golden.npz: binary PBM files written by Pillow -- an encoder that shares nothing with the
writer of tests/pnm_cases.py -- and the arrays they were written from.

Needs Pillow; the tests need neither Pillow nor this script.

    python tests/golden/make_pnm_golden.py

Per case i the file holds pnm_<i> (the file's bytes) and img_<i> (the image as R G B samples, uint8 [H, W, 3]: a mode 1
pixel three times, 0 or 255), and the label array name.  Mode 1 (P4) at 1x1, 8x3, 13x5 and 37x9 (Pillow writes no PAM,
and P6 is not read)."""
import io
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = [(1, 1), (8, 3), (13, 5), (37, 9)]


def image(mode, w, h, seed):
    rng = np.random.default_rng(seed)
    return Image.fromarray(rng.integers(0, 2, (h, w)).astype(bool))


def main():
    out, names = {}, []
    for k, (mode, (w, h)) in enumerate((m, s) for m in ("1",) for s in SIZES):
        im = image(mode, w, h, 80 + k)
        buf = io.BytesIO()
        im.save(buf, "PPM")
        assert buf.getvalue()[:2] == b"P4"
        names.append(f"{mode}_{w}x{h}")
        out[f"pnm_{k}"] = np.frombuffer(buf.getvalue(), np.uint8)
        out[f"img_{k}"] = np.asarray(im.convert("RGB"))
    out["name"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "pnm_golden.npz")
    np.savez_compressed(path, **out)
    print(len(names), "cases,", os.path.getsize(path), "bytes ->", path)


if __name__ == "__main__":
    main()
