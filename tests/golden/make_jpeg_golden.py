"""Writes tests/golden/jpeg_golden.npz: baseline JPEG files and the luma plane libjpeg's default decoder gives for each.

Needs Pillow (built on libjpeg-turbo); the tests need neither Pillow nor this script.  What cv::imread(IMREAD_GRAYSCALE)
asks libjpeg for is JCS_GRAYSCALE, i.e. for a grey or YCbCr file the luma plane after the default integer inverse DCT;
`im.draft('L', im.size)` makes Pillow ask for exactly that, so np.asarray(im) is the expected plane, byte for byte.

    python tests/golden/make_jpeg_golden.py

Per case i the file holds jpg_<i> (the file's bytes), luma_<i> (uint8 [H, W]; empty where the file is expected to be
unreadable) and the label arrays name / readable / width / height / blocks_w / blocks_h (luma blocks padded to whole MCUs).
"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SIZES = [(8, 8), (17, 9), (16, 16), (31, 33), (53, 37), (48, 64)]          # (width, height)
SAMPLINGS = ["grey", "444", "422", "420"]
MCU = {"grey": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}         # luma sampling factors (H, V)
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def content(kind, w, h, colour, seed):
    rng = np.random.RandomState(seed)
    shape = (h, w, 3) if colour else (h, w)
    if kind == "noise":
        return rng.randint(0, 256, size=shape).astype(np.uint8)
    if kind == "black":
        return np.zeros(shape, np.uint8)
    if kind == "white":
        return np.full(shape, 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    c = (((xx // 3) + (yy // 5)) & 1).astype(np.uint8) * 255                  # checker
    return np.stack([c, 255 - c, c // 2], axis=-1) if colour else c


def encode(img, sampling, quality, restart_rows, **kw):
    buf = io.BytesIO()
    if sampling != "grey":
        kw["subsampling"] = SUBSAMPLING[sampling]
    if restart_rows:
        kw["restart_marker_rows"] = restart_rows
    if quality is not None:                     # (None: the tables given as qtables are written as they are)
        kw["quality"] = quality
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def luma(data):
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    a = np.asarray(im)
    assert a.dtype == np.uint8 and a.ndim == 2, (a.dtype, a.shape)
    return a


def blocks(w, h, sampling):
    H, V = MCU[sampling]
    return -(-w // (8 * H)) * H, -(-h // (8 * V)) * V


def main():
    cases = []  # (name, bytes, expected plane or None, blocks_w, blocks_h)

    def add(name, data, sampling, readable=True):
        if readable:
            plane = luma(data)
            bw, bh = blocks(plane.shape[1], plane.shape[0], sampling)
            cases.append((name, data, plane, bw, bh))
        else:
            cases.append((name, data, None, 0, 0))

    qualities, restarts = [30, 75, 95, 100], [0, 1, 3]
    for i, (w, h) in enumerate(SIZES):
        for j, sampling in enumerate(SAMPLINGS):
            colour = sampling != "grey"
            k = i + j
            q, r = qualities[k % 4], restarts[k % 3]
            add(f"noise_{w}x{h}_{sampling}_q{q}_r{r}", encode(content("noise", w, h, colour, 100 + k), sampling, q, r), sampling)
            kind = ["checker", "black", "white"][k % 3]
            q, r = qualities[(k + 2) % 4], restarts[(k + 1) % 3]
            add(f"{kind}_{w}x{h}_{sampling}_q{q}_r{r}", encode(content(kind, w, h, colour, 0), sampling, q, r), sampling)
    # planes that cross the seams of the device kernel: 33 and 65 blocks per row
    add("noise_264x16_420_q75_r1", encode(content("noise", 264, 16, True, 7), "420", 75, 1), "420")
    add("noise_520x8_grey_q95_r0", encode(content("noise", 520, 8, False, 8), "grey", 95, 0), "grey")
    # SOF1 instead of SOF0 (extended sequential, same coding)
    base = encode(content("noise", 31, 33, True, 9), "420", 75, 0)
    at = base.index(b"\xff\xc0")
    add("sof1_patched_31x33_420", base[:at] + b"\xff\xc1" + base[at + 2:], "420")
    # a 16-bit quantisation table (written as SOF1)
    add("qtable16_53x37_grey", encode(content("noise", 53, 37, False, 10), "grey", None, 0, qtables=[[300] + [1] * 63]), "grey")
    # not read: progressive, and four components
    add("progressive_48x64_420", encode(content("noise", 48, 64, True, 11), "420", 75, 0, progressive=True), "420", readable=False)
    buf = io.BytesIO()
    Image.fromarray(content("noise", 16, 16, True, 12)).convert("CMYK").save(buf, "JPEG", quality=75)
    add("cmyk_16x16", buf.getvalue(), "444", readable=False)
    # a frame the detector finds a board in
    from mrgingham_amd import synth
    board = synth.board_frame(640, 480).numpy()
    add("board_640x480_grey_q90", encode(board, "grey", 90, 0), "grey")

    out = {"name": np.array([c[0] for c in cases]), "readable": np.array([c[2] is not None for c in cases]),
           "width": np.array([c[2].shape[1] if c[2] is not None else 0 for c in cases], np.int32),
           "height": np.array([c[2].shape[0] if c[2] is not None else 0 for c in cases], np.int32),
           "blocks_w": np.array([c[3] for c in cases], np.int32), "blocks_h": np.array([c[4] for c in cases], np.int32)}
    for i, c in enumerate(cases):
        out[f"jpg_{i}"] = np.frombuffer(c[1], np.uint8)
        out[f"luma_{i}"] = c[2] if c[2] is not None else np.zeros((0, 0), np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz")
    np.savez_compressed(path, **out)
    print(len(cases), "cases,", os.path.getsize(path), "bytes ->", path)


if __name__ == "__main__":
    main()
