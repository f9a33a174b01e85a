"""Writes tests/golden/jpeg_rst_golden.npz: baseline JPEG files WITH restart intervals (and one without) at the smallest
shapes where a decoder that takes the intervals apart can go wrong, and the luma plane libjpeg's default decoder gives.

Needs Pillow (restart_marker_blocks / restart_marker_rows); the tests need neither Pillow nor this script.

    python tests/golden/make_jpeg_rst_golden.py

Same schema as jpeg_golden.npz (make_jpeg_golden.py): per case i jpg_<i>, luma_<i> (empty for the 640x480 board), and the
label arrays name / readable / width / height / blocks_w / blocks_h.  The name ends in _dri<N>: the MCUs per restart interval the file's DRI segment
states (0: none).
"""
import io
import os
import struct
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_jpeg_golden import MCU, SUBSAMPLING, blocks, content, luma  # noqa: E402


def encode(img, sampling, quality, **kw):
    buf = io.BytesIO()
    if sampling != "grey":
        kw["subsampling"] = SUBSAMPLING[sampling]
    Image.fromarray(img).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def dri_of(data):
    at = data.find(b"\xff\xdd")
    return struct.unpack(">H", data[at + 4:at + 6])[0] if at >= 0 else 0


def entropy_of(data):
    sos = data.index(b"\xff\xda")
    return data[sos + 2 + struct.unpack(">H", data[sos + 2:sos + 4])[0]:-2]


def main():
    cases = []

    def add(label, w, h, sampling, quality, kind="noise", seed=0, **kw):
        colour = sampling != "grey"
        data = encode(content(kind, w, h, colour, seed), sampling, quality, **kw)
        plane = luma(data)
        bw, bh = blocks(w, h, sampling)
        name = f"{label}_{w}x{h}_{sampling}_q{quality}_dri{dri_of(data)}"
        cases.append((name, data, plane, bw, bh))
        return data

    add("noise", 8, 8, "grey", 75, seed=1, restart_marker_blocks=1)            # one MCU, one interval, no RST marker at all
    add("noise", 17, 9, "444", 75, seed=2, restart_marker_blocks=1)
    add("noise", 31, 33, "420", 75, seed=3, restart_marker_blocks=4)           # 2 x 3 MCUs: intervals cross MCU rows
    add("noise", 31, 33, "422", 75, seed=4, restart_marker_blocks=1)           # block order inside an MCU
    add("noise", 31, 33, "grey", 75, seed=5, restart_marker_blocks=1)
    add("noise", 53, 37, "420", 75, seed=6, restart_marker_blocks=5)           # 12 MCUs: a short last interval
    d = add("noise", 48, 64, "grey", 75, seed=7, restart_marker_blocks=1)      # 48 intervals: RST numbers wrap six times
    assert d.count(b"\xff\xd7") >= 5
    add("noise", 136, 136, "grey", 75, seed=8, restart_marker_blocks=1)        # 289 intervals: two workgroups, the second partly filled
    add("noise", 264, 16, "420", 75, seed=9, restart_marker_blocks=7)          # 17 MCUs -> 7, 7, 3; 34 stored blocks per row
    d = add("noise", 48, 64, "444", 100, seed=10, restart_marker_blocks=2)     # codes longer than 9 bits, size-10 values
    assert b"\xff\x00" in entropy_of(d)
    add("noise", 48, 64, "420", 30, seed=11, restart_marker_blocks=3)          # ZRL / long runs
    add("black", 48, 64, "grey", 75, kind="black", restart_marker_blocks=1)            # the shortest intervals: three bytes each
    add("optimize", 48, 64, "420", 75, seed=12, restart_marker_blocks=2, optimize=True)   # non-standard tables
    add("rows", 48, 64, "420", 75, seed=13, restart_marker_rows=1)
    d = add("nodri", 48, 64, "420", 75, seed=14)                               # must route to the host
    assert dri_of(d) == 0
    # a frame the detector finds a board in, one interval per MCU row
    from mrgingham_amd import synth
    board = synth.board_frame(640, 480).numpy()
    data = encode(board, "grey", 90, restart_marker_rows=1)
    # (its plane is not stored, to keep the file small: the tests compare the detector's result, and the host decoder is
    # pinned on every other file)
    assert luma(data).shape == (480, 640)
    cases.append((f"board_640x480_grey_q90_dri{dri_of(data)}", data, None, 80, 60))
    assert MCU["grey"] == (1, 1) and dri_of(data) == 80

    out = {"name": np.array([c[0] for c in cases]), "readable": np.array([True] * len(cases)),
           "width": np.array([c[2].shape[1] if c[2] is not None else 640 for c in cases], np.int32),
           "height": np.array([c[2].shape[0] if c[2] is not None else 480 for c in cases], np.int32),
           "blocks_w": np.array([c[3] for c in cases], np.int32), "blocks_h": np.array([c[4] for c in cases], np.int32)}
    for i, c in enumerate(cases):
        out[f"jpg_{i}"] = np.frombuffer(c[1], np.uint8)
        out[f"luma_{i}"] = c[2] if c[2] is not None else np.zeros((0, 0), np.uint8)
    path = os.path.join(HERE, "jpeg_rst_golden.npz")
    np.savez_compressed(path, **out)
    print(len(cases), "cases,", os.path.getsize(path), "bytes ->", path)
    for c in cases:
        print(" ", c[0], len(c[1]))


if __name__ == "__main__":
    main()
