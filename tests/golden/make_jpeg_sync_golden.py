"""Writes tests/golden/jpeg_sync_golden.npz: baseline JPEG files WITHOUT restart intervals, as cameras and libraries write
them, for the self-synchronising Huffman decoder (csrc/jpeg_huff_sync.h), and the luma plane libjpeg's default decoder
gives.

Needs Pillow and the built library (it asserts what the decoder needs of the files); the tests need neither Pillow nor
this script.

    python tests/golden/make_jpeg_sync_golden.py

Same schema as jpeg_golden.npz (make_jpeg_golden.py): per case i jpg_<i>, luma_<i> (empty where LUMA_STORED says so, to
keep the file small: those files are compared with the host decoder, which every other file pins), and the label arrays
name / readable / width / height / blocks_w / blocks_h.  Names are <label>_<width>x<height>_<sampling>_q<quality>.

  realistic   320 x 240: synth.board_frame blended with blurred colour noise (what a lens and a sensor leave of a
              board), in the samplings and qualities below, and the plain board in 4:2:0.  Every one of them has to
              synchronise within half the default cap at 32-byte subsequences: rounds * 32 <= 4096.
  large       640 x 480, 4:2:0, quality 90: several thousand subsequences at 8 bytes, i.e. many workgroups.
  noise       48 wide, 64 high (the size of the small fixtures of the other two files, so that one loader call can mix
              them), grey, quality 100: no end-of-block symbols, many stuffed FF 00, and it hardly synchronises: the
              rounds it needs grow with its length (more than half its subsequences).  At 5 KB it still fits under the
              default cap of 8 KB; the tests lower the cap to send it the late way.

The measured rounds are printed; DESIGN.md section 4.10 quotes them.
"""
import io
import os
import sys

import numpy as np
from PIL import Image, ImageFilter

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_jpeg_golden import SUBSAMPLING, blocks, luma  # noqa: E402
from make_jpeg_rst_golden import dri_of, entropy_of  # noqa: E402

LUMA_STORED = ("blend_320x240_grey_q90", "noise")    # substrings of the names whose plane is kept


def encode(img, sampling, quality, **kw):
    buf = io.BytesIO()
    if sampling == "grey":
        img = img if img.ndim == 2 else np.asarray(Image.fromarray(img).convert("L"))
    else:
        kw["subsampling"] = SUBSAMPLING[sampling]
        img = img if img.ndim == 3 else np.stack([img] * 3, axis=-1)
    Image.fromarray(img).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def textured(w, h, seed):
    """The board under blurred colour noise: uint8 [h, w, 3]."""
    from mrgingham_amd import synth
    board = synth.board_frame(w, h).numpy().astype(np.float32)
    rng = np.random.RandomState(seed)
    noise = Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).filter(ImageFilter.GaussianBlur(2.0))
    noise = (np.asarray(noise).astype(np.float32) - 128.0) * 3.0 + 128.0
    return np.clip(0.7 * board[:, :, None] + 0.3 * noise, 0, 255).astype(np.uint8)


def main():
    import mrgingham_amd
    from mrgingham_amd import synth
    cases = []

    def add(label, img, sampling, quality, realistic=True, **kw):
        data = encode(img, sampling, quality, **kw)
        assert dri_of(data) == 0
        plane = luma(data)
        h, w = plane.shape
        name = f"{label}_{w}x{h}_{sampling}_q{quality}"
        rounds = {S: mrgingham_amd.jpeg_sync_rounds(data, S) for S in (8, 32, 64, 128)}
        print(f"  {name:40s} {len(data):6d} bytes  rounds (of subsequences) at S = 8 / 32 / 64 / 128: "
              + " / ".join(f"{r} ({n})" for r, n in rounds.values()))
        if realistic:
            assert rounds[32][0] * 32 <= 4096, (name, rounds)       # a margin of two under the default cap
        bw, bh = blocks(w, h, sampling)
        cases.append((name, data, plane if any(s in name for s in LUMA_STORED) else None, bw, bh, w, h))
        return data

    blend = textured(320, 240, 1)
    add("blend", blend, "grey", 90)
    add("blendopt", blend, "grey", 90, optimize=True)
    add("blend", blend, "444", 95)
    add("blend", blend, "422", 75)
    add("blend", blend, "420", 90)
    add("blend", blend, "420", 50)
    add("plain", synth.board_frame(320, 240).numpy(), "420", 90)
    d = add("blend", textured(640, 480, 2), "420", 90)
    assert len(entropy_of(d)) // 8 >= 4 * 256, len(d)               # several workgroups' worth of 8-byte subsequences
    noise = np.random.RandomState(3).randint(0, 256, size=(64, 48)).astype(np.uint8)
    d = add("noise", noise, "grey", 100, realistic=False)
    assert entropy_of(d).count(b"\xff\x00") >= 8
    r, n = mrgingham_amd.jpeg_sync_rounds(d, 32)
    assert r > n // 2, (r, n)                                     # rounds in proportion to the file's length

    out = {"name": np.array([c[0] for c in cases]), "readable": np.array([True] * len(cases)),
           "width": np.array([c[5] for c in cases], np.int32), "height": np.array([c[6] for c in cases], np.int32),
           "blocks_w": np.array([c[3] for c in cases], np.int32), "blocks_h": np.array([c[4] for c in cases], np.int32)}
    for i, c in enumerate(cases):
        out[f"jpg_{i}"] = np.frombuffer(c[1], np.uint8)
        out[f"luma_{i}"] = c[2] if c[2] is not None else np.zeros((0, 0), np.uint8)
    path = os.path.join(HERE, "jpeg_sync_golden.npz")
    np.savez_compressed(path, **out)
    print(len(cases), "cases,", os.path.getsize(path), "bytes ->", path)
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
