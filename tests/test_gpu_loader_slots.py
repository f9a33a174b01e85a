"""The two chunk slots that the JPEG and the PNG file loaders share (Detector.read_jpegs, Detector.read_pngs): both
loaders called in turn on ONE Detector, every route of them, with chunks of two files so that both slots cycle and then
as single chunks.  A loader must not depend on the size, the event or the staging contents the other one left behind.
The yardsticks are the host decoder (read_image) and, for PNG, the array written into the file; a loader's output is
never compared against a loader's output.  Byte equality (read_image gives the high byte of a 16-bit sample; the source
array pins all sixteen bits)."""
import os

import numpy as np
import pytest

import mrgingham_amd
from test_jpeg_io import case
from tests import png_cases

pytestmark = pytest.mark.gpu

W, H = 48, 64
JPEGS = ["noise_48x64_grey", "checker_48x64_444", "progressive_48x64", "noise_48x64_422", "noise_16x16_444", "noise_48x64_420",
         "white_48x64_420"]                                      # (the seven files of test_gpu_jpeg.py)
JPEG_STATUS = [0, 0, -1, 0, -2, 0, 0]
PNG8_STATUS = [0, 0, 0, 0, -1]
PNG16_STATUS = [0, 0, 0]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """-> {"jpeg" | "png8" | "png16": (paths, statuses, what read_image gives per file, the source array or None)}"""
    d = str(tmp_path_factory.mktemp("loader_slots"))
    jpegs = []
    for i, name in enumerate(JPEGS):
        jpegs.append(os.path.join(d, f"{i}_{name}.jpg"))
        with open(jpegs[-1], "wb") as f:
            f.write(case(name).data)
    png8, src8 = [], []
    for k, ct in enumerate((0, 2, 6)):
        img = png_cases.random_image(W, H, ct, 8, seed=70 + k)
        png8.append(os.path.join(d, f"type{ct}_8.png"))
        png_cases.write(png8[-1], img, ct, 8, filters=("random", k), nidat=1 + k)
        src8.append(png_cases.grey_of(img, ct))
    rng = np.random.default_rng(7)
    png8.append(os.path.join(d, "palette.png"))
    png_cases.write(png8[-1], rng.integers(0, 40, (H, W)).astype(np.uint8), 3, 8, palette=rng.integers(0, 256, (40, 3)).astype(np.uint8))
    src8.append(None)
    png8.append(os.path.join(d, "truncated.png"))
    with open(png8[-1], "wb") as f:
        f.write(open(png8[1], "rb").read()[:-40])
    src8.append(None)
    # 16 bits, grey and RGBA: (48 * 8 + 1) * 64 bytes of scanlines per file, the largest area of all (three files: two chunks)
    png16, src16 = [], []
    for k, ct in enumerate((0, 6, 6)):
        img = png_cases.random_image(W, H, ct, 16, seed=80 + k)
        png16.append(os.path.join(d, f"{k}_type{ct}_16.png"))
        png_cases.write(png16[-1], img, ct, 16, filters="rotate", nidat=2)
        src16.append(png_cases.grey_of(img, ct))
    sets = {"jpeg": (jpegs, JPEG_STATUS, [None] * len(jpegs)), "png8": (png8, PNG8_STATUS, src8), "png16": (png16, PNG16_STATUS, src16)}
    return {k: (paths, status, [mrgingham_amd.read_image(p) for p in paths], src) for k, (paths, status, src) in sets.items()}


def _check(what, files, key, frames, status):
    paths, want_status, host, source = files[key]
    assert status.tolist() == want_status, what
    got = frames.cpu().numpy()
    assert got.shape == (len(paths), H, W) and got.dtype == (np.uint16 if key == "png16" else np.uint8), what
    for f, p in enumerate(paths):
        if want_status[f] != 0:
            assert not got[f].any(), (what, p)
            continue
        high = got[f] if got.dtype == np.uint8 else (got[f] >> 8).astype(np.uint8)    # (read_image: the high byte of 16 bits)
        assert host[f] is not None and np.array_equal(high, host[f]), (what, p)
        if source[f] is not None:
            assert np.array_equal(got[f], source[f]), (what, p)


def test_both_loaders_in_turn_on_one_detector(files):
    det = mrgingham_amd.Detector()
    calls = [("png16", lambda: det.read_pngs(files["png16"][0], nthreads=4)),
             ("jpeg", lambda: det.read_jpegs(files["jpeg"][0], nthreads=4)),
             ("png8", lambda: det.read_pngs(files["png8"][0], nthreads=4)),
             ("jpeg", lambda: det.read_jpegs(files["jpeg"][0], nthreads=4, entropy="device", sync=True)),
             ("png8", lambda: det.read_pngs(files["png8"][0], nthreads=4)),
             ("jpeg", lambda: det.read_jpegs(files["jpeg"][0], nthreads=4))]
    try:
        for chunk in (2, 0):                                     # chunks of two files: both slots cycle; then single chunks
            det.set_option("jpeg_chunk_frames", chunk)
            det.set_option("png_chunk_frames", chunk)
            for step, (key, call) in enumerate(calls):
                frames, status = call()
                _check(f"call {step + 1} ({key}), chunk {chunk}", files, key, frames, status)
    finally:
        for name in ("jpeg_chunk_frames", "png_chunk_frames", "jpeg_entropy", "jpeg_sync"):
            det.set_option(name, 0)
        det.close()
