"""The host half of the PNG device route (mrgingham_amd.png_scanlines over mrgingham_amd_png_scanlines; no GPU): the
inflated, still filtered scanlines of every pixel size the device takes, the sizes, the palette code, and the files that
break a rule -- each judged exactly as read_image judges it.  tests/boundary/png_scanlines_main.cpp walks the same files
under the address and undefined-behaviour sanitizers as a program of its own."""
import struct
import subprocess

import numpy as np
import pytest

import mrgingham_amd
from tests import png_cases
from tests.host_program import build_sanitized


def palette_file():
    rng = np.random.default_rng(5)
    palette = rng.integers(0, 256, (17, 3)).astype(np.uint8)
    idx = rng.integers(0, 17, (7, 9)).astype(np.uint8)
    data, _ = png_cases.encode(idx, 3, 8, filters="rotate", palette=palette)
    p = palette.astype(np.uint32)
    grey = ((p[:, 0] * 4899 + p[:, 1] * 9617 + p[:, 2] * 1868 + 8192) >> 14).astype(np.uint8)
    return data, grey[idx]


def read_bytes(tmp_path, data, name="case.png"):
    path = tmp_path / name
    path.write_bytes(data)
    return mrgingham_amd.read_image(str(path)), str(path)


@pytest.mark.parametrize("color_type,bits", png_cases.TAKEN, ids=[f"type{c}_{b}bit" for c, b in png_cases.TAKEN])
def test_scanlines_are_the_writers_filtered_bytes(tmp_path, color_type, bits):
    img = png_cases.random_image(21, 13, color_type, bits, seed=color_type + bits)
    for filters, nidat in (("rotate", 1), (("random", 7), 3), (4, 2)):
        data, scan = png_cases.encode(img, color_type, bits, filters=filters, nidat=nidat)
        got = mrgingham_amd.png_scanlines(data)
        assert got is not None and got is not mrgingham_amd.PNG_NOT_TAKEN
        assert got[1:] == ((13, 21), bits, color_type)
        assert got[0].dtype == np.uint8 and got[0].shape == (13, 21 * png_cases.bpp_of(color_type, bits) + 1)
        assert np.array_equal(got[0], scan)
        # the size query agrees with probe_image, and read_image reads the file: the writer's grey (the high byte of 16 bit)
        pixels, path = read_bytes(tmp_path, data)
        assert mrgingham_amd.probe_image(path) == (13, 21, bits, 2)
        want = png_cases.grey_of(img, color_type)
        assert np.array_equal(pixels, want if bits == 8 else (want >> 8).astype(np.uint8))


def test_a_palette_file_is_readable_but_not_taken(tmp_path):
    data, grey = palette_file()
    assert mrgingham_amd.png_scanlines(data) is mrgingham_amd.PNG_NOT_TAKEN
    pixels, path = read_bytes(tmp_path, data)
    assert np.array_equal(pixels, grey)
    assert mrgingham_amd.probe_image(path) == (7, 9, 8, 2)


def test_the_capacity_is_checked_and_sizes_are_still_reported():
    import ctypes
    from mrgingham_amd import _lib
    L = _lib.lib()
    img = png_cases.random_image(9, 7, 2, 8)
    data, scan = png_cases.encode(img, 2, 8)
    w, h, b, ct = (ctypes.c_int() for _ in range(4))
    refs = [ctypes.byref(v) for v in (w, h, b, ct)]
    buf = np.full(scan.size + 8, 0xAB, np.uint8)
    assert L.mrgingham_amd_png_scanlines(data, len(data), buf.ctypes.data, scan.size - 1, *refs) == -2
    assert (w.value, h.value, b.value, ct.value) == (9, 7, 8, 2) and (buf == 0xAB).all()
    assert L.mrgingham_amd_png_scanlines(data, len(data), buf.ctypes.data, scan.size, *refs) == 0
    assert np.array_equal(buf[:scan.size], scan.reshape(-1)) and (buf[scan.size:] == 0xAB).all()
    assert L.mrgingham_amd_png_scanlines(None, 0, None, 0, *refs) == -1
    assert L.mrgingham_amd_png_scanlines(data, len(data), None, 0, None, None, None, None) == 0


BROKEN, GOOD, GOOD_IMG = png_cases.broken_files()


def test_the_good_file_the_broken_ones_are_cut_from_is_good(tmp_path):
    got = mrgingham_amd.png_scanlines(GOOD)
    assert got is not None and got[1:] == ((7, 9), 8, 0)
    assert np.array_equal(read_bytes(tmp_path, GOOD)[0], GOOD_IMG)


@pytest.mark.parametrize("name", ["interlace", "depth4", "filter5", "truncated_idat", "row_too_few", "row_too_many",
                                  "ihdr_not_first", "two_ihdr", "side_32768"])
def test_unreadable_like_read_image(tmp_path, name):
    assert mrgingham_amd.png_scanlines(BROKEN[name]) is None
    assert read_bytes(tmp_path, BROKEN[name])[0] is None


def test_scanlines_program_under_sanitizers(tmp_path):
    """tests/boundary/png_scanlines_main.cpp with the host readers (tests/host_program.py), as a program of its own: every file of this module, and
    the good ones cut off at a spread of lengths."""
    exe = build_sanitized(tmp_path, "png_scanlines_main.cpp")
    good = [GOOD, palette_file()[0]]
    for color_type, bits in png_cases.TAKEN:
        good.append(png_cases.encode(png_cases.random_image(21, 13, color_type, bits), color_type, bits, filters=("random", 1), nidat=3)[0])
    items = good + list(BROKEN.values())
    for data in good[:4]:
        items += [data[:n] for n in sorted({0, 7, 8, 20, 32, 33, 40, len(data) // 2, len(data) - 13, len(data) - 12, len(data) - 1})]
    blob = tmp_path / "corpus.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for data in items:
            f.write(struct.pack("<I", len(data)) + data)
    r = subprocess.run([exe, str(blob), str(tmp_path / "scratch.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) == len(items), r.stdout
    assert int(words[3]) >= 9 and int(words[5]) >= 1, r.stdout          # the good files were taken, the palette file was not
