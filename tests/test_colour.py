"""Colour frames to grey on the host (colour_grey; csrc/image_io.cpp over csrc/colour_pixels.h, the text the kernel runs),
no GPU: against the numpy yardstick of tests/colour_cases.py, which is first held against the known answers of the
definition; tied to the colour file readers through PNG and PAM files of the same samples; and through a stand-alone
program under the address and undefined-behaviour sanitizers.  The definition is integer: np.array_equal everywhere, no
tolerance."""
import subprocess

import numpy as np
import pytest

import mrgingham_amd
from mrgingham_amd import _lib
from tests import colour_cases as cc
from tests import png_cases, pnm_cases
from tests.host_program import build_sanitized

CASES = cc.cases()
CASE_IDS = [f"{fmt}-{np.dtype(dtype).name}" for fmt, dtype in CASES]


def _image(frame, fmt, strided=False):
    """mrgingham_amd_colour_grey_image on rows w*C + 3 apart (planar: w + 3, the planes h rows and 5 samples apart) into rows
    w + 2 apart, or dense; everything else 0xA5, and what lies outside w x h of the output must keep it"""
    h, w = cc.hw(fmt, frame.shape)
    dtype = frame.dtype
    fill = 0xA5A5 & np.iinfo(dtype).max
    C = cc.CHANNELS[fmt] or 1
    stride, out_stride = (w * C + 3, w + 2) if strided else (w * C, w)
    if cc.planar(fmt):
        pitch = h * stride + (5 if strided else 0)
        src = np.full(3 * pitch, fill, dtype)
        np.lib.stride_tricks.as_strided(src, (3, h, w), (pitch * src.itemsize, stride * src.itemsize, src.itemsize))[...] = frame
    else:
        pitch = 0
        src = np.full((h, stride), fill, dtype)
        src[:, :w * C] = frame.reshape(h, w * C)
    out = np.full((h, out_stride), fill, dtype)
    rc = _lib.lib().mrgingham_amd_colour_grey_image(src.ctypes.data, 8 * src.itemsize, mrgingham_amd.COLOUR_FORMATS[fmt], w, h, stride, pitch,
                                                    out.ctypes.data, out_stride)
    assert rc == 0
    assert (out[:, w:] == fill).all(), (frame.shape, fmt)
    return out[:, :w]


def test_the_yardstick_gives_the_known_answers():
    cc.check_known()


def test_known_answers_through_the_library():
    cc.check_known(mrgingham_amd.colour_grey)
    cc.check_known(_image)
    cc.check_known(lambda f, fmt: _image(f, fmt, strided=True))


@pytest.mark.parametrize("fmt,dtype", CASES, ids=CASE_IDS)
def test_grey_equals_numpy(fmt, dtype):
    """every shape, dense rows and strided rows; what lies outside w x h of `out` keeps its 0xA5"""
    for k, (h, w) in enumerate(cc.SHAPES):
        f = cc.random_frames(1, h, w, fmt, dtype, seed=100 + k)[0]
        want = cc.grey(f, fmt)
        got = mrgingham_amd.colour_grey(f, fmt)
        assert got.dtype == dtype and got.shape == (h, w) and np.array_equal(got, want), (h, w)
        assert np.array_equal(_image(f, fmt), want), (h, w)
        assert np.array_equal(_image(f, fmt, strided=True), want), (h, w)


@pytest.mark.parametrize("fmt,dtype", CASES, ids=CASE_IDS)
def test_impulses(fmt, dtype):
    """the top value in one sample of one pixel of a 3 x 5 frame in turn, every channel: the grey is the yardstick's, and
    an alpha or chroma impulse changes nothing"""
    frames = cc.impulse_frames(fmt, dtype)
    skip = cc.ignored(fmt)
    assert skip.sum() == {3: 0, 4: 15, 0: 0, 2: 15}[cc.CHANNELS[fmt]]
    for k, f in enumerate(frames):
        got = mrgingham_amd.colour_grey(f, fmt)
        assert np.array_equal(got, cc.grey(f, fmt)), (fmt, k)
        assert np.array_equal(_image(f, fmt, strided=True), got), (fmt, k)
        assert (not got.any()) == bool(skip[k]), (fmt, k)


@pytest.mark.parametrize("fmt,dtype", CASES, ids=CASE_IDS)
def test_all_top_gives_top(fmt, dtype):
    top = np.iinfo(dtype).max
    for h, w in ((1, 1), (3, 5), (9, 17), (4, 33)):
        assert (mrgingham_amd.colour_grey(np.full(cc.frame_shape(fmt, h, w), top, dtype), fmt) == top).all(), (h, w)


def test_argument_errors_leave_out_untouched():
    L = _lib.lib()
    h, w = 5, 9
    for fmt, dtype in CASES:
        f = mrgingham_amd.COLOUR_FORMATS[fmt]
        C = cc.CHANNELS[fmt] or 1
        fill = 0xA5A5 & np.iinfo(dtype).max
        stride = w * C + 3
        pitch = h * stride + 5
        frame = cc.random_frames(1, h, w, fmt, dtype, seed=1)[0]
        src = np.zeros(3 * pitch, dtype)
        if cc.planar(fmt):
            np.lib.stride_tricks.as_strided(src, (3, h, w), (pitch * src.itemsize, stride * src.itemsize, src.itemsize))[...] = frame
        else:
            src[:h * stride].reshape(h, stride)[:, :w * C] = frame.reshape(h, w * C)
        out = np.full((h, w + 2), fill, dtype)

        def call(image=src.ctypes.data, bits=8 * src.itemsize, format=f, width=w, height=h, stride_=stride, pitch_=pitch, o=out.ctypes.data,
                 out_stride=w + 2):
            return L.mrgingham_amd_colour_grey_image(image, bits, format, width, height, stride_, pitch_, o, out_stride)
        bad = [dict(image=None), dict(o=None), dict(format=8), dict(format=-1), dict(bits=12), dict(bits=0), dict(bits=32), dict(width=0),
               dict(width=-1), dict(height=0), dict(height=-1), dict(width=32768, stride_=32768 * C, out_stride=32768), dict(height=32768),
               dict(stride_=w * C - 1), dict(out_stride=w - 1), dict(stride_=0), dict(stride_=-stride), dict(out_stride=-(w + 2))]
        if cc.planar(fmt):
            bad += [dict(pitch_=-1), dict(pitch_=-pitch)]
        if np.dtype(dtype) == np.uint8:
            bad += [dict(bits=16, format=6), dict(bits=16, format=7)]
        for kw in bad:
            assert call(**kw) == -1, (fmt, dtype, kw)
        assert (out == fill).all(), (fmt, dtype)
        if not cc.planar(fmt):                                           # plane_pitch is read for the planar formats only
            assert call(pitch_=-7) == 0
            out[...] = fill
        assert call() == 0
        assert np.array_equal(out[:, :w], cc.grey(frame, fmt)) and (out[:, w:] == fill).all(), (fmt, dtype)
    for bad in ("RGB", "rgbx", "argb", "nv12", 0, None):
        with pytest.raises(ValueError):
            mrgingham_amd.colour_grey(np.zeros((4, 4, 3), np.uint8), bad)
    for bad, fmt in ((np.zeros((4, 4, 3), np.int16), "rgb"), (np.zeros((4, 4, 3), np.float32), "rgb"), (np.zeros((4, 4), np.uint8), "rgb"),
                     (np.zeros((4, 4, 4), np.uint8), "rgb"), (np.zeros((4, 4, 3), np.uint8), "rgba"), (np.zeros((4, 4, 3), np.uint8), "rgb_planar"),
                     (np.zeros((3, 4, 4), np.uint8), "bgr"), (np.zeros((4, 4, 2), np.uint16), "yuyv"), (np.zeros((4, 4, 3), np.uint8), "uyvy"),
                     (np.zeros((0, 4, 3), np.uint8), "rgb"), (np.zeros((3, 4, 0), np.uint8), "rgb_planar")):
        with pytest.raises(ValueError):
            mrgingham_amd.colour_grey(bad, fmt)


def test_formats_exports_and_abi():
    assert mrgingham_amd.COLOUR_FORMATS == {"rgb": 0, "bgr": 1, "rgba": 2, "bgra": 3, "rgb_planar": 4, "bgr_planar": 5, "yuyv": 6, "uyvy": 7}
    assert tuple(mrgingham_amd.COLOUR_FORMATS) == cc.FORMATS
    for name in ("mrgingham_amd_colour_grey_image", "mrgingham_amd_colour_grey_batch", "mrgingham_amd_colour_grey_geometry"):
        assert name in _lib.EXPORTS
    assert _lib.lib().mrgingham_amd_abi_version() == 4
    lanes, per_cu = mrgingham_amd.colour_grey_geometry()
    assert lanes % 64 == 0 and lanes > 0 and per_cu > 0
    assert (lanes, per_cu) == mrgingham_amd.pnm_unpack_geometry()                 # the one row schedule
    assert _lib.lib().mrgingham_amd_colour_grey_batch(None, None, 8, 0, 0, 4, 4, 48, 0, 12, None, 16, 4, None) == -1     # no context: no device work


@pytest.mark.parametrize("bits", (8, 16))
@pytest.mark.parametrize("color_type,fmt", ((2, "rgb"), (6, "rgba")))
def test_png_reader_gives_the_same_grey(tmp_path, color_type, fmt, bits):
    """an RGB and an RGBA PNG of random samples: read_image of the file (16 bit: the high byte of the 16-bit grey) equals
    colour_grey of the same samples -- the readers' png_grey and the pixel text's expression are one formula"""
    dtype = np.uint8 if bits == 8 else np.uint16
    for k, (h, w) in enumerate(((9, 17), (4, 33))):
        samples = cc.random_frames(1, h, w, fmt, dtype, seed=40 + k)[0]
        path = tmp_path / f"c{color_type}_{bits}_{k}.png"
        png_cases.write(str(path), samples, color_type, bits)
        got = mrgingham_amd.read_image(str(path))
        want = mrgingham_amd.colour_grey(samples, fmt)
        assert np.array_equal(want, png_cases.grey_of(samples, color_type))
        assert got is not None and np.array_equal(got, want if bits == 8 else (want >> 8).astype(np.uint8)), (h, w)


@pytest.mark.parametrize("bits", (8, 16))
def test_pam_reader_gives_the_same_grey(tmp_path, bits):
    """the same for a PAM depth-3 file"""
    dtype = np.uint8 if bits == 8 else np.uint16
    for k, (h, w) in enumerate(((9, 17), (4, 33))):
        samples = cc.random_frames(1, h, w, "rgb", dtype, seed=50 + k)[0]
        path = tmp_path / f"rgb{bits}_{k}.pam"
        path.write_bytes(pnm_cases.write(samples, 7, bits))
        got = mrgingham_amd.read_image(str(path))
        want = mrgingham_amd.colour_grey(samples, "rgb")
        assert np.array_equal(want, pnm_cases.expected(samples, bits, 3))
        assert got is not None and np.array_equal(got, want if bits == 8 else (want >> 8).astype(np.uint8)), (h, w)


def test_host_entry_under_address_and_undefined_sanitizers(tmp_path):
    """the host readers (tests/host_program.py) built with -fsanitize=address,undefined into a stand-alone program
    (tests/boundary/colour_main.cpp), run as a child process: the host entry on heap buffers of exactly the bytes the
    arguments describe, at all 16 byte phases of source and destination, every format, sample width and width, against a
    per-pixel decoder written from the definition."""
    exe = build_sanitized(tmp_path, "colour_main.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.stdout, r.stderr[-4000:])
    words = r.stdout.split()
    assert words[0::2] == ["frames", "pixels", "refused"], r.stdout
    frames, pixels, refused = (int(v) for v in words[1::2])
    assert frames == len(cc.SHAPES) * len(CASES) * 16                     # shapes x (format, dtype) x byte phases
    assert pixels == len(CASES) * 16 * sum(h * w for h, w in cc.SHAPES) and refused == 8 * frames
