"""Bayer mosaics to grey on the host (bayer_grey; csrc/image_io.cpp over csrc/bayer_pixels.h, the text the kernel runs),
no GPU: against the numpy yardstick of tests/bayer_cases.py, which is first held against the known answers of the
definition, and through a stand-alone program under the address and undefined-behaviour sanitizers.  The definition is
integer: np.array_equal everywhere, no tolerance."""
import ctypes
import subprocess

import numpy as np
import pytest

import mrgingham_amd
from mrgingham_amd import _lib, synth
from tests import bayer_cases as bc
from tests.host_program import build_sanitized


def _image(m, pat, stride=None, out_stride=None):
    """mrgingham_amd_bayer_grey_image on rows `stride` apart into rows `out_stride` apart, everything else 0xA5"""
    h, w = m.shape
    stride, out_stride = stride or w, out_stride or w
    src = np.full((h, stride), 0xA5A5 & np.iinfo(m.dtype).max, m.dtype)
    src[:, :w] = m
    out = np.full((h, out_stride), 0xA5A5 & np.iinfo(m.dtype).max, m.dtype)
    rc = _lib.lib().mrgingham_amd_bayer_grey_image(src.ctypes.data, 8 * m.itemsize, w, h, stride, mrgingham_amd.BAYER_PATTERNS[pat],
                                                   out.ctypes.data, out_stride)
    assert rc == 0
    assert (out[:, w:] == (0xA5A5 & np.iinfo(m.dtype).max)).all(), (m.shape, pat)
    return out[:, :w]


def test_the_yardstick_gives_the_known_answers():
    bc.check_known()


def test_known_answers_through_the_library():
    bc.check_known(mrgingham_amd.bayer_grey)
    bc.check_known(lambda m, pat: _image(m, pat, m.shape[1] + 3, m.shape[1] + 2))


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("pat", bc.PATTERNS)
def test_grey_equals_numpy(pat, dtype):
    """every shape, dense rows and strided rows (in w + 3, out w + 2); what lies outside w x h keeps its 0xA5"""
    for k, (h, w) in enumerate(bc.SHAPES):
        m = bc.random_frames(1, h, w, dtype, seed=100 + k)[0]
        want = bc.grey(m, pat)
        got = mrgingham_amd.bayer_grey(m, pat)
        assert got.dtype == dtype and got.shape == (h, w) and np.array_equal(got, want), (h, w)
        assert np.array_equal(_image(m, pat), want), (h, w)
        assert np.array_equal(_image(m, pat, w + 3, w + 2), want), (h, w)


@pytest.mark.parametrize("dtype", bc.DTYPES)
def test_impulses(dtype):
    """the top value at every pixel of a 6 x 7 frame in turn, and the complement: corners, edges and interior at both
    parities; a leak or a wrong reflection shows"""
    frames = bc.impulse_frames(6, 7, dtype)
    for pat in bc.PATTERNS:
        for k, m in enumerate(frames):
            assert np.array_equal(mrgingham_amd.bayer_grey(m, pat), bc.grey(m, pat)), (pat, k)


@pytest.mark.parametrize("dtype", bc.DTYPES)
def test_all_top_gives_top(dtype):
    top = np.iinfo(dtype).max
    for h, w in ((2, 2), (5, 3), (9, 17), (4, 33)):
        for pat in bc.PATTERNS:
            assert (mrgingham_amd.bayer_grey(np.full((h, w), top, dtype), pat) == top).all(), (h, w, pat)


def test_argument_errors_leave_out_untouched():
    L = _lib.lib()
    h, w = 5, 9
    for dtype in bc.DTYPES:
        fill = 0xA5A5 & np.iinfo(dtype).max
        m = np.ascontiguousarray(bc.random_frames(1, h, w + 3, dtype, seed=1)[0])
        out = np.full((h, w + 2), fill, dtype)

        def call(mosaic=m.ctypes.data, bits=8 * m.itemsize, width=w, height=h, stride=w + 3, pattern=0, o=out.ctypes.data, out_stride=w + 2):
            return L.mrgingham_amd_bayer_grey_image(mosaic, bits, width, height, stride, pattern, o, out_stride)
        bad = [dict(mosaic=None), dict(o=None), dict(pattern=4), dict(pattern=-1), dict(bits=12), dict(bits=0), dict(bits=32), dict(width=1),
               dict(width=0), dict(width=-1), dict(height=1), dict(height=0), dict(height=-1), dict(width=32768, stride=32768, out_stride=32768),
               dict(height=32768), dict(stride=w - 1), dict(out_stride=w - 1), dict(stride=0), dict(stride=-(w + 3)), dict(out_stride=-(w + 2))]
        for kw in bad:
            assert call(**kw) == -1, (dtype, kw)
        assert (out == fill).all(), dtype
        assert call() == 0
        assert np.array_equal(out[:, :w], bc.grey(m[:, :w], "rggb")) and (out[:, w:] == fill).all(), dtype
    for bad in ("RGGB", "rgbg", 0, None):
        with pytest.raises(ValueError):
            mrgingham_amd.bayer_grey(np.zeros((4, 4), np.uint8), bad)
    for bad in (np.zeros((4, 4), np.int16), np.zeros((4, 4), np.float32), np.zeros((2, 4, 4), np.uint8), np.zeros((1, 4), np.uint8),
                np.zeros((4, 1), np.uint16)):
        with pytest.raises(ValueError):
            mrgingham_amd.bayer_grey(bad, "rggb")


def test_patterns_exports_and_abi():
    assert mrgingham_amd.BAYER_PATTERNS == {"rggb": 0, "grbg": 1, "gbrg": 2, "bggr": 3}
    assert tuple(mrgingham_amd.BAYER_PATTERNS) == bc.PATTERNS
    for name in ("mrgingham_amd_bayer_grey_image", "mrgingham_amd_bayer_grey_batch", "mrgingham_amd_bayer_grey_geometry"):
        assert name in _lib.EXPORTS
    assert _lib.lib().mrgingham_amd_abi_version() == 4
    lanes, rows, per_cu = mrgingham_amd.bayer_grey_geometry()
    assert lanes % 64 == 0 and lanes > 0 and rows > 0 and rows % 2 == 0 and per_cu >= 0
    assert _lib.lib().mrgingham_amd_bayer_grey_batch(None, None, 8, 0, 4, 4, 16, 4, 0, None, 16, 4, None) == -1     # no context: no device work


def test_host_entry_under_address_and_undefined_sanitizers(tmp_path):
    """the host readers (tests/host_program.py) built with -fsanitize=address,undefined into a stand-alone program
    (tests/boundary/bayer_main.cpp), run as a child process: the host entry on heap buffers of exactly the bytes the
    arguments describe, at all four byte phases, against a per-pixel decoder written from the definition."""
    exe = build_sanitized(tmp_path, "bayer_main.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.stdout, r.stderr[-4000:])
    words = r.stdout.split()
    assert words[0::2] == ["frames", "pixels", "refused"], r.stdout
    frames, pixels, refused = (int(v) for v in words[1::2])
    nshapes = len(bc.SHAPES)
    assert frames == nshapes * 4 * 2 * 4                                  # shapes x patterns x dtypes x byte phases
    assert pixels == 4 * 2 * 4 * sum(h * w for h, w in bc.SHAPES) and refused == 10 * frames


def test_tinted_boards_through_the_reference_detector():
    """a board tinted R : G : B = 1 : 3/4 : 1/2 behind each of the four filters, through the host entry, then the
    oracle's corner finder at level 0: exactly 100 candidates, one per lattice point, each within 0.4 px (the yardstick
    alone gives at most 0.315 px on these 16 cases)"""
    from oracle import oracle
    for seed in range(4):
        lattice = synth.board_lattice(640, 480, 10, seed)
        for pat in bc.PATTERNS:
            m = bc.tinted_board(seed, pat)
            g = mrgingham_amd.bayer_grey(m, pat)
            assert np.array_equal(g, bc.grey(m, pat))
            pts = oracle.find_corners(g, 0)
            assert pts is not None and len(pts) == 100, (seed, pat, None if pts is None else len(pts))
            bc.check_corners(pts / 1000.0, lattice, (seed, pat))
