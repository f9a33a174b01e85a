"""Packed 10 / 12 / 14-bit camera frames on the host (raw_unpack, raw_row_bytes; csrc/image_io.cpp over csrc/raw_pixels.h,
the text the kernel runs), no GPU: against the numpy packer and yardstick of tests/raw_cases.py, which are first held
against the known answers of the format definitions, and through a stand-alone program under the address and
undefined-behaviour sanitizers.  The formats are lossless bit layouts: np.array_equal everywhere, no tolerance."""
import ctypes
import subprocess

import numpy as np
import pytest

import mrgingham_amd
from mrgingham_amd import _lib
from tests import raw_cases as rc
from tests.host_program import build_sanitized


def test_the_packer_gives_the_known_answers():
    rc.check_known()
    for fmt in rc.FORMATS:                                    # and the yardstick undoes the packer, padding set to ones
        a = rc.random_frames(1, 7, 13, fmt, seed=1)[0]
        for pad in (0, 3):
            rows = rc.pack(a, fmt, rc.min_row_bytes(13, fmt) + pad)
            assert rows.shape == (7, rc.min_row_bytes(13, fmt) + pad) and np.array_equal(rc.unpack(rows, 13, fmt), a)
            assert pad == 0 or (rows[:, -pad:] == 0xFF).all()


def test_known_answers_through_the_library():
    for fmt, samples, data in rc.KNOWN:
        got = mrgingham_amd.raw_unpack(data, 1, len(samples), fmt)
        assert got.dtype == np.uint16 and got.shape == (1, len(samples)) and got[0].tolist() == list(samples), fmt
    # the ignored bits of a GEV10 middle byte
    assert mrgingham_amd.raw_unpack(bytes([0xA9, 0x13 | 0xCC, 0x56]), 1, 2, "gev10")[0].tolist() == [0x2A7, 0x159]


def test_row_bytes_against_the_table():
    L = _lib.lib()
    for w in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 300, 4096, 32767):
        assert mrgingham_amd.raw_row_bytes(w, "p10") == -(-w * 10 // 8)
        assert mrgingham_amd.raw_row_bytes(w, "p12") == -(-w * 12 // 8)
        assert mrgingham_amd.raw_row_bytes(w, "p14") == -(-w * 14 // 8)
        assert mrgingham_amd.raw_row_bytes(w, "gev10") == mrgingham_amd.raw_row_bytes(w, "gev12") == 3 * -(-w // 2)
        for fmt in rc.FORMATS:
            assert mrgingham_amd.raw_row_bytes(w, fmt) == rc.min_row_bytes(w, fmt)
    assert [mrgingham_amd.RAW_FORMATS[f] for f in rc.FORMATS] == [0, 1, 2, 3, 4]
    for w, f in ((0, 0), (-1, 1), (32768, 2), (8, 5), (8, -1)):
        assert L.mrgingham_amd_raw_row_bytes(w, f) == -1
    for bad in ("P12", "mono12p", 1, None):
        with pytest.raises(ValueError):
            mrgingham_amd.raw_row_bytes(8, bad)
    with pytest.raises(ValueError):
        mrgingham_amd.raw_row_bytes(0, "p12")


@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_unpack_equals_numpy(fmt):
    """every shape at the minimum row_bytes and with three bytes of row padding; padding bits, padding bytes and the
    ignored bits of GEV10 are ones"""
    for k, (h, w) in enumerate(rc.SHAPES):
        a = rc.random_frames(1, h, w, fmt, seed=100 + k)[0]
        rmin = rc.min_row_bytes(w, fmt)
        for rowb in (rmin, rmin + 3):
            rows = rc.pack(a, fmt, rowb)
            data = rows.reshape(-1)[:(h - 1) * rowb + rmin]          # (not a byte behind the last row's samples)
            want = rc.unpack(rows, w, fmt)
            assert np.array_equal(want, a)
            got = mrgingham_amd.raw_unpack(data.tobytes(), h, w, fmt, row_bytes=rowb)
            assert got.dtype == np.uint16 and got.shape == (h, w) and np.array_equal(got, want), (h, w, rowb)
            if rowb == rmin:
                assert np.array_equal(mrgingham_amd.raw_unpack(data, h, w, fmt), want), (h, w)     # a uint8 array, the default row


@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_every_value_once(fmt):
    a = rc.every_value(fmt)
    n = 1 << rc.BITS[fmt]
    assert np.array_equal(np.sort(a.reshape(-1)[:n]), np.arange(n))
    got = mrgingham_amd.raw_unpack(rc.pack(a, fmt).tobytes(), a.shape[0], a.shape[1], fmt)
    assert np.array_equal(got, a)


@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_nothing_leaks_between_neighbours(fmt):
    """2^N - 1 at one of the pixels 0 .. 15 and 0 elsewhere, and the complement; the bits no sample owns are zeros here, so
    a one that shows anywhere else came from the neighbour"""
    frames = rc.single_pixel_frames(fmt)
    for k, a in enumerate(frames):
        for fill in (False, True):
            got = mrgingham_amd.raw_unpack(rc.pack(a, fmt, fill=fill).tobytes(), 1, 16, fmt)
            assert np.array_equal(got, a), (k, fill)


def test_argument_errors_leave_out_untouched():
    L = _lib.lib()
    h, w = 5, 9
    for f, fmt in enumerate(rc.FORMATS):
        rmin = rc.min_row_bytes(w, fmt)
        rowb = rmin + 2
        a = rc.random_frames(1, h, w, fmt, seed=f)[0]
        pay = np.ascontiguousarray(rc.pack(a, fmt, rowb).reshape(-1)[:(h - 1) * rowb + rmin])
        out = np.full((h, w + 2), 0xA5A5, np.uint16)

        def call(payload=pay.ctypes.data, nbytes=pay.size, width=w, height=h, row_bytes=rowb, fmt_=f, o=out.ctypes.data, stride=w + 2):
            return L.mrgingham_amd_raw_unpack_image(payload, nbytes, width, height, row_bytes, fmt_, o, stride)
        bad = [dict(nbytes=pay.size - 1), dict(nbytes=0), dict(row_bytes=rmin - 1), dict(row_bytes=0), dict(row_bytes=-rowb),
               dict(row_bytes=rowb + 1), dict(fmt_=5), dict(fmt_=-1), dict(width=0), dict(width=-1), dict(width=32768, stride=32768),
               dict(height=0), dict(height=-1), dict(height=32768), dict(height=h + 1), dict(stride=w - 1), dict(payload=None), dict(o=None)]
        for kw in bad:
            assert call(**kw) == -1, (fmt, kw)
        assert (out == 0xA5A5).all(), fmt
        assert call() == 0
        assert np.array_equal(out[:, :w], a) and (out[:, w:] == 0xA5A5).all(), fmt
        with pytest.raises(ValueError):
            mrgingham_amd.raw_unpack(pay.tobytes()[:-1], h, w, fmt, row_bytes=rowb)
        with pytest.raises(ValueError):
            mrgingham_amd.raw_unpack(pay.tobytes(), h, w, fmt, row_bytes=rmin - 1)
    with pytest.raises(ValueError):
        mrgingham_amd.raw_unpack(bytes(64), 2, 4, "p16")
    with pytest.raises(ValueError):
        mrgingham_amd.raw_unpack(np.zeros(64, np.uint16), 2, 4, "p12")


def test_geometry_and_abi():
    lanes, per_cu = mrgingham_amd.raw_unpack_geometry()
    assert lanes == 256 and per_cu == 8
    assert _lib.lib().mrgingham_amd_abi_version() == 4
    for name in ("mrgingham_amd_raw_row_bytes", "mrgingham_amd_raw_unpack_image", "mrgingham_amd_raw_unpack_batch",
                 "mrgingham_amd_raw_unpack_geometry"):
        assert name in _lib.EXPORTS
    assert _lib.lib().mrgingham_amd_raw_unpack_batch(None, None, 0, 0, 1, 1, 2, 1, None, 0, 1, None) == -1     # no context: no device work


def test_host_entry_under_address_and_undefined_sanitizers(tmp_path):
    """the host readers (tests/host_program.py) built with -fsanitize=address,undefined into a stand-alone program
    (tests/boundary/raw_unpack_main.cpp), run as a child process: the host entry and the pixel text on payloads held in
    heap buffers of exactly nbytes, against a bit-by-bit decoder."""
    exe = build_sanitized(tmp_path, "raw_unpack_main.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.stdout, r.stderr[-4000:])
    words = r.stdout.split()
    assert words[0::2] == ["frames", "multiple4", "other", "words"], r.stdout
    frames, mult4, other, nwords = (int(v) for v in words[1::2])
    assert frames == 5 * 19 * 5 * 4 and mult4 > 100 and other > 100 and nwords > 100000
