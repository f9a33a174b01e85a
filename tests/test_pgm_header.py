"""The one parser of a binary PGM's header (mrgingham_amd.pgm_header over mrgingham_amd_pgm_header; no GPU) against the
two things built on it, read_image and probe_image: the three agree on every file, and a file is readable exactly when
its header is good and the payload is all there.  tests/boundary/pgm_header_main.cpp walks truncations and corruptions
of a good file under the address and undefined-behaviour sanitizers as a program of its own.  And the loader flags of
mrgingham_amd_find_boards_files_ex, as far as they can be checked without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mrgingham_amd
from mrgingham_amd import _lib
from tests import files_cases
from tests.host_program import build_sanitized


def test_loader_flags_of_find_boards_files_ex():
    """nfiles 0 needs no device: PNG_DEVICE (1), DEEP_CHUNKS (2) and both are accepted, any other bit is refused."""
    L = _lib.lib()
    o = _lib.FilesOptions(1, 1, 10, -1, 1, 4, 2, 0, -1)
    cb = _lib.PROGRESS_F(lambda nfinal, cookie: None)
    for flags, want in ((0, 0), (1, 0), (2, 0), (3, 0), (4, -1), (6, -1), (8, -1)):
        assert L.mrgingham_amd_find_boards_files_ex(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, flags) == want, flags


def test_deep_keyword_is_checked_before_anything_else():
    with pytest.raises(ValueError, match='deep is "one" or "chunks"'):
        mrgingham_amd.find_boards_files([], deep="both")


def _pgm(w, h, maxval, payload=None, head=None):
    es = 2 if maxval > 255 else 1
    head = (b"P5\n%d %d\n%d\n" % (w, h, maxval)) if head is None else head
    return head + (bytes(range(256)) * (w * h * es // 256 + 1))[:w * h * es] if payload is None else head + payload


def _cases(tmp_path):
    """{label: (bytes, readable)}: the PGM cases of tests/test_files_plan.py, more maxvals, payloads a byte short."""
    paths = files_cases.write_all(tmp_path)
    cases = {}
    for name in ("board.pgm", "board16.pgm"):
        data = open(paths[name], "rb").read()
        head = len(data) - 640 * 480 * (2 if "16" in name else 1)
        for cut in (0, 1, 2, 7, 8, 12, 20, head - 3, head - 1):
            cases[f"{name}.cut{cut}"] = (data[:cut], False)
        cases[f"{name}.short"] = (data[:-1], False)
        cases[f"{name}.whole"] = (data, True)
        cases[f"{name}.longer"] = (data + b"xyz", True)               # (bytes behind the payload are not the decoder's business)
    cases["empty"] = (b"", False)
    cases["text"] = (b"hello, world: not an image at all", False)
    cases["pgm_zero_width"] = (b"P5\n0 4\n255\n" + bytes(16), False)
    cases["pgm_maxval_0"] = (b"P5\n4 4\n0\n" + bytes(16), False)
    cases["pgm_maxval_65536"] = (b"P5\n4 4\n65536\n" + bytes(32), False)
    cases["pgm_side_32768"] = (b"P5\n32768 1\n255\n" + bytes(32768), False)
    cases["pgm_long_comment"] = (b"P5\n#" + b"c" * 6000 + b"\n4 2\n255\n" + bytes(8), True)
    cases["pgm_long_comment16"] = (b"P5\n#" + b"c" * 9000 + b"\n4 2\n4095\n" + bytes(16), True)
    for maxval in (1, 255, 256, 4095, 65535):
        cases[f"maxval_{maxval}"] = (_pgm(5, 3, maxval), True)
        cases[f"maxval_{maxval}_short"] = (_pgm(5, 3, maxval)[:-1], False)
    cases["maxval_2e30"] = (_pgm(5, 3, 1 << 31, payload=bytes(30)), False)
    cases["odd_offset_comments"] = (_pgm(5, 3, 65535, head=b"P5 # one\n# two.\n5\t3 #three\n65535\r"), True)
    cases["no_space_after_magic"] = (_pgm(5, 3, 255, head=b"P55 3 255 "), True)       # (the numbers begin right behind "P5")
    cases["p6"] = (b"P6\n4 4\n255\n" + bytes(48), False)
    cases["header_only"] = (b"P5\n4 4\n255", False)
    cases["header_and_white"] = (b"P5\n4 4\n255\n", False)
    cases["negative"] = (b"P5\n-4 4\n255\n" + bytes(16), False)
    return cases


def _decoder_says(path):
    L = _lib.lib()
    w, h, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if L.mrgingham_amd_read_image(os.fsencode(path), 0, None, 0, ctypes.byref(w), ctypes.byref(h), ctypes.byref(d)) != 0:
        return None
    return h.value, w.value, d.value


def test_pgm_header_and_probe_image_agree_with_read_image(tmp_path):
    readable = 0
    for label, (data, accepted) in _cases(tmp_path).items():
        p = tmp_path / ("case_" + label)
        p.write_bytes(data)
        want = _decoder_says(str(p))
        assert (want is not None) == accepted, label
        head = mrgingham_amd.pgm_header(data)
        by_header = None
        if head is not None and head != mrgingham_amd.PGM_HEADER_CUT:
            hh, ww, bits, off = head
            assert bits in (8, 16) and off <= len(data), label
            if len(data) - off >= hh * ww * bits // 8:
                by_header = (hh, ww, bits)
        assert by_header == want, label
        probe = mrgingham_amd.probe_image(str(p))
        assert (None if probe is None else probe[:3]) == want and (probe is None or probe[3] == 1), label
        # the first bytes of a file: the header of a readable file is there or asks for more, never a different verdict
        if accepted:
            first = mrgingham_amd.pgm_header(data[:4096])
            assert first == head or first == mrgingham_amd.PGM_HEADER_CUT, label
            readable += 1
    assert readable >= 12


def test_the_offset_is_where_the_samples_begin(tmp_path):
    data = _pgm(5, 3, 65535, head=b"P5 # one\n# two.\n5\t3 #three\n65535\r")
    hh, ww, bits, off = mrgingham_amd.pgm_header(data)
    assert (hh, ww, bits) == (3, 5, 16) and off == len(data) - 30 and off % 2 == 1
    assert mrgingham_amd.pgm_header(data[:off - 1]) == mrgingham_amd.PGM_HEADER_CUT and mrgingham_amd.pgm_header(data[:off]) == (3, 5, 16, off)
    assert mrgingham_amd.pgm_header(b"P5") == mrgingham_amd.PGM_HEADER_CUT and mrgingham_amd.pgm_header(b"P") is None and mrgingham_amd.pgm_header(b"") is None
    L = _lib.lib()
    assert L.mrgingham_amd_pgm_header(data, len(data), None, None, None, None) == 0


def test_header_program_under_sanitizers(tmp_path):
    """tests/boundary/pgm_header_main.cpp with the host readers (tests/host_program.py), as a program of its own: every truncation of a good
    16-bit file and several hundred single-byte corruptions of its header."""
    exe = build_sanitized(tmp_path, "pgm_header_main.cpp")
    head = b"P5\n# a comment, then the sizes\n12 7 # and one more\n65535\n"
    good = tmp_path / "good16.pgm"
    good.write_bytes(head + np.arange(12 * 7, dtype=">u2").tobytes())
    r = subprocess.run([exe, str(good), str(tmp_path / "scratch.pgm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) >= len(head) + 12 * 7 * 2 + 300, r.stdout
    assert int(words[3]) >= 1 and int(words[5]) >= len(head) - 2, r.stdout      # the whole file is readable; the header's truncations are cut
