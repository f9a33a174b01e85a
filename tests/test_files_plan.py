"""Host-only pieces of the file-list pipeline (mrgingham_amd_find_boards_files): the chunking policy
(mrgingham_amd.files_plan; the same properties again in tests/boundary/files_plan_main.cpp under the sanitizers) and
the header probe (mrgingham_amd.probe_image) against the decoder.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mrgingham_amd
from tests import files_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrgingham_amd", "csrc")


def check_plan(keys, batch):
    keys = np.asarray(keys, np.int32)
    n = len(keys)
    chunk, slot, nchunks = mrgingham_amd.files_plan(keys, batch)
    assert chunk.shape == slot.shape == (n,)
    neg = keys < 0
    assert (chunk[neg] == -1).all() and (slot[neg] == -1).all()                    # keys < 0 are left out
    assert ((chunk[~neg] >= 0) & (chunk[~neg] < nchunks)).all()                    # every batched file has a chunk
    placed = np.zeros(n, bool)
    last_of_key = {}
    prefix = 0

    def skip(prefix):
        while prefix < n and (keys[prefix] < 0 or placed[prefix]):
            prefix += 1
        return prefix
    prefix = skip(prefix)
    for c in range(nchunks):
        m = np.flatnonzero(chunk == c)
        assert 1 <= len(m) <= batch
        assert slot[m].tolist() == list(range(len(m)))                             # exactly one slot each, in list order
        k0 = keys[m[0]]
        assert (keys[m] == k0).all()                                               # homogeneous
        assert m[0] == prefix                                                      # the creation-order rule
        rest = [i for i in np.flatnonzero(keys == k0) if i > last_of_key.get(k0, -1)]
        assert rest[:len(m)] == m.tolist()                                         # the key's NEXT files, none skipped
        if len(m) < batch:
            assert len(rest) == len(m)                                             # a short chunk ends its key
        last_of_key[k0] = m[-1]
        placed[m] = True
        before, prefix = prefix, skip(prefix)
        assert prefix > before                                                     # the final prefix grows with every chunk
    assert prefix == n
    return nchunks


def test_plan_on_seeded_random_keys_and_chunk_sizes():
    rng = np.random.default_rng(20261019)
    for _ in range(300):
        n = int(rng.integers(0, 60))
        nkeys = int(rng.integers(1, 6))
        keys = rng.integers(0, nkeys, n) * 100003 + 7
        if rng.integers(0, 2):
            keys[rng.random(n) < 0.15] = -1 - int(rng.integers(0, 3))
        for batch in (1, int(rng.integers(2, 9)), n + 1 + int(rng.integers(0, 3))):
            check_plan(keys, batch)


def test_plan_fixed_shapes():
    assert check_plan([], 4) == 0                                                  # an empty list
    assert check_plan([-1, -2], 4) == 0
    assert check_plan([3, 3, 3, 3, 3], 1) == 5                                     # batch 1
    assert check_plan([3, 9, 3, 9, 3], 100) == 2                                   # batch >= n
    chunk, slot, n = mrgingham_amd.files_plan([3, -1, 5, 3, 3, 5, 3], 2)            # buckets take turns
    assert chunk.tolist() == [0, -1, 1, 0, 2, 1, 2] and slot.tolist() == [0, -1, 0, 1, 0, 1, 1] and n == 3
    with pytest.raises(ValueError):
        mrgingham_amd.files_plan([1, 2], 0)


def _run_under_sanitizers(tmp_path, name, *args):
    """tests/boundary/<name>_main.cpp, which includes a host-only header of csrc/, built and run as a program of its own."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the sanitizer runtime of g++ is not installed")
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "boundary", name + "_main.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


def test_plan_program_under_sanitizers(tmp_path):
    """tests/boundary/files_plan_main.cpp includes files_plan.h and runs as a program of its own."""
    _run_under_sanitizers(tmp_path, "files_plan", "1500")


def test_loader_chunk_program_under_sanitizers(tmp_path):
    """tests/boundary/loader_plan_main.cpp: loader.h's loader_chunk_frames against a hand-made table and its properties."""
    _run_under_sanitizers(tmp_path, "loader_plan", "4000")


def _decoder_says(path):
    """(height, width, bits) as the decoder sees the file, or None (mrgingham_amd_read_image, sizes only)."""
    import ctypes
    from mrgingham_amd import _lib
    w, h, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if _lib.lib().mrgingham_amd_read_image(os.fsencode(path), 0, None, 0, ctypes.byref(w), ctypes.byref(h), ctypes.byref(d)) != 0:
        return None
    return h.value, w.value, d.value


def test_probe_agrees_with_the_decoder_on_every_fixture(tmp_path):
    paths = files_cases.write_all(tmp_path)
    for name, _, readable, width, height in files_cases.golden_jpegs():
        got = mrgingham_amd.probe_image(paths[name])
        want = _decoder_says(paths[name])
        if readable:
            assert got == (height, width, 8, 3) and want == (height, width, 8), name
        else:                                        # progressive, CMYK: rejected from the header, by both
            assert got is None and want is None, name
    assert mrgingham_amd.probe_image(paths["board.pgm"]) == (480, 640, 8, 1) and _decoder_says(paths["board.pgm"]) == (480, 640, 8)
    assert mrgingham_amd.probe_image(paths["board.png"]) == (480, 640, 8, 2) and _decoder_says(paths["board.png"]) == (480, 640, 8)
    assert mrgingham_amd.probe_image(paths["board16.pgm"]) == (480, 640, 16, 1) and _decoder_says(paths["board16.pgm"]) == (480, 640, 16)
    png16 = tmp_path / "grey16.png"
    files_cases.write_png(png16, (np.arange(12 * 20).reshape(12, 20) * 257).astype(np.uint16), bits=16)
    assert mrgingham_amd.probe_image(png16) == (12, 20, 16, 2) and _decoder_says(png16) == (12, 20, 16)
    assert mrgingham_amd.probe_image(paths["missing"]) is None and _decoder_says(paths["missing"]) is None


def test_probe_rejects_what_the_decoder_rejects_at_header_level(tmp_path):
    paths = files_cases.write_all(tmp_path)
    cases = {}
    for name in ("board.pgm", "board.png", "board16.pgm", files_cases.BOARD, "blend_320x240_420_q90"):
        data = open(paths[name], "rb").read()
        if name.endswith(".pgm"):
            head = len(data) - 640 * 480 * (2 if "16" in name else 1)      # header bytes in front of the pixels
        elif name.endswith(".png"):
            head = 33                                                      # signature + IHDR chunk
        else:
            head = data.index(b"\xff\xda") + 4                            # up to and into the SOS segment
        for cut in (0, 1, 2, 7, 8, 12, 20, head - 3, head - 1):            # inside the header: both reject
            cases[f"{name}.cut{cut}"] = (data[:cut], False)
        if name.endswith(".pgm"):                                          # a PGM shorter than its header promises
            cases[f"{name}.short"] = (data[:-1], False)
        cases[f"{name}.whole"] = (data, True)
    cases["empty"] = (b"", False)
    cases["text"] = (b"hello, world: not an image at all", False)
    cases["pgm_zero_width"] = (b"P5\n0 4\n255\n" + bytes(16), False)
    cases["pgm_maxval_0"] = (b"P5\n4 4\n0\n" + bytes(16), False)
    cases["pgm_maxval_65536"] = (b"P5\n4 4\n65536\n" + bytes(32), False)
    cases["pgm_side_32768"] = (b"P5\n32768 1\n255\n" + bytes(32768), False)
    cases["pgm_long_comment"] = (b"P5\n#" + b"c" * 6000 + b"\n4 2\n255\n" + bytes(8), True)
    for label, (data, accepted) in cases.items():
        p = tmp_path / ("case_" + label)
        p.write_bytes(data)
        got, want = mrgingham_amd.probe_image(p), _decoder_says(p)
        assert (got is not None) == accepted, label
        assert (want is not None) == accepted, label
        if accepted:
            assert got[:3] == want, label
    # kMaxSide + 1 in a PNG header: refused before anything is sized from it; kMaxSide itself passes the probe
    tiny = np.zeros((2, 2), np.uint8)
    for w, h, ok in ((32768, 2, False), (2, 32768, False), (32767, 2, True)):
        p = tmp_path / f"png_{w}x{h}.png"
        files_cases.write_png(p, tiny, width=w, height=h)
        assert (mrgingham_amd.probe_image(p) is not None) == ok
        assert _decoder_says(p) is None                       # (the decoder goes on to the pixels, which are not there)
    for bad_ihdr in (struct_ihdr(2, 2, 4, 0, 0), struct_ihdr(2, 2, 8, 0, 1), struct_ihdr(2, 2, 16, 3, 0), struct_ihdr(2, 2, 8, 5, 0)):
        p = tmp_path / "bad.png"
        p.write_bytes(bad_ihdr)
        assert mrgingham_amd.probe_image(p) is None and _decoder_says(p) is None


def struct_ihdr(w, h, bits, ctype, interlace):
    import struct
    import zlib
    body = struct.pack(">IIBBBBB", w, h, bits, ctype, 0, 0, interlace)
    idat = zlib.compress(bytes((w * 8 + 1) * h))
    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", body) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")
