"""Baseline JPEG on the host (csrc/jpeg.cpp behind mrgingham_amd_read_image and mrgingham_amd_jpeg_coefficients): every
fixture of tests/golden/jpeg_golden.npz (made by make_jpeg_golden.py with Pillow / libjpeg-turbo: the luma plane of
libjpeg's default decoder) byte for byte, the arithmetic of the inverse DCT restated in numpy, and truncated / corrupted
files.  No GPU."""
import os
import struct
import subprocess

import numpy as np

import mrgingham_amd
from tests.host_program import build_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Case:
    def __init__(self, g, i):
        self.name = str(g["name"][i])
        self.data = g[f"jpg_{i}"].tobytes()
        self.readable = bool(g["readable"][i])
        self.luma = g[f"luma_{i}"] if self.readable else None
        self.width, self.height = int(g["width"][i]), int(g["height"][i])
        self.blocks_w, self.blocks_h = int(g["blocks_w"][i]), int(g["blocks_h"][i])


_cases = None


def cases():
    global _cases
    if _cases is None:
        g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz"))
        _cases = [Case(g, i) for i in range(len(g["name"]))]
    return _cases


def case(prefix):
    return next(c for c in cases() if c.name.startswith(prefix))


def _u32(v):
    return np.uint32(v & 0xFFFFFFFF)


def _step(d, s):
    """The one-dimensional step on eight uint32 arrays: sums and products modulo 2^32, the descaling shift arithmetic on
    the value taken as int32."""
    d0, d1, d2, d3, d4, d5, d6, d7 = d
    z1 = (d2 + d6) * _u32(4433)
    t2 = z1 - d6 * _u32(15137)
    t3 = z1 + d2 * _u32(6270)
    t0 = (d0 + d4) << _u32(13)
    t1 = (d0 - d4) << _u32(13)
    e0, e3, e1, e2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = d7, d5, d3, d1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * _u32(9633)
    o0, o1, o2, o3 = o0 * _u32(2446), o1 * _u32(16819), o2 * _u32(25172), o3 * _u32(12299)
    z1, z2 = z1 * _u32(-7373), z2 * _u32(-20995)
    z3 = z3 * _u32(-16069) + z5
    z4 = z4 * _u32(-3196) + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    outs = [e0 + o3, e1 + o2, e2 + o1, e3 + o0, e3 - o0, e2 - o1, e1 - o2, e0 - o3]
    return [((x + _u32(1 << (s - 1))).view(np.int32) >> np.int32(s)).view(np.uint32) for x in outs]


def idct_blocks(coef, quant):
    """coef int16 [..., 64], quant uint16 [64] (or [..., 64]) -> uint8 [..., 8, 8]: pass 1 down the columns (>> 11),
    pass 2 along the rows (>> 18), + 128, clamped."""
    with np.errstate(over="ignore"):
        d = np.ascontiguousarray(coef.astype(np.int32)).view(np.uint32) * quant.astype(np.uint32)
        d = d.reshape(d.shape[:-1] + (8, 8))
        ws = np.stack(_step([d[..., r, :] for r in range(8)], 11), axis=-2)
        px = np.stack(_step([ws[..., :, k] for k in range(8)], 18), axis=-1)
    return np.clip(px.view(np.int32) + 128, 0, 255).astype(np.uint8)


def plane_of(coef, quant, height, width):
    bh, bw = coef.shape[:2]
    px = idct_blocks(coef, quant)                                   # [bh, bw, 8, 8]
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:height, :width]


def _read(tmp_path, data, name="a.jpg"):
    f = tmp_path / name
    f.write_bytes(data)
    return mrgingham_amd.read_image(str(f))


def test_fixture_set_is_what_the_other_tests_rely_on():
    names = [c.name for c in cases()]
    assert 50 <= len(names) <= 70 and len(set(names)) == len(names)
    for size in ("8x8", "17x9", "16x16", "31x33", "53x37", "48x64", "264x16", "520x8", "640x480"):
        assert any(f"_{size}_" in n for n in names), size
    for part in ("_grey_", "_444_", "_422_", "_420_", "_r0", "_r1", "_r3", "_q30_", "_q100_", "sof1_patched", "qtable16",
                 "progressive", "cmyk", "board_640x480"):
        assert any(part in n for n in names), part
    assert [c.name for c in cases() if not c.readable] == ["progressive_48x64_420", "cmyk_16x16"]
    q16 = case("qtable16").data
    assert q16[q16.index(b"\xff\xdb") + 4] >> 4 == 1 and b"\xff\xc1" in q16      # a 16-bit DQT is really in there
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz")) < 512 * 1024


def test_read_image_gives_libjpegs_luma_plane_for_every_fixture(tmp_path):
    for c in cases():
        got = _read(tmp_path, c.data)
        if not c.readable:
            assert got is None, c.name
            continue
        assert got is not None and got.shape == c.luma.shape and np.array_equal(got, c.luma), c.name


def test_jpeg_coefficients_block_counts_and_numpy_idct():
    for c in cases():
        r = mrgingham_amd.jpeg_coefficients(c.data)
        if not c.readable:
            assert r is None, c.name
            continue
        coef, quant, (h, w) = r
        assert (h, w) == (c.height, c.width) and coef.shape == (c.blocks_h, c.blocks_w, 64), c.name
        assert coef.dtype == np.int16 and quant.dtype == np.uint16 and quant.shape == (64,)
        assert np.array_equal(plane_of(coef, quant, h, w), c.luma), c.name
    assert case("noise_31x33_420").blocks_w == 4 and case("noise_31x33_420").blocks_h == 6    # padded past ceil(33 / 8)
    assert mrgingham_amd.jpeg_coefficients(case("qtable16").data)[1].max() == 300


def test_jpeg_coefficients_c_boundary():
    import ctypes
    from mrgingham_amd import _lib
    L = _lib.lib()
    c = case("noise_17x9_420")
    w, h, bw, bh = (ctypes.c_int() for _ in range(4))
    sizes = [ctypes.byref(v) for v in (w, h, bw, bh)]
    assert L.mrgingham_amd_jpeg_coefficients(c.data, len(c.data), None, 0, None, *sizes) == 0
    assert (w.value, h.value, bw.value, bh.value) == (17, 9, 4, 2)
    n = bw.value * bh.value * 64
    small = np.full(n + 64, 77, np.int16)
    assert L.mrgingham_amd_jpeg_coefficients(c.data, len(c.data), small.ctypes.data, n - 1, None, *sizes) == -2
    assert (small == 77).all()                                                 # too small: nothing written
    assert L.mrgingham_amd_jpeg_coefficients(c.data, len(c.data), small.ctypes.data, n, None, *sizes) == 0
    assert (small[n:] == 77).all() and (small[:n] != 77).any()
    assert L.mrgingham_amd_jpeg_coefficients(None, 10, None, 0, None, *sizes) == -1
    assert L.mrgingham_amd_jpeg_coefficients(b"\xff\xd8\xff", 3, None, 0, None, *sizes) == -1


def _sof_size(data, at):
    return struct.unpack(">HH", data[at + 5:at + 9])                          # (height, width) of the SOF segment at `at`


def corpus():
    """Every prefix of two small fixtures and 2000 seeded single-byte corruptions of them: (bytes, offset of the
    fixture's SOF marker) pairs."""
    out = []
    rng = np.random.RandomState(1234)
    small = [case("noise_8x8_grey"), case("noise_31x33_444")]                   # (the second has restart markers)
    assert small[1].name.endswith("_r1") and b"\xff\xd3" in small[1].data
    for c in small:
        at = c.data.index(b"\xff\xc0")
        out += [(c.data[:n], at) for n in range(len(c.data))]
    for k in range(2000):
        c = small[k & 1]
        b = bytearray(c.data)
        b[rng.randint(len(b))] = rng.randint(256)
        out.append((bytes(b), c.data.index(b"\xff\xc0")))
    return out


def test_truncated_and_corrupted_files_return_a_value(tmp_path):
    """A file that still reads after a corruption has the size its frame header states -- the fixture's, except for the
    few corruptions that land in the four size bytes themselves, where libjpeg reports the changed size as well."""
    readable = 0
    for data, at in corpus():
        got = _read(tmp_path, data)
        r = mrgingham_amd.jpeg_coefficients(data)
        assert (got is None) == (r is None)
        if got is not None:
            readable += 1
            assert got.shape == _sof_size(data, at) == r[2]
            assert np.array_equal(got, plane_of(r[0], r[1], *r[2]))
    assert 0 < readable < 2000                                                    # (most corruptions change pixels only)
    assert all(_read(tmp_path, d) is None for d, _ in corpus()[:case("noise_8x8_grey").data.index(b"\xff\xda")])


def test_malformed_jpeg_files_are_unreadable(tmp_path):
    c = case("noise_16x16_444")
    d = c.data
    assert _read(tmp_path, d) is not None
    sof, sos = d.index(b"\xff\xc0"), d.index(b"\xff\xda")
    def patched(at, new):
        return d[:at] + bytes(new) + d[at + len(new):]
    assert _read(tmp_path, patched(sof + 1, [0xC2])) is None                      # progressive
    assert _read(tmp_path, patched(sof + 1, [0xC9])) is None                      # arithmetic
    assert _read(tmp_path, patched(sof + 4, [12])) is None                        # 12 bit
    assert _read(tmp_path, patched(sof + 5, [0, 0])) is None                      # height 0 (DNL)
    assert _read(tmp_path, patched(sof + 5, [0x80, 0x00])) is None                # 32768 rows
    assert _read(tmp_path, patched(sof + 2, [0xFF, 0xFF])) is None                # a segment length past the end of the file
    assert _read(tmp_path, patched(sos + 6, [0x70])) is None                      # Huffman table id 7
    assert _read(tmp_path, d[:sof] + d[sof:sos] + d[sof:]) is None                # two frame headers
    assert _read(tmp_path, d[:-2]) is not None                                    # (a missing EOI alone is tolerated)
    assert _read(tmp_path, d[:-3]) is None                                        # ... a missing last byte of data is not
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"                  # transform 0: RGB data
    assert _read(tmp_path, d[:2] + adobe + d[2:]) is None
    assert _read(tmp_path, d[:2] + adobe[:-1] + b"\x01" + d[2:]) is not None       # transform 1: YCbCr
    r = case("noise_31x33_444")                                                    # restart markers out of sequence
    first = r.data.index(b"\xff\xd0")
    assert _read(tmp_path, r.data[:first + 1] + b"\xd1" + r.data[first + 2:]) is None
    assert _read(tmp_path, r.data[:first] + b"\xff" + r.data[first:]) is not None  # a fill byte in front of one is fine


def test_corpus_under_address_and_undefined_sanitizers(tmp_path):
    """The same corpus through the host readers (tests/host_program.py) built with -fsanitize=address,undefined into a stand-alone
    program (tests/boundary/jpeg_fuzz_main.cpp), run as a child process."""
    exe = build_sanitized(tmp_path, "jpeg_fuzz_main.cpp")
    items = corpus()
    blob = tmp_path / "corpus.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for data, _ in items:
            f.write(struct.pack("<I", len(data)) + data)
    want = sum(mrgingham_amd.jpeg_coefficients(d) is not None for d, _ in items)
    r = subprocess.run([exe, str(blob), str(tmp_path / "scratch.jpg")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.split() == ["cases", str(len(items)), "readable", str(want)], r.stdout
