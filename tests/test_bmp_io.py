"""The host BMP reader (read_image, probe_image, bmp_layout; csrc/image_io.cpp, csrc/bmp_pixels.h), no GPU: files written by
the writer of tests/bmp_cases.py and by Pillow (tests/golden/bmp_golden.npz) against the arrays they were written from
through the library's grey weights, one broken rule per file, and the whole corpus and the pixel text through a
stand-alone program under the address and undefined-behaviour sanitizers.  No tolerance anywhere."""
import io
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import mrgingham_amd
from tests import bmp_cases as bc
from tests.host_program import build_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 65)
HEIGHTS = (1, 2, 5)


def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "bmp_golden.npz"))
    for i, name in enumerate(g["name"]):
        rgb = g[f"img_{i}"]
        yield str(name), g[f"bmp_{i}"].tobytes(), bc.grey(rgb[..., 0], rgb[..., 1], rgb[..., 2]).astype(np.uint8)


def read_all_three(tmp_path, data):
    """-> (read_image's array or None, probe_image's tuple or None, bmp_layout's result or None)"""
    path = str(tmp_path / "case.bmp")
    with open(path, "wb") as f:
        f.write(data)
    return mrgingham_amd.read_image(path), mrgingham_amd.probe_image(path), mrgingham_amd.bmp_layout(data)


def assert_reads_to(tmp_path, data, want, what, bits=None, top_down=None, taken=True):
    img, probe, lay = read_all_three(tmp_path, data)
    assert img is not None and probe is not None and lay is not None, what
    assert img.dtype == np.uint8 and np.array_equal(img, want), what
    h, w = want.shape
    assert probe == (h, w, 8, 5), what
    assert (lay.height, lay.width, lay.taken) == (h, w, taken), what
    assert lay.row_bytes == bc.row_bytes(w, lay.bits)
    if bits is not None:
        assert lay.bits == bits, what
    if top_down is not None:
        assert lay.top_down == int(top_down), what
    return lay


def palette_for(bits, seed):
    return bc.random_palette(1 << bits, seed)


@pytest.mark.parametrize("bits", [1, 4, 8, 24, 32])
def test_every_width_height_and_row_order(tmp_path, bits):
    for k, (w, h, top_down) in enumerate(itertools.product(WIDTHS, HEIGHTS, (False, True))):
        pix = bc.random_pixels(w, h, bits, seed=1000 * bits + k)
        pal = palette_for(bits, k) if bits <= 8 else None
        lay = assert_reads_to(tmp_path, bc.write(pix, bits, pal, top_down=top_down), bc.expected(pix, bits, pal),
                              (bits, w, h, top_down), bits=bits, top_down=top_down)
        assert lay.compression == 0 and lay.payload_offset == 14 + 40 + (4 << bits if bits <= 8 else 0)
        if bits <= 8:
            assert np.array_equal(lay.lut[:1 << bits], bc.grey(pal[:, 0], pal[:, 1], pal[:, 2])) and not lay.lut[1 << bits:].any()


@pytest.mark.parametrize("header", [40, 52, 56, 108, 124])
@pytest.mark.parametrize("bits", [1, 4, 8, 24, 32])
def test_header_sizes(tmp_path, header, bits):
    pix = bc.random_pixels(17, 5, bits, seed=header + bits)
    pal = palette_for(bits, header) if bits <= 8 else None
    lay = assert_reads_to(tmp_path, bc.write(pix, bits, pal, header=header, gap=3 if header == 108 else 0), bc.expected(pix, bits, pal),
                          (header, bits))
    assert lay.payload_offset == 14 + header + (4 << bits if bits <= 8 else 0) + (3 if header == 108 else 0)


@pytest.mark.parametrize("header,top_down", [(40, False), (40, True), (52, False), (56, True), (108, False), (124, True)])
def test_bitfields_with_the_one_set_of_masks(tmp_path, header, top_down):
    """the masks behind a 40-byte header (the pixel array begins 12 bytes later), inside a longer one"""
    pix = bc.random_pixels(9, 5, 32, seed=header)
    lay = assert_reads_to(tmp_path, bc.write(pix, 32, header=header, bitfields=True, top_down=top_down), bc.expected(pix, 32),
                          (header, top_down), bits=32, top_down=top_down)
    assert lay.compression == 3 and lay.payload_offset == 14 + header + (12 if header == 40 else 0)


@pytest.mark.parametrize("bits,used", [(1, 0), (1, 2), (4, 0), (4, 2), (4, 16), (8, 0), (8, 2), (8, 16), (8, 200)])
def test_clr_used_and_an_index_beyond_a_short_palette(tmp_path, bits, used):
    n = used or 1 << bits
    pal = bc.random_palette(n, seed=used + bits)
    pix = bc.random_pixels(33, 5, bits, seed=used)            # (indices up to 2^bits - 1: some lie beyond a short palette)
    if n < 1 << bits:
        pix[0, 0], pix[-1, -1] = n, (1 << bits) - 1
    want = bc.expected(pix, bits, pal)
    assert n == 1 << bits or (want[0, 0] == 0 and want[-1, -1] == 0)
    lay = assert_reads_to(tmp_path, bc.write(pix, bits, pal, clr_used=used), want, (bits, used))
    assert not lay.lut[n:].any()


def test_the_identity_flag_is_the_grey_ramp(tmp_path):
    pix = bc.random_pixels(31, 2, 8, seed=1)
    lay = assert_reads_to(tmp_path, bc.write(pix, 8, bc.grey_ramp()), pix, "ramp")
    assert lay.lut_identity == 1 and np.array_equal(lay.lut, np.arange(256))
    pal = bc.grey_ramp()
    pal[200] = (200, 201, 200)                              # its grey is 201
    assert bc.grey(200, 201, 200) == 201
    lay = assert_reads_to(tmp_path, bc.write(pix, 8, pal), bc.expected(pix, 8, pal), "almost a ramp")
    assert lay.lut_identity == 0
    # a short ramp leaves indices the depth can produce undefined: not the identity
    lay = assert_reads_to(tmp_path, bc.write(np.minimum(pix, 199), 8, bc.grey_ramp(200)), np.minimum(pix, 199), "short ramp")
    assert lay.lut_identity == 0
    # at 4 bits: the first sixteen entries decide
    pix4 = bc.random_pixels(9, 2, 4, seed=2)
    assert assert_reads_to(tmp_path, bc.write(pix4, 4, bc.grey_ramp(16)), pix4, "ramp of 16").lut_identity == 1


def test_grey_palette_entries_are_exact():
    """the weights sum to 2^14: a grey entry (v, v, v) reads v"""
    v = np.arange(256)
    assert np.array_equal(bc.grey(v, v, v), v) and 4899 + 9617 + 1868 == 1 << 14


def test_rle8_with_every_escape(tmp_path):
    w, h, stream, idx = bc.rle8_every_escape()
    pal = bc.random_palette(256, seed=9)
    lay = assert_reads_to(tmp_path, bc.write_rle8(w, h, stream, pal), bc.expected(idx, 8, pal), "escapes", bits=8, taken=False)
    assert lay.compression == 1 and lay.rc == mrgingham_amd.BMP_NOT_TAKEN and (idx == 0).sum() > w
    # the plain encoder's stream of a whole image, with a header of 124 bytes; and cut inside its last row, which is begun
    pix = bc.random_pixels(33, 9, 8, seed=10)
    pix[3, 5:20] = 77
    stream = bc.rle8_encode(pix)
    assert_reads_to(tmp_path, bc.write_rle8(33, 9, stream, pal, header=124), bc.expected(pix, 8, pal), "plain", taken=False)
    cut = np.array(pix)
    cut[0, 20:] = 0
    assert_reads_to(tmp_path, bc.write_rle8(33, 9, bc.rle8_encode(pix[1:])[:-2] + bc.rle8_encode(pix[:1, :20])[:-4], pal),
                    bc.expected(cut, 8, pal), "cut in the last row", taken=False)


def test_a_file_longer_than_the_probe_reads(tmp_path):
    """probe_image looks at the first 4096 bytes and the file's size: a payload one byte short is seen from the size alone;
    the stream of a long RLE8 file is walked to its end"""
    pix = bc.random_pixels(130, 65, 8, seed=12)
    pal = bc.random_palette(256, seed=13)
    data = bc.write(pix, 8, pal)
    assert len(data) > 2 * 4096
    assert_reads_to(tmp_path, data, bc.expected(pix, 8, pal), "long")
    assert read_all_three(tmp_path, data[:-1]) == (None, None, None)
    stream = bc.rle8_encode(pix)
    assert len(stream) > 2 * 4096
    assert_reads_to(tmp_path, bc.write_rle8(130, 65, stream, pal), bc.expected(pix, 8, pal), "long stream", taken=False)
    assert read_all_three(tmp_path, bc.write_rle8(130, 65, stream[:-2 - 2 * 200], pal)) == (None, None, None)      # cut rows below the top


def test_writer_agrees_with_pillow(tmp_path):
    """Pillow decodes the writer's files to the same samples.  Left out: the index beyond a short palette (Pillow has its
    own idea of an undefined entry) and what Pillow does not read -- the 52- and 56-byte headers, and 32 bits with masks
    behind a 40-byte header where it keeps the fourth byte as alpha (convert("RGB") drops it)."""
    Image = pytest.importorskip("PIL.Image")
    seen = 0
    for bits, header, top_down in itertools.product((1, 4, 8, 24, 32), (40, 108, 124), (False, True)):
        for w, h in ((1, 1), (7, 2), (17, 5), (33, 5), (65, 2)):
            pix = bc.random_pixels(w, h, bits, seed=bits + w)
            pal = palette_for(bits, w) if bits <= 8 else None
            data = bc.write(pix, bits, pal, header=header, top_down=top_down)
            rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
            want = pal[pix] if bits <= 8 else pix[..., :3]
            assert np.array_equal(rgb, want), (bits, header, top_down, w, h)
            img, _, _ = read_all_three(tmp_path, data)
            assert np.array_equal(img, bc.grey(rgb[..., 0], rgb[..., 1], rgb[..., 2]))
            seen += 1
    # RLE8: Pillow passes over an end of line in an empty row and fills a row up at an end of line only, so the stream of
    # rle8_every_escape is left out; this one has the odd absolute run, the end of line in mid-row, the delta across a
    # row and unwritten pixels in a form both readers take
    pal = bc.random_palette(256, seed=9)
    stream = bytes([4, 7, 0, 3, 11, 12, 13, 0xAA, 0, 0]) + bytes([0, 2, 2, 1, 5, 200, 0, 0]) + bytes([0, 1])
    idx = np.zeros((3, 9), np.uint8)
    idx[2, :7] = [7, 7, 7, 7, 11, 12, 13]
    idx[0, 2:7] = 200
    data = bc.write_rle8(9, 3, stream, pal)
    rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert np.array_equal(rgb, pal[idx])
    assert np.array_equal(read_all_three(tmp_path, data)[0], bc.expected(idx, 8, pal))
    assert seen == 150


def test_pillow_written_files_read_to_their_arrays(tmp_path):
    cases = list(golden())
    assert len(cases) == 10 and {n.split("_")[0] for n, _, _ in cases} == {"1", "L", "P", "RGB", "RGBA"}
    for name, data, want in cases:
        lay = assert_reads_to(tmp_path, data, want, name)
        assert lay.lut_identity == int(name.startswith("L_")), name


def test_broken_files_are_unreadable_by_all_three(tmp_path):
    broken, good = bc.broken_files()
    assert read_all_three(tmp_path, good)[0] is not None
    assert len(broken) >= 35
    for name, data in broken.items():
        assert read_all_three(tmp_path, data) == (None, None, None), name


def test_files_ex4_takes_the_bmp_flag_and_files_ex3_goes_on_refusing_it():
    """With no files the call returns before it needs a device: flags 0 .. 31 are fine for _ex4 (Deflate only with TIFF), 32
    is not; _ex3 refuses 16."""
    import ctypes
    from mrgingham_amd import _lib
    L = _lib.lib()
    o = _lib.FilesOptions(1, 1, 10, -1, 1, 0, 0, 0, -1)
    cb = _lib.PROGRESS_F(lambda n, cookie: None)
    for flags in range(64):
        want = 0 if flags < 32 and not (flags & 8 and not flags & 4) else -1
        assert L.mrgingham_amd_find_boards_files_ex4(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, flags) == want, flags
    for flags in (16, 17, 20, 31):
        assert L.mrgingham_amd_find_boards_files_ex3(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, flags) == -1
    assert L.mrgingham_amd_find_boards_files_ex3(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, 15) == 0
    with pytest.raises(ValueError):
        mrgingham_amd.find_boards_files([], bmp="both")


def corpus():
    """Good files, broken files and seeded byte mutations of both."""
    items = [d for _, d, _ in golden()]
    for k, (bits, header) in enumerate(itertools.product((1, 4, 8, 24, 32), (40, 108))):
        pix = bc.random_pixels(17 + k, 3, bits, seed=k)
        items.append(bc.write(pix, bits, palette_for(bits, k) if bits <= 8 else None, header=header, top_down=bool(k & 1)))
    items.append(bc.write(bc.random_pixels(9, 3, 32, seed=1), 32, bitfields=True))
    w, h, stream, _ = bc.rle8_every_escape()
    items.append(bc.write_rle8(w, h, stream, bc.random_palette(256, seed=9)))
    broken, good = bc.broken_files()
    items += [good] + list(broken.values())
    rng = np.random.default_rng(17)
    mutated = []
    for data in items:
        for _ in range(40):
            b = bytearray(data)
            for _ in range(int(rng.integers(1, 4))):
                # (mostly in the headers, where every byte is a rule)
                at = int(rng.integers(0, min(len(b), 70))) if rng.integers(0, 4) else int(rng.integers(0, len(b)))
                b[at] = int(rng.integers(0, 256))
            mutated.append(bytes(b))
        mutated.append(data[:int(rng.integers(1, len(data)))])
    return items + mutated


def test_corpus_and_pixel_text_under_address_and_undefined_sanitizers(tmp_path):
    """The corpus through the host readers (tests/host_program.py) built with -fsanitize=address,undefined into a stand-alone program
    (tests/boundary/bmp_fuzz_main.cpp), run as a child process: read_image, probe_image and bmp_layout on every case, and
    bmp_pixels.h on source rows held in buffers of exactly the padded row length."""
    exe = build_sanitized(tmp_path, "bmp_fuzz_main.cpp")
    items = corpus()
    assert len(items) > 2000
    blob = tmp_path / "corpus.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for data in items:
            f.write(struct.pack("<I", len(data)) + data)
    scratch = tmp_path / "scratch.bmp"
    want_layouts = sum(mrgingham_amd.bmp_layout(d) is not None for d in items)
    r = subprocess.run([exe, str(blob), str(scratch)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    words = r.stdout.split()
    assert words[:4] == ["cases", str(len(items)), "readable", str(want_layouts)], r.stdout
    assert want_layouts > 200 and int(words[5]) > 1000         # (rows walked through the pixel text, at sixteen phases each)
