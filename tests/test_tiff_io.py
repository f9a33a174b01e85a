"""The host TIFF reader (read_image, probe_image, tiff_layout; csrc/image_io.cpp, csrc/tiff_lzw.h), no GPU: files written by
Pillow's libtiff (tests/golden/tiff_golden.npz) and by the writer of tests/tiff_cases.py against the arrays they were
written from, the strip tables against what the writer laid out, one broken rule per file, and the whole corpus through a
stand-alone program under the address and undefined-behaviour sanitizers."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import mrgingham_amd
from tests import tiff_cases as tc
from tests.host_program import build_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff_golden.npz")


def _read(tmp_path, data, name="case.tif"):
    p = tmp_path / name
    p.write_bytes(data)
    return mrgingham_amd.read_image(str(p)), mrgingham_amd.probe_image(str(p))


def _as_read_image(grey):
    """read_image gives 8 bit: the high byte of a 16-bit sample."""
    return grey if grey.dtype == np.uint8 else (grey >> 8).astype(np.uint8)


def golden():
    g = np.load(GOLDEN)
    return [(str(n), g[f"tif_{i}"].tobytes(), g[f"img_{i}"]) for i, n in enumerate(g["name"])]


def grid():
    """The writer's parameter grid: (label, keyword arguments of tc.encode, image)."""
    out, n = [], 0
    for bits in (8, 16):
        for samples in (1, 2, 3, 4):
            for comp in (tc.NONE, tc.LZW, tc.PACKBITS, tc.ADOBE_DEFLATE, tc.DEFLATE):
                for pred in (1, 2):
                    order = "<>"[n % 2]
                    rps = [None, 3, 1, 40][n % 4]
                    kw = dict(order=order, compression=comp, predictor=pred, rows_per_strip=rps, reverse=n % 3 == 1, odd=n % 5 < 2)
                    if n % 7 == 3:
                        kw.update(rows_per_strip=None, rps_tag=[2 ** 32 - 1, 1000][n % 2])
                    if samples <= 2 and n % 4 == 2:
                        kw["photometric"] = 0
                    if samples >= 3 and n % 6 == 5:
                        kw["photometric"] = 1      # grey with extra samples
                    img = tc.random_image(37, 11, samples, bits, seed=n)
                    out.append((f"b{bits}_s{samples}_c{comp}_p{pred}_{n}", kw, img))
                    n += 1
    return out


def test_golden_files_from_libtiff_read_as_pillow_reads_them(tmp_path):
    cases = golden()
    assert len(cases) >= 20
    for name, data, img in cases:
        got, probe = _read(tmp_path, data)
        want = tc.grey_of(img, 2 if img.ndim == 3 else 1)
        assert probe == (img.shape[0], img.shape[1], 8 * img.dtype.itemsize, 4), name
        assert got is not None and np.array_equal(got, _as_read_image(want)), name
        lay = mrgingham_amd.tiff_layout(data)
        assert lay is not None and (lay.height, lay.width) == img.shape[:2], name
        # the device route takes what is uncompressed or LZW; PackBits and Deflate are the host decoder's
        assert lay.taken == (lay.compression in (1, 5)) and lay.rc == (0 if lay.taken else mrgingham_amd.TIFF_NOT_TAKEN), name
        if "rps4" in name:
            assert lay.predictor == 2 and lay.nstrips == (img.shape[0] + 3) // 4 and int(lay.strips["rows"][0]) == 4, name


def _photometric_of(kw, img):
    return kw.get("photometric", 2 if img.ndim == 3 and img.shape[2] >= 3 else 1)


def test_writer_grid_reads_back(tmp_path):
    """TIFF here is lossless: the array handed to the writer is the yardstick, grey by the library's one set of weights."""
    for label, kw, img in grid():
        data, strips = tc.encode(img, **kw)
        got, probe = _read(tmp_path, data)
        assert probe == (11, 37, 8 * img.dtype.itemsize, 4), label
        assert got is not None and np.array_equal(got, _as_read_image(tc.grey_of(img, _photometric_of(kw, img)))), label


def test_pillow_decodes_the_writers_files_to_the_same_arrays():
    """Where Pillow has the mode (L, I;16, 8-bit RGB / RGBA) it must decode the writer's file to the array handed to the
    writer, so that writer and reader cannot share one misreading.  Pillow reads neither 16-bit RGB nor grey + alpha as
    written here, and hands out 16-bit WhiteIsZero samples as they are stored: those rest on test_writer_grid_reads_back
    alone.  libtiff undoes predictor 2 only under LZW and Deflate (its other codecs ignore the tag); this library follows
    the TIFF 6.0 text and undoes it under every compression, so predictor 2 without LZW / Deflate is left out here."""
    Image = pytest.importorskip("PIL.Image", reason="Pillow is the independent decoder this test compares the writer with")
    compared = []
    for label, kw, img in grid():
        photo = _photometric_of(kw, img)
        samples = 1 if img.ndim == 2 else img.shape[2]
        pil_has = (samples == 1 and not (photo == 0 and img.dtype == np.uint16)) or (img.dtype == np.uint8 and samples in (3, 4) and photo == 2)
        if pil_has and (kw["predictor"] == 1 or kw["compression"] in (tc.LZW, tc.ADOBE_DEFLATE, tc.DEFLATE)):
            back = np.asarray(Image.open(io.BytesIO(tc.encode(img, **kw)[0])))
            assert back.shape == img.shape and np.array_equal(back, img), label
            compared.append((img.dtype.itemsize, samples, kw["compression"], kw["predictor"], kw["order"]))
    # every depth, both byte orders, every compression and LZW with predictor 2 came up
    assert {c[0] for c in compared} == {1, 2} and {c[4] for c in compared} == {"<", ">"}
    assert {c[2] for c in compared} == {tc.NONE, tc.LZW, tc.PACKBITS, tc.ADOBE_DEFLATE, tc.DEFLATE}
    assert any(c[2] == tc.LZW and c[3] == 2 for c in compared) and any(c[1] in (3, 4) for c in compared)


def test_sixteen_bit_samples_come_out_native_through_the_c_reader(tmp_path):
    """px16 behind mrgingham_amd_read_image: cli_scaling converts with 255/65535, which tells the samples' order."""
    img = tc.random_image(19, 5, 1, 16, seed=9)
    for order in "<>":
        p = tmp_path / f"deep{ord(order)}.tif"
        p.write_bytes(tc.encode(img, order=order, compression=tc.LZW, predictor=2)[0])
        got = mrgingham_amd.read_image(str(p), cli_scaling=True)
        want = np.clip(np.rint(img.astype(np.float64) * (255. / 65535.)), 0, 255).astype(np.uint8)
        assert np.array_equal(got, want)


def test_layout_returns_the_strip_tables_the_writer_laid_out():
    for label, kw, img in grid():
        data, strips = tc.encode(img, **kw)
        lay = mrgingham_amd.tiff_layout(data)
        assert lay is not None, label
        assert [tuple(int(v) for v in r) for r in lay.strips] == strips, label
        assert lay.nstrips == len(strips) and lay.key() == (37, 11, 8 * img.dtype.itemsize, 1 if img.ndim == 2 else img.shape[2],
                                                            kw.get("photometric", 2 if img.ndim == 3 and img.shape[2] >= 3 else 1),
                                                            kw["compression"], kw["predictor"], int(kw["order"] == ">")), label
        assert lay.taken == (kw["compression"] in (tc.NONE, tc.LZW)), label
    # strips in reverse file order and at odd offsets
    img = tc.random_image(33, 20, 1, 8, seed=1)
    data, strips = tc.encode(img, compression=tc.LZW, rows_per_strip=3, reverse=True, odd=True)
    lay = mrgingham_amd.tiff_layout(data)
    assert [tuple(int(v) for v in r) for r in lay.strips] == strips and len(strips) == 7 and strips[-1][3] == 2
    assert all(o % 2 == 1 for o, _, _, _ in strips) and strips[0][0] > strips[-1][0]
    # a strip above tiff_lzw_max_strip is the host decoder's; the sizes are still reported
    small = mrgingham_amd.tiff_layout(data, lzw_max_strip=3 * 33 - 1)
    assert small.rc == mrgingham_amd.TIFF_NOT_TAKEN and not small.taken and small.nstrips == 7 and small.width == 33
    assert mrgingham_amd.tiff_layout(data, lzw_max_strip=3 * 33).taken
    # capacity too small: -2 with the counts
    short = mrgingham_amd.tiff_layout(data, capacity=6)
    assert short.rc == -2 and short.nstrips == 7 and len(short.strips) == 6 and (short.height, short.width) == (20, 33)
    assert [tuple(int(v) for v in r) for r in short.strips] == strips[:6]


def test_every_broken_file_is_unreadable(tmp_path):
    """One rule broken per file.  A fault in the directory makes the file unreadable for probe_image and tiff_layout too;
    a fault inside a compressed strip is found by decoding alone -- tiff_layout, which decodes nothing, still reports
    the directory (that is what lets the device meet such a strip: test_gpu_tiff.py)."""
    broken, good, img = tc.broken_files()
    got, probe = _read(tmp_path, good)
    assert np.array_equal(got, img) and probe == (7, 9, 8, 4)
    assert len(broken) == 21
    for name, (data, in_header) in broken.items():
        got, probe = _read(tmp_path, data, name + ".tif")
        assert got is None, name
        lay = mrgingham_amd.tiff_layout(data)
        if in_header:
            assert probe is None and lay is None, name
        else:
            assert probe is not None and lay is not None, name


def test_lzw_streams_the_rules_allow(tmp_path):
    """No ClearCode in front, bytes behind the last needed code, no EOI at all: readable, the same samples."""
    img = tc.noise()
    plain, _ = _read(tmp_path, tc.encode(img, compression=tc.LZW)[0])
    assert np.array_equal(plain, img)
    st = {}
    tc.lzw_encode(img.tobytes(), stats=st)
    assert st["widths"] == [9, 10, 11, 12] and st["clears"] >= 2      # every width, the table filled more than once
    for lzw in (dict(open_with_clear=False), dict(trailing=b"\xff\x00\xaa" * 5)):
        got, _ = _read(tmp_path, tc.encode(img, compression=tc.LZW, lzw=lzw)[0])
        assert np.array_equal(got, img), lzw
    strip = tc.lzw_encode(img.tobytes())
    while True:      # cut the EOI (and only it) off: the last needed code stays whole
        got, _ = _read(tmp_path, tc.encode(img, compression=tc.LZW, strip_bytes=[strip[:-1]])[0])
        if got is None:
            break
        strip = strip[:-1]
        assert np.array_equal(got, img)
    assert len(tc.lzw_encode(img.tobytes())) - len(strip) in (1, 2, 3)
    const = np.full((128, 512), 7, np.uint8)     # every code the not-yet-in-table case
    got, _ = _read(tmp_path, tc.encode(const, compression=tc.LZW)[0])
    assert np.array_equal(got, const)


def test_files_ex2_takes_the_tiff_flag_and_files_ex_goes_on_refusing_it():
    """With no files the call returns before it needs a device: flags 0 .. 7 are fine for _ex2, 8 is not; _ex still
    refuses 4."""
    import ctypes
    from mrgingham_amd import _lib
    L = _lib.lib()
    o = _lib.FilesOptions(1, 1, 10, -1, 1, 0, 0, 0, -1)
    seen = []
    cb = _lib.PROGRESS_F(lambda n, cookie: seen.append(n))
    for flags in range(8):
        assert L.mrgingham_amd_find_boards_files_ex2(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, flags) == 0, flags
    assert seen == [0] * 8
    assert L.mrgingham_amd_find_boards_files_ex2(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, 8) == -1
    for flags in (4, 5, 6, 7):
        assert L.mrgingham_amd_find_boards_files_ex(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, flags) == -1
    assert L.mrgingham_amd_find_boards_files_ex(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, 3) == 0


def corpus():
    """Good files, broken files and seeded byte mutations of both."""
    items = [d for _, d, _ in golden()]
    items += [tc.encode(img, **kw)[0] for _, kw, img in grid()[::3]]
    broken, good, _ = tc.broken_files()
    items += [good] + [d for d, _ in broken.values()]
    rng = np.random.default_rng(11)
    mutated = []
    for data in items:
        for _ in range(6):
            b = bytearray(data)
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            mutated.append(bytes(b))
        mutated.append(data[:int(rng.integers(1, len(data)))])
    return items + mutated


def test_corpus_under_address_and_undefined_sanitizers(tmp_path):
    """The corpus through the host readers (tests/host_program.py) built with -fsanitize=address,undefined into a stand-alone
    program (tests/boundary/tiff_fuzz_main.cpp), run as a child process: read_image, probe_image, tiff_layout and the
    strip decoder of tiff_lzw.h with the host's table and with the kernel's packed one.  The only sanitizer run."""
    exe = build_sanitized(tmp_path, "tiff_fuzz_main.cpp")
    items = corpus()
    blob = tmp_path / "corpus.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for data in items:
            f.write(struct.pack("<I", len(data)) + data)
    scratch = tmp_path / "scratch.tif"
    want_layouts = sum(mrgingham_amd.tiff_layout(d) is not None for d in items)
    want_readable = 0
    for d in items:
        scratch.write_bytes(d)
        want_readable += mrgingham_amd.read_image(str(scratch)) is not None
    r = subprocess.run([exe, str(blob), str(scratch)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    words = r.stdout.split()
    assert words[:6] == ["cases", str(len(items)), "layouts", str(want_layouts), "readable", str(want_readable)], r.stdout
    # the crafted strips went through the shared decoder here: test_gpu_tiff.py hands exactly these to the device
    assert int(words[7]) > 100 and int(words[9]) >= len(tc.broken_lzw_strips())
