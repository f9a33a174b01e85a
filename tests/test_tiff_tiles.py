"""Tiled TIFF on the host (read_image, probe_image, tiff_layout(tiles=True); csrc/image_io.cpp), no GPU: files written by the
tiled writer of tests/tiff_tile_cases.py against the arrays they were written from, the tile records against what the writer
laid out, the return code (0: the device route takes the file) against the stated rules, one broken rule per file, the
writer against Pillow's libtiff, and the corpus with truncations and directory mutations through a stand-alone program
under the address and undefined-behaviour sanitizers."""
import io
import struct
import subprocess

import numpy as np
import pytest

import mrgingham_amd
from tests import tiff_cases as tc
from tests import tiff_tile_cases as tt
from tests.host_program import build_sanitized

CODECS = (tt.NONE, tt.LZW, tt.PACKBITS, tt.ADOBE_DEFLATE, tt.DEFLATE)


def _read(tmp_path, data, name="case.tif"):
    p = tmp_path / name
    p.write_bytes(data)
    return mrgingham_amd.read_image(str(p)), mrgingham_amd.probe_image(str(p))


def _as_read_image(grey):
    return grey if grey.dtype == np.uint8 else (grey >> 8).astype(np.uint8)


def grid():
    """(label, tw, tl, keyword arguments of tt.encode, image): every codec at both depths and byte orders with and without
    the predictor, tw in {16, 20, 48, 272}, 1 to 4 samples, WhiteIsZero, reverse order, odd offsets."""
    out, n = [], 0
    tiles = [(16, 16), (20, 12), (48, 24), (272, 16)]
    for bits in (8, 16):
        for comp in CODECS:
            for pred in (1, 2):
                for order in "<>":
                    tw, tl = tiles[n % 4]
                    samples = (1, 3, 2, 4, 1)[n % 5]
                    kw = dict(order=order, compression=comp, predictor=pred, reverse=n % 3 == 1, odd=n % 5 < 2, seed=n)
                    if samples <= 2 and n % 4 == 2:
                        kw["photometric"] = 0
                    if samples >= 3 and n % 6 == 5:
                        kw["photometric"] = 1
                    out.append((f"b{bits}_c{comp}_p{pred}_{order}_{tw}x{tl}_s{samples}_{n}", tw, tl, kw, tc.random_image(37, 29, samples, bits, seed=n)))
                    n += 1
    return out


def sizes():
    """(w, h, tw, tl): w < tw, h < tl, and exact multiples of the tile and one more or less."""
    out = [(5, 3, 16, 16), (1, 1, 16, 16), (7, 40, 20, 12), (40, 7, 48, 24)]
    for tw, tl in ((16, 16), (20, 12), (48, 24)):
        for dw in (-1, 0, 1):
            for dh in (-1, 0, 1):
                out.append((2 * tw + dw, 2 * tl + dh, tw, tl))
    out += [(271, 5, 272, 16), (272, 16, 272, 16), (273, 17, 272, 16)]
    return out


def test_writer_grid_reads_back(tmp_path):
    """The array handed to the writer is the yardstick; the padding of the edge tiles is random and must not show."""
    seen = set()
    for label, tw, tl, kw, img in grid():
        data, recs = tt.encode(img, tw, tl, **kw)
        got, probe = _read(tmp_path, data)
        assert probe == (29, 37, 8 * img.dtype.itemsize, 4), label
        assert got is not None and np.array_equal(got, _as_read_image(tc.grey_of(img, tt.photometric_of(kw, img)))), label
        seen.add((img.dtype.itemsize, kw["compression"], kw["predictor"], kw["order"]))
    assert len(seen) == 2 * len(CODECS) * 2 * 2


def test_every_size_against_the_tile_reads_back(tmp_path):
    n = 0
    for w, h, tw, tl in sizes():
        for comp, pred, bits, samples in ((tt.NONE, 2, 8, 1), (tt.LZW, 2, 16, 3), (tt.ADOBE_DEFLATE, 1, 8, 3), (tt.PACKBITS, 2, 16, 1)):
            img = tc.random_image(w, h, samples, bits, seed=n)
            data, recs = tt.encode(img, tw, tl, order="<>"[n % 2], compression=comp, predictor=pred, odd=n % 2 == 0, seed=n)
            got, probe = _read(tmp_path, data)
            label = (w, h, tw, tl, comp, pred, bits, samples)
            assert probe == (h, w, bits, 4), label
            assert got is not None and np.array_equal(got, _as_read_image(tc.grey_of(img, 2 if samples == 3 else 1))), label
            lay = mrgingham_amd.tiff_layout(data, tiles=True)
            assert lay is not None and lay.nstrips == len(recs) == (-(-w // tw)) * (-(-h // tl)), label
            n += 1


def test_sixteen_bit_samples_come_out_native_through_the_c_reader(tmp_path):
    img = tc.random_image(37, 29, 1, 16, seed=9)
    for order in "<>":
        p = tmp_path / f"deep{ord(order)}.tif"
        p.write_bytes(tt.encode(img, 20, 12, order=order, compression=tt.LZW, predictor=2)[0])
        got = mrgingham_amd.read_image(str(p), cli_scaling=True)
        want = np.clip(np.rint(img.astype(np.float64) * (255. / 65535.)), 0, 255).astype(np.uint8)
        assert np.array_equal(got, want)


def test_the_literal_lzw_stream_of_the_large_gpu_shapes_reads_back(tmp_path):
    """tt.lzw_literal: a ClearCode in front of every 250 codes of 9 bits -- read by this library and by libtiff alike."""
    img = tc.random_image(300, 29, 3, 8, seed=3)
    data = tt.encode(img, 272, 16, compression=tt.LZW, predictor=2, literal_lzw=True)[0]
    got, probe = _read(tmp_path, data)
    assert probe == (29, 300, 8, 4) and np.array_equal(got, tc.grey_of(img, 2))
    Image = pytest.importorskip("PIL.Image", reason="Pillow is the independent decoder this test compares the writer with")
    from PIL import features
    if not features.check("libtiff"):
        pytest.skip("Pillow without libtiff reads no LZW")
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img)


def test_layout_returns_the_tile_records_and_the_route_verdict():
    for label, tw, tl, kw, img in grid():
        data, recs = tt.encode(img, tw, tl, **kw)
        samples = 1 if img.ndim == 2 else img.shape[2]
        # without tiles=True the file stays unreadable to the strip parsers
        assert mrgingham_amd.tiff_layout(data) is None and mrgingham_amd.tiff_layout(data, deflate_max_strip=1 << 20) is None, label
        for lzw_max, deflate_max in ((0, 0), (0, 1 << 20), (1000, 1000)):
            lay = mrgingham_amd.tiff_layout(data, lzw_max_strip=lzw_max, deflate_max_strip=deflate_max, tiles=True)
            assert lay is not None, label
            assert (lay.tile_width, lay.tile_length) == (tw, tl), label
            assert [tuple(int(v) for v in r) for r in lay.strips] == recs and lay.nstrips == len(recs), label
            assert lay.key() == (37, 29, 8 * img.dtype.itemsize, samples, tt.photometric_of(kw, img), kw["compression"], kw["predictor"],
                                 int(kw["order"] == ">")), label
            want = tt.taken(tw, tl, img, kw["compression"], lzw_max, deflate_max)
            assert lay.taken == want and lay.rc == (0 if want else mrgingham_amd.TIFF_NOT_TAKEN), (label, lzw_max, deflate_max)
    img = tc.random_image(100, 40, 1, 8, seed=1)
    data, recs = tt.encode(img, 48, 24, compression=tt.LZW, reverse=True, odd=True)
    lay = mrgingham_amd.tiff_layout(data, tiles=True)
    assert [tuple(int(v) for v in r) for r in lay.strips] == recs and len(recs) == 6
    assert all(o % 2 == 1 for o, _, _, _ in recs) and recs[0][0] > recs[-1][0]
    assert [r[2] for r in recs] == [0, 0, 0, 24, 24, 24] and all(r[3] == 24 for r in recs)
    # the limit is on a TILE's decoded bytes, 48 x 24
    assert mrgingham_amd.tiff_layout(data, lzw_max_strip=48 * 24, tiles=True).taken
    small = mrgingham_amd.tiff_layout(data, lzw_max_strip=48 * 24 - 1, tiles=True)
    assert small.rc == mrgingham_amd.TIFF_NOT_TAKEN and small.nstrips == 6 and small.tile_width == 48
    short = mrgingham_amd.tiff_layout(data, capacity=5, tiles=True)
    assert short.rc == -2 and short.nstrips == 6 and len(short.strips) == 5 and (short.tile_width, short.tile_length) == (48, 24)
    # a Deflate tile of more bytes than any zlib stream of it needs keeps the host decoder
    rows = tc.strip_rows(tt.tile_array(img, 0, 0, 48, 24, np.random.default_rng(0)), 0, 24, "<", 1, 1).tobytes()
    fat = tt.encode(img, 48, 24, compression=tt.ADOBE_DEFLATE, tile_bytes={0: zlib_stored(rows) + bytes(48 * 24 // 8 + 600)})[0]
    assert mrgingham_amd.tiff_layout(fat, deflate_max_strip=1 << 20, tiles=True).rc == mrgingham_amd.TIFF_NOT_TAKEN
    # a strip file through the tiled parser: exactly tiff_layout, tile sizes 0
    sdata, strips = tc.encode(img, compression=tc.LZW, rows_per_strip=7)
    a, b = mrgingham_amd.tiff_layout(sdata), mrgingham_amd.tiff_layout(sdata, tiles=True)
    assert (b.tile_width, b.tile_length) == (0, 0) and a.key() == b.key() and a.rc == b.rc == 0 and np.array_equal(a.strips, b.strips)
    # RowsPerStrip in a tiled file is ignored
    data, recs = tt.encode(img, 48, 24, tags={278: (tc.LONG, [5])})
    assert [tuple(int(v) for v in r) for r in mrgingham_amd.tiff_layout(data, tiles=True).strips] == recs


def zlib_stored(raw):
    import zlib
    c = zlib.compressobj(0)
    return c.compress(raw) + c.flush()


def test_every_broken_tiled_file_is_unreadable(tmp_path):
    broken, good, img = tt.broken_files()
    got, probe = _read(tmp_path, good)
    assert np.array_equal(got, img) and probe == (29, 37, 8, 4)
    assert len(broken) == 17
    for name, (data, in_header) in broken.items():
        got, probe = _read(tmp_path, data, name + ".tif")
        assert got is None, name
        lay = mrgingham_amd.tiff_layout(data, tiles=True, deflate_max_strip=1 << 20)
        if in_header:
            assert probe is None and lay is None, name
        else:
            assert probe is not None and lay is not None, name
    # the mixture test_tiff_io.py pins (322 and 323 beside strip tags) stays unreadable to the tiled parser too
    mixed = tc.broken_files()[0]["tiles"][0]
    assert mrgingham_amd.tiff_layout(mixed, tiles=True) is None and _read(tmp_path, mixed) == (None, None)


def test_pillow_decodes_the_tiled_writers_files_to_the_same_arrays():
    """Pillow's libtiff must decode the writer's file to the array handed to the writer, so that writer and reader cannot
    share one misreading -- tile widths that are no multiple of 16 included, which libtiff reads.  The modes Pillow lacks
    and predictor 2 outside LZW / Deflate are left out, as in test_tiff_io.py."""
    Image = pytest.importorskip("PIL.Image", reason="Pillow is the independent decoder this test compares the writer with")
    from PIL import features
    if not features.check("libtiff"):
        pytest.skip("Pillow without libtiff reads no compressed or tiled TIFF")
    compared = []
    cases = [(tw, tl, kw, img) for _, tw, tl, kw, img in grid()]
    n = 100
    for tw, tl in ((20, 12), (16, 16), (272, 16), (1040, 16)):
        for comp in (tt.NONE, tt.LZW, tt.ADOBE_DEFLATE):
            cases.append((tw, tl, dict(order="<>"[n % 2], compression=comp, predictor=2 if comp != tt.NONE else 1, seed=n),
                          tc.random_image(37, 29, 1, (8, 16)[n % 2], seed=n)))
            n += 1
    for tw, tl, kw, img in cases:
        photo = tt.photometric_of(kw, img)
        samples = 1 if img.ndim == 2 else img.shape[2]
        pil_has = (samples == 1 and not (photo == 0 and img.dtype == np.uint16)) or (img.dtype == np.uint8 and samples in (3, 4) and photo == 2)
        if pil_has and (kw["predictor"] == 1 or kw["compression"] in (tt.LZW, tt.ADOBE_DEFLATE, tt.DEFLATE)):
            back = np.asarray(Image.open(io.BytesIO(tt.encode(img, tw, tl, **kw)[0])))
            assert back.shape == img.shape and np.array_equal(back, img), (tw, tl, kw)
            compared.append((img.dtype.itemsize, samples, kw["compression"], kw["predictor"], kw["order"], tw))
    assert {c[0] for c in compared} == {1, 2} and {c[4] for c in compared} == {"<", ">"}
    assert {c[2] for c in compared} == set(CODECS) and {c[5] for c in compared} >= {16, 20, 48, 272, 1040}
    assert any(c[2] == tt.LZW and c[3] == 2 for c in compared) and any(c[2] == tt.ADOBE_DEFLATE and c[3] == 2 for c in compared)


def corpus():
    """Good and broken tiled files, every truncation of two good files, and seeded mutations of their directories."""
    items = [tt.encode(img, tw, tl, **kw)[0] for _, tw, tl, kw, img in grid()[::3]]
    broken, good, img = tt.broken_files()
    items += [good] + [d for d, _ in broken.values()]
    small = tc.random_image(21, 18, 1, 8, seed=31)
    two = [tt.encode(small, 16, 16, compression=tt.LZW, predictor=2)[0], tt.encode(small, 20, 12, order=">", compression=tt.PACKBITS)[0]]
    items += [d[:k] for d in two for k in range(len(d))]
    rng = np.random.default_rng(12)
    for d in two:
        ifd = struct.unpack("<>"[d[:2] == b"MM"] + "I", d[4:8])[0]
        # the directory, the values behind the header's offsets, and the 8 bytes of the header
        lo = min(ifd, len(d) - 200)
        for _ in range(2000):
            b = bytearray(d)
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(lo, len(b))) if rng.integers(0, 8) else int(rng.integers(0, 8))
                b[at] = int(rng.integers(0, 256))
            items.append(bytes(b))
    return items


def test_corpus_under_address_and_undefined_sanitizers(tmp_path):
    """The corpus through the host readers (tests/host_program.py) built with -fsanitize=address,undefined into a stand-alone program
    (tests/boundary/tiff_tiles_fuzz_main.cpp), run as a child process: tiff_layout_tiled, probe_image and read_image on
    buffers of exact size.  It must not crash, and probe and read agree with the parser at header level."""
    exe = build_sanitized(tmp_path, "tiff_tiles_fuzz_main.cpp")
    items = corpus()
    assert len(items) > 4000
    blob = tmp_path / "corpus.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for data in items:
            f.write(struct.pack("<I", len(data)) + data)
    scratch = tmp_path / "scratch.tif"
    lays = [mrgingham_amd.tiff_layout(d, tiles=True) for d in items]
    want_layouts = sum(l is not None for l in lays)
    want_tiled = sum(l is not None and l.tile_width > 0 for l in lays)
    want_readable = 0
    for d in items:
        scratch.write_bytes(d)
        want_readable += mrgingham_amd.read_image(str(scratch)) is not None
    r = subprocess.run([exe, str(blob), str(scratch)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    assert r.stdout.split() == ["cases", str(len(items)), "layouts", str(want_layouts), "tiled", str(want_tiled), "readable", str(want_readable)], r.stdout
    assert want_tiled > 100 and want_readable > 50
