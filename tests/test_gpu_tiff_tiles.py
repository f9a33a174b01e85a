"""Tiled TIFF files into device frames (mrgingham_amd_tiff_decode_batch_tiled through Detector.tiff_decode and the C ABI,
Detector.read_tiffs, find_boards_files(tiff="device"), the tool's --tiff-lzw): LZW and Deflate tiles decoded one lane each,
tile rows gathered into image rows with a segmented scan for predictor 2.  The yardstick is the array the test wrote into
the file (tests/tiff_tile_cases.py; TIFF here is lossless, and the writer fills the edge tiles' padding with random non-zero
bytes), byte for byte.  No tolerance anywhere.

The shapes sit on the seams of tiff_finish_tiles_kernel (mrgingham_amd.tiff_geometry: 16 pixels per lane, 1024 per step of a
wave): one lane per tile, lane counts per tile that do not divide 64, a tile straddling a step boundary, tiles of exactly
one step and one pixel more or less of image, tiles longer than one and than two steps."""
import ctypes
import os
import zlib

import numpy as np
import pytest

import mrgingham_amd
from mrgingham_amd import _lib
from tests import tiff_cases as tc
from tests import tiff_tile_cases as tt
from tests.test_gpu_files import parse_vnlog, run_child, run_tool

pytestmark = pytest.mark.gpu

LANES, SEG, STEP = mrgingham_amd.tiff_geometry()
MiB = 1 << 20


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector()
    yield d
    d.close()


def _layouts(datas):
    return [mrgingham_amd.tiff_layout(d, deflate_max_strip=MiB, tiles=True) for d in datas]


# (w, h, tw, tl)
SHAPES = [(5, 3, SEG, 16), (1, 1, SEG, 16),                                   # one partial tile, w < tw, h < tl
          (SEG, 16, SEG, 16), (2 * SEG + 1, 17, SEG, 16), (2 * SEG - 1, 15, SEG, 16),   # one lane per tile
          (100, 40, 3 * SEG, 24),                                                # 3 lanes per tile, partial last column and row
          (STEP + 76, 20, 3 * SEG, 16),                                          # a tile straddling the step boundary (1008 .. 1056)
          (STEP + 76, 9, 17 * SEG, 8),                                           # 17 lanes per tile
          (STEP, 4, STEP, 16), (STEP + 1, 4, STEP, 16), (STEP - 1, 4, STEP, 16),  # a tile of exactly one step
          (2 * STEP + 52, 5, STEP + SEG, 16),                                    # a tile longer than a step
          (2 * STEP + 22, 3, 2 * STEP + SEG, 16)]                                # a tile longer than two steps
EXTRA_SAMPLES = {(100, 40, 3 * SEG, 24), (STEP + 76, 9, 17 * SEG, 8)}            # samples 2 and 4, WhiteIsZero
REAL_LZW_BYTES = 16 << 10


def _run_shape(det, w, h, tw, tl, samples, photo, bits, order, comp, pred, n):
    import torch
    B = 2 if n % 3 == 0 else 1
    # (the Python LZW encoder takes a second per MiB: above 16 KiB of tiles the stream that compresses nothing)
    across, down = -(-w // tw), -(-h // tl)
    literal = across * down * tw * tl * samples * bits // 8 > REAL_LZW_BYTES
    imgs = [tc.random_image(w, h, samples, bits, seed=1000 * n + k) for k in range(B)]
    datas = [tt.encode(img, tw, tl, order=order, compression=comp, predictor=pred, photometric=photo, odd=comp == tt.NONE or n % 2 == 0,
                       reverse=n % 3 == 0, seed=n + k, literal_lzw=literal)[0] for k, img in enumerate(imgs)]
    lays = _layouts(datas)
    label = (w, h, tw, tl, samples, photo, bits, order, comp, pred)
    assert all(l is not None and l.taken and (l.tile_width, l.tile_length) == (tw, tl) for l in lays), label
    if comp == tt.NONE:
        assert all(int(o) % 2 == 1 for l in lays for o in l.strips["offset"]), label
    sentinel = 0xA5 if bits == 8 else 0xA5C3
    big = torch.from_numpy(np.full((B, h + 2, w + 5), sentinel, np.uint8 if bits == 8 else np.uint16)).cuda()
    got, status, tile_status = det.tiff_decode(datas, layouts=lays, out=big[:, :h, :])
    assert status.tolist() == [0] * B and not tile_status.any(), label
    whole = big.cpu().numpy()
    for k in range(B):
        assert np.array_equal(whole[k, :h, :w], tc.grey_of(imgs[k], photo)), label
    assert (whole[:, :h, w:] == sentinel).all() and (whole[:, h:, :] == sentinel).all(), label


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d_in_%dx%d" % s for s in SHAPES])
def test_finish_tiles_kernel(det, shape):
    """Every shape with predictor 1 and 2, LZW / Deflate / uncompressed at odd offsets, 8 bit and 16 bit in both byte orders,
    1 sample and RGB; on two shapes also 2 and 4 samples and WhiteIsZero.  One or two frames a call; out has a wider stride and a
    larger frame pitch, filled with a sentinel that must survive."""
    w, h, tw, tl = shape
    n = 0
    kinds = [(1, 1), (3, 2)]
    if shape in EXTRA_SAMPLES:
        kinds += [(2, 1), (4, 2), (1, 0), (2, 0), (4, 1)]
    for pred in (1, 2):
        for comp in (tt.LZW, tt.ADOBE_DEFLATE, tt.NONE):
            for bits, order in ((8, "<"), (8, ">"), (16, "<"), (16, ">")):
                for samples, photo in kinds:
                    _run_shape(det, w, h, tw, tl, samples, photo, bits, order, tt.DEFLATE if comp == tt.ADOBE_DEFLATE and n % 2 else comp, pred, n)
                    n += 1
    assert n == 2 * 3 * 4 * len(kinds)


def test_the_device_equals_the_host_decoder(det, tmp_path):
    """read_image on the same files: the same bytes (the high byte of 16-bit samples)."""
    n = 0
    for (w, h, tw, tl) in ((100, 40, 3 * SEG, 24), (STEP + 76, 9, 17 * SEG, 8)):
        for bits, comp in ((8, tt.LZW), (16, tt.ADOBE_DEFLATE), (16, tt.NONE)):
            img = tc.random_image(w, h, 3, bits, seed=n)
            data = tt.encode(img, tw, tl, order="<>"[n % 2], compression=comp, predictor=2, seed=n)[0]
            got, status, _ = det.tiff_decode([data], layouts=_layouts([data]))
            p = tmp_path / "host.tif"
            p.write_bytes(data)
            host = mrgingham_amd.read_image(str(p))
            g = got[0].cpu().numpy()
            assert status.tolist() == [0] and np.array_equal(g if bits == 8 else (g >> 8).astype(np.uint8), host), (w, h, bits, comp)
            n += 1


def test_finish_tiles_kernel_takes_a_second_trip_over_the_rows(det):
    """The grid is capped at eight workgroups per CU, four waves each, a row per wave and trip: two frames of 33 x (16 CUs +
    100) rows make one full trip and a ragged second one that begins inside the second frame."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W, H, B = 33, 16 * cus + 100, 2
    assert 8 * cus * 4 < B * H < 2 * 8 * cus * 4
    imgs = [tc.random_image(W, H, 1, 16, seed=70 + k) for k in range(B)]
    datas = [tt.encode(img, 16, 256, order=">", predictor=2, seed=k)[0] for k, img in enumerate(imgs)]
    got, status, _ = det.tiff_decode(datas)
    assert status.tolist() == [0] * B
    for k in range(B):
        assert np.array_equal(got[k].cpu().numpy(), imgs[k]), k


# ---- bad frames -----------------------------------------------------------------------------------------------------------
BW, BH, BTW, BTL = 100, 40, 48, 24


def _four(comp, pred=2, bits=8):
    imgs = [tc.random_image(BW, BH, 1, bits, seed=300 + k) for k in range(4)]
    return imgs, [tt.encode(img, BTW, BTL, compression=comp, predictor=pred, seed=k)[0] for k, img in enumerate(imgs)]


def _check_three_good_one_zero(got, status, imgs, bad):
    assert status.tolist() == [-1 if k == bad else 0 for k in range(4)]
    got = got.cpu().numpy()
    for k in range(4):
        if k == bad:
            assert not got[k].any()
        else:
            assert np.array_equal(got[k], imgs[k]), k


def test_a_cut_lzw_tile_costs_a_status_and_a_zero_frame(det):
    imgs, datas = _four(tt.LZW)
    rows = tc.strip_rows(tt.tile_array(imgs[2], 1, 1, BTW, BTL, np.random.default_rng(0)), 0, BTL, "<", 2, 1)
    cut = tc.lzw_encode(rows.tobytes())
    datas[2] = tt.encode(imgs[2], BTW, BTL, compression=tt.LZW, predictor=2, tile_bytes={4: cut[:len(cut) // 2]})[0]
    got, status, tile_status = det.tiff_decode(datas, layouts=_layouts(datas))
    _check_three_good_one_zero(got, status, imgs, 2)
    assert tile_status[2, 4] != 0 and np.count_nonzero(tile_status) == 1


def test_a_deflate_tile_with_a_wrong_trailer_costs_a_status_and_a_zero_frame(det):
    imgs, datas = _four(tt.ADOBE_DEFLATE)
    rows = tc.strip_rows(tt.tile_array(imgs[1], 2, 0, BTW, BTL, np.random.default_rng(0)), 0, BTL, "<", 2, 1)
    z = bytearray(zlib.compress(rows.tobytes(), 6))
    z[-1] ^= 0x55                                              # the Adler-32
    datas[1] = tt.encode(imgs[1], BTW, BTL, compression=tt.ADOBE_DEFLATE, predictor=2, tile_bytes={2: bytes(z)})[0]
    got, status, tile_status = det.tiff_decode(datas, layouts=_layouts(datas))
    _check_three_good_one_zero(got, status, imgs, 1)
    assert tile_status[1, 2] != 0 and np.count_nonzero(tile_status) == 1


def test_a_tile_past_its_files_area_and_a_wrong_first_row_cost_a_status_and_a_zero_frame(det):
    imgs, datas = _four(tt.NONE, bits=16)
    pitch = (max(len(d) for d in datas) + 15) // 16 * 16
    for field, tile, value, bad in (("offset", 5, pitch - BTW * BTL * 2 + 1, 3), ("first_row", 3, 0, 0), ("rows", 0, BTL - 1, 2)):
        lays = _layouts(datas)
        lays[bad].strips = lays[bad].strips.copy()
        lays[bad].strips[field][tile] = value
        got, status, _ = det.tiff_decode(datas, layouts=lays)
        _check_three_good_one_zero(got, status, imgs, bad)
    # a record count that is not across x down
    lays = _layouts(datas)
    lays[1].strips, lays[1].nstrips = lays[1].strips[:5].copy(), 5
    got, status, _ = det.tiff_decode(datas, layouts=lays)
    _check_three_good_one_zero(got, status, imgs, 1)


def test_more_tiles_than_lanes_in_flight(det):
    """Lanes loop over the tile slots: four frames of 21 tiles on 64 lanes, LZW and Deflate."""
    imgs = [tc.random_image(BW, BH, 3, 8, seed=400 + k) for k in range(4)]
    for comp, option in ((tt.LZW, "tiff_lzw_lanes"), (tt.ADOBE_DEFLATE, "tiff_deflate_lanes")):
        datas = [tt.encode(img, 16, 16, compression=comp, predictor=2, seed=k)[0] for k, img in enumerate(imgs)]
        lays = _layouts(datas)
        assert sum(l.nstrips for l in lays) == 4 * 21 > 64
        det.set_option(option, 64)
        try:
            got, status, tile_status = det.tiff_decode(datas, layouts=lays)
        finally:
            det.set_option(option, 0)
        assert status.tolist() == [0] * 4 and not tile_status.any()
        for k in range(4):
            assert np.array_equal(got[k].cpu().numpy(), tc.grey_of(imgs[k], 2)), (comp, k)


def test_decode_batch_tiled_refuses_bad_tile_sizes_and_equals_the_strip_entry_at_zero(det):
    import torch
    img = tc.random_image(33, 17, 1, 8, seed=2)
    data = tt.encode(img, 16, 16)[0]
    lay = mrgingham_amd.tiff_layout(data, tiles=True)
    pitch = (len(data) + 15) // 16 * 16
    files = torch.zeros((1, pitch), dtype=torch.uint8, device="cuda")
    files[0, :len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    recs = torch.from_numpy(lay.strips.view(np.uint8).copy()).cuda()
    ns = torch.full((1,), lay.nstrips, dtype=torch.int32, device="cuda")
    out = torch.full((1, 17, 33), 9, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    tile_status = torch.full((1, lay.nstrips), 3, dtype=torch.int32, device="cuda")
    info = _lib.TiffInfo(*lay.key())

    def call(tw, tl, recs_ptr=None, n=None, pitch_=None):
        return det.L.mrgingham_amd_tiff_decode_batch_tiled(det.ctx, files.data_ptr(), pitch, recs.data_ptr() if recs_ptr is None else recs_ptr,
                                                           lay.nstrips if pitch_ is None else pitch_, ns.data_ptr() if n is None else n, 1,
                                                           ctypes.byref(info), tw, tl, out.data_ptr(), 17 * 33, 33, status.data_ptr(),
                                                           tile_status.data_ptr(), None)
    for tw, tl in ((16, 0), (0, 16), (20, 16), (8, 16), (32768, 16), (16, 32768), (-16, 16), (16, -1)):
        assert call(tw, tl) == -1, (tw, tl)
    torch.cuda.synchronize()
    assert (out == 9).all() and status.tolist() == [5] and (tile_status == 3).all()          # nothing written
    assert call(16, 16) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0] and np.array_equal(out[0].cpu().numpy(), img)
    # tile sizes 0 and 0: mrgingham_amd_tiff_decode_batch, on a strip file's records
    sdata = tc.encode(img, rows_per_strip=5)[0]
    slay = mrgingham_amd.tiff_layout(sdata)
    assert len(sdata) <= pitch
    files.zero_()
    files[0, :len(sdata)] = torch.from_numpy(np.frombuffer(sdata, np.uint8).copy()).cuda()
    srecs = torch.from_numpy(slay.strips.view(np.uint8).copy()).cuda()
    sns = torch.full((1,), slay.nstrips, dtype=torch.int32, device="cuda")
    out.fill_(9)
    assert call(0, 0, recs_ptr=srecs.data_ptr(), n=sns.data_ptr(), pitch_=slay.nstrips) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0] and np.array_equal(out[0].cpu().numpy(), img)
    # the tiled file's records read as strips: a dead frame, not a misread one
    out.fill_(9)
    files.zero_()
    files[0, :len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    assert call(0, 0) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [-1] and not out.any()


# ---- read_tiffs -----------------------------------------------------------------------------------------------------------
W0, H0 = 45, 37


@pytest.fixture(scope="module")
def mixed_files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tiled"))
    paths, source = {}, {}

    def put(name, img, tile=None, **kw):
        paths[name] = os.path.join(d, name + ".tif")
        if tile is None:
            tc.write(paths[name], img, **kw)
        else:
            tt.write(paths[name], img, *tile, **kw)
        source[name] = tc.grey_of(img, 2 if img.ndim == 3 else 1)
    put("strip_lzw", tc.random_image(W0, H0, 1, 8, seed=1), compression=tc.LZW, predictor=2, rows_per_strip=4)
    put("tiled_lzw_16", tc.random_image(W0, H0, 1, 8, seed=2), (16, 16), compression=tt.LZW, predictor=2)
    put("tiled_none_48", tc.random_image(W0, H0, 3, 8, seed=3), (48, 24), order=">", odd=True, reverse=True)
    put("tiled_lzw_16_again", tc.random_image(W0, H0, 1, 8, seed=4), (16, 16), compression=tt.LZW, predictor=2)
    put("tiled_20", tc.random_image(W0, H0, 1, 8, seed=5), (20, 12), compression=tt.LZW, predictor=2)
    put("tiled_packbits", tc.random_image(W0, H0, 1, 8, seed=6), (16, 16), compression=tt.PACKBITS)
    put("tiled_more_tiles_than_rows", tc.random_image(W0, H0, 1, 8, seed=7), (16, 1), compression=tt.LZW, predictor=2)
    put("tiled_deflate_32", tc.random_image(W0, H0, 1, 8, seed=8), (32, 8), compression=tt.ADOBE_DEFLATE, predictor=2)
    put("strip_rgb", tc.random_image(W0, H0, 3, 8, seed=9), rows_per_strip=5)
    put("tiled_other_size", tc.random_image(W0 + 1, H0, 1, 8, seed=10), (16, 16), compression=tt.LZW)
    paths["missing"] = os.path.join(d, "missing.tif")
    return paths, source


MIXED = ["strip_lzw", "tiled_lzw_16", "tiled_none_48", "tiled_other_size", "tiled_lzw_16_again", "tiled_20", "missing", "tiled_packbits",
         "tiled_more_tiles_than_rows", "tiled_deflate_32", "strip_rgb"]
MIXED_STATUS = [0, 0, 0, -2, 0, 0, -1, 0, 0, 0, 0]


@pytest.mark.parametrize("nthreads,chunk,deflate", [(1, 0, None), (0, 0, "device"), (4, 3, "device")],
                         ids=["one_thread", "all_threads_deflate_device", "chunks_of_3_deflate_device"])
def test_read_tiffs_mixes_strip_and_tiled_files(det, mixed_files, nthreads, chunk, deflate):
    """Strip files and tiled files of one size in one list: two tilings the device takes, a tile width of 20, a PackBits file
    and a file with more tiles than rows, which keep the host threads; a file of another size and a missing one."""
    paths, source = mixed_files
    assert mrgingham_amd.tiff_layout(open(paths["tiled_more_tiles_than_rows"], "rb").read(), tiles=True).nstrips == 3 * H0 > H0
    det.set_option("tiff_chunk_frames", chunk)
    try:
        frames, status = det.read_tiffs([paths[n] for n in MIXED], nthreads=nthreads, deflate=deflate)
    finally:
        det.set_option("tiff_chunk_frames", 0)
    assert status.tolist() == MIXED_STATUS
    got = frames.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (len(MIXED), H0, W0)
    for f, name in enumerate(MIXED):
        if MIXED_STATUS[f] == 0:
            assert np.array_equal(got[f], source[name]), name
        else:
            assert not got[f].any(), name


def test_read_tiffs_on_tiles_that_are_mostly_padding(det, tmp_path):
    """A 16 x 600 frame in 600 Deflate tiles of 8192 x 1 whose padding is zeros: a file of some 30 KB whose tiles, all
    decoded, are 4.9 MB for 9600 samples -- more than the loader holds per frame on the device, so a host thread decodes it
    inside the batch; its neighbour in 16 x 16 tiles goes through the device.  Same bytes either way."""
    imgs = [tc.random_image(16, 600, 1, 8, seed=50 + k) for k in range(2)]
    paths = [str(tmp_path / "padding.tif"), str(tmp_path / "plain.tif")]
    tiles = {i: zlib.compress(imgs[0][i].tobytes() + bytes(8192 - 16), 6) for i in range(600)}
    data, recs = tt.encode(imgs[0], 8192, 1, compression=tt.ADOBE_DEFLATE, tile_bytes=tiles)
    lay = mrgingham_amd.tiff_layout(data, deflate_max_strip=8192, tiles=True)
    # (small enough to be staged -- the loader stages files up to four times the frame's samples + 16 bytes a row + 64 KiB --,
    # and as many tiles as rows, so that only the padding keeps it off the device)
    assert lay.taken and lay.nstrips == 600 and len(data) < 4 * 16 * 600 + 16 * 600 + 65536 and 600 * 8192 > 16 * 16 * 600 + (1 << 20)
    with open(paths[0], "wb") as f:
        f.write(data)
    tt.write(paths[1], imgs[1], 16, 16, compression=tt.ADOBE_DEFLATE, predictor=2)
    frames, status = det.read_tiffs(paths, nthreads=2, deflate="device")
    assert status.tolist() == [0, 0]
    for k in range(2):
        assert np.array_equal(frames[k].cpu().numpy(), imgs[k]), k


# ---- find_boards_files and the tool -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def board_files(tmp_path_factory):
    from mrgingham_amd import synth
    from tests import files_cases
    d = str(tmp_path_factory.mktemp("boards"))
    board = synth.board_frame(640, 480, 10, seed=0).numpy()
    files = {n: os.path.join(d, n) for n in ("board.pgm", "board_strip_lzw.tif", "board_tiled_lzw_128.tif", "board_tiled_deflate_64.tif")}
    files_cases.write_pgm(files["board.pgm"], board)
    tc.write(files["board_strip_lzw.tif"], board, compression=tc.LZW, predictor=2, rows_per_strip=16)
    tt.write(files["board_tiled_lzw_128.tif"], board, 128, 128, compression=tt.LZW, predictor=2)
    tt.write(files["board_tiled_deflate_64.tif"], board, 64, 64, compression=tt.ADOBE_DEFLATE, predictor=2, order=">")
    return files, list(files.values())


def test_find_boards_files_gives_the_same_boards_for_tiled_files(board_files, tmp_path_factory):
    files, paths = board_files
    runs = [{"id": "device", "paths": paths, "kw": {"batch": 4, "nthreads": 4, "tiff": "device", "tiff_deflate": "device"}},
            {"id": "host", "paths": paths, "kw": {"batch": 4, "nthreads": 4, "tiff": "host"}}]
    out = run_child(str(tmp_path_factory.mktemp("board_runs")), {"runs": runs})
    for rid in ("device", "host"):
        assert out[rid + "_status"].tolist() == [0] * 4 and out[rid + "_found"][0] >= 0
        for i in range(1, 4):
            assert out[rid + "_found"][i] == out[rid + "_found"][0], (rid, paths[i])
            assert np.array_equal(out[rid + "_boards"][i], out[rid + "_boards"][0]), (rid, paths[i])
            assert np.array_equal(out[rid + "_levels"][i], out[rid + "_levels"][0]), (rid, paths[i])
    assert np.array_equal(out["device_boards"], out["host_boards"], equal_nan=True)


def test_tool_batch_with_the_device_route_prints_the_records_of_the_tool_without_batch(board_files):
    files, paths = board_files

    def records(r):
        assert r.returncode == 0, r.stderr
        order, rec, _ = parse_vnlog(r.stdout)
        assert order == paths
        return [[line.split(" ", 1)[1] for line in rec[p]] for p in paths]
    want = records(run_tool("--jobs", "1", *paths))
    assert all(len(r) == 100 for r in want) and all(r == want[0] for r in want)
    assert records(run_tool("--jobs", "4", "--batch", "4", "--tiff-lzw", "device", *paths)) == want
    assert records(run_tool("--jobs", "4", "--batch", "4", "--tiff-lzw", "device", "--tiff-deflate", "device", *paths)) == want
