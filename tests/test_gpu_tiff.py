"""TIFF files into device frames (Detector.tiff_decode, Detector.read_tiffs, find_boards_files(tiff="device"), the tool's
--tiff-lzw): LZW strips decoded one lane each, the predictor undone and colour reduced to grey on the device.  The
yardstick is read_image on the same file, byte for byte, plus the array the test wrote into the file (tests/tiff_cases.py;
TIFF here is lossless).  No tolerance anywhere.

The shapes are the smallest that reach the seams of the two schedules (mrgingham_amd.tiff_geometry): the lanes in flight
of the LZW launch, the 16 pixels of a lane and the 1024 pixels of a wave's step in the finish kernel."""
import os

import numpy as np
import pytest

import mrgingham_amd
from tests import files_cases, tiff_cases as tc
from tests.test_gpu_files import STATS, parse_vnlog, run_child, run_tool

pytestmark = pytest.mark.gpu

LANES, SEG, STEP = mrgingham_amd.tiff_geometry()


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector()
    yield d
    d.close()


def _host(tmp_path, data):
    p = tmp_path / "host.tif"
    p.write_bytes(data)
    return mrgingham_amd.read_image(str(p))


def _high(a):
    return a if a.dtype == np.uint8 else (a >> 8).astype(np.uint8)


def _decode(det, datas, **kw):
    frames, status, strip_status = det.tiff_decode(datas, **kw)
    return frames.cpu().numpy(), status, strip_status


# ---- LZW ----------------------------------------------------------------------------------------------------------------
def test_lzw_noise_every_width_and_a_clear_in_mid_stream(det, tmp_path):
    img = tc.noise()                                               # 67 x 131 in one strip
    st = {}
    tc.lzw_encode(img.tobytes(), stats=st)
    assert st["widths"] == [9, 10, 11, 12] and st["clears"] >= 2 and st["codes"] > 8000
    data = tc.encode(img, compression=tc.LZW)[0]
    got, status, strip_status = _decode(det, [data])
    assert status.tolist() == [0] and not strip_status.any()
    assert np.array_equal(got[0], img) and np.array_equal(got[0], _host(tmp_path, data))


def test_lzw_constant_image_every_code_not_yet_in_the_table(det, tmp_path):
    img = np.full((128, 512), 7, np.uint8)                          # strings grow to 361 bytes, every copy overlaps its destination
    st = {}
    tc.lzw_encode(img.tobytes(), stats=st)
    assert st["codes"] < 400
    data = tc.encode(img, compression=tc.LZW)[0]
    got, status, _ = _decode(det, [data])
    assert status.tolist() == [0] and np.array_equal(got[0], img) and np.array_equal(got[0], _host(tmp_path, data))


def _strips_33x200(seed, **kw):
    img = tc.random_image(33, 200, 1, 8, seed=seed)
    data, strips = tc.encode(img, compression=tc.LZW, rows_per_strip=3, **kw)
    assert len(strips) == 67 and strips[-1][3] == 2                 # more strips than a wave has lanes; the last one short
    return img, data


def test_lzw_more_strips_than_a_wave_and_streams_the_rules_allow(det, tmp_path):
    imgs, datas = zip(*[_strips_33x200(1, reverse=True, odd=True), _strips_33x200(2, lzw=dict(open_with_clear=False)),
                        _strips_33x200(3, lzw=dict(trailing=b"\xff\x00\xaa" * 3))])
    got, status, strip_status = _decode(det, datas)
    assert status.tolist() == [0, 0, 0] and not strip_status.any()
    for k in range(3):
        assert np.array_equal(got[k], imgs[k]) and np.array_equal(got[k], _host(tmp_path, datas[k])), k


def test_lzw_more_strips_than_lanes_in_flight(det):
    """Lanes loop over the strips: with the test hook at 64 lanes three frames of 67 strips, and at the shipped lane count
    enough frames of 67 strips to exceed it."""
    a, da = _strips_33x200(4)
    b, db = _strips_33x200(5)
    det.set_option("tiff_lzw_lanes", 64)
    try:
        got, status, _ = _decode(det, [da, db, da])
    finally:
        det.set_option("tiff_lzw_lanes", 0)
    assert status.tolist() == [0, 0, 0] and np.array_equal(got[0], a) and np.array_equal(got[1], b) and np.array_equal(got[2], a)
    n = LANES // 67 + 2
    assert n * 67 > LANES and n < 300
    got, status, _ = _decode(det, [da, db] * (n // 2))
    assert not status.any()
    assert (got[0::2] == a).all() and (got[1::2] == b).all()


# ---- the finish kernel ----------------------------------------------------------------------------------------------------
WIDTHS = (1, SEG - 1, SEG, SEG + 1, 67, STEP - 1, STEP, STEP + 1)


@pytest.mark.parametrize("width", WIDTHS)
def test_finish_kernel(det, tmp_path, width):
    """Widths on the seams of a lane's segment and of a wave's step, crossed with 8 / 16 bit, 1 .. 4 samples, predictor
    1 / 2 and both byte orders; WhiteIsZero, grey with extra samples, RowsPerStrip above the height and 2^32 - 1, strips at
    odd offsets and in reverse order, uncompressed and LZW take turns.  out has a wider stride and a larger frame pitch,
    filled with a sentinel that must survive."""
    import torch
    H, B, n = 5, 2, 0
    for bits in (8, 16):
        for samples in (1, 2, 3, 4):
            for pred in (1, 2):
                for order in "<>":
                    kw = dict(order=order, predictor=pred, compression=tc.LZW if n % 4 in (1, 2) else tc.NONE,
                              rows_per_strip=[None, 2, 1, 3][n % 4], odd=n % 3 == 0, reverse=n % 5 == 0)
                    if n % 8 == 4:
                        kw.update(rows_per_strip=None, rps_tag=[2 ** 32 - 1, H + 7][(n // 8) % 2])
                    photo = 2 if samples >= 3 else 1
                    if samples <= 2 and n % 2 == 0:
                        photo = 0
                    if samples >= 3 and n % 6 == 1:
                        photo = 1
                    kw["photometric"] = photo
                    imgs = [tc.random_image(width, H, samples, bits, seed=100 * n + k) for k in range(B)]
                    datas = [tc.encode(img, **kw)[0] for img in imgs]
                    sentinel = 0xA5 if bits == 8 else 0xA5C3
                    big = torch.from_numpy(np.full((B, H + 2, width + 5), sentinel, np.uint8 if bits == 8 else np.uint16)).cuda()
                    got, status, _ = det.tiff_decode(datas, out=big[:, :H, :])
                    label = (width, bits, samples, pred, order, kw)
                    assert status.tolist() == [0] * B, label
                    whole = big.cpu().numpy()
                    for k in range(B):
                        want = tc.grey_of(imgs[k], photo)
                        assert np.array_equal(whole[k, :H, :width], want), label
                        if k == 0 or n % 4 == 0:
                            assert np.array_equal(_high(want), _host(tmp_path, datas[k])), label
                    assert (whole[:, :H, width:] == sentinel).all() and (whole[:, H:, :] == sentinel).all(), label
                    n += 1
    assert n == 32


@pytest.mark.parametrize("bits,samples,compression,predictor,order", [(8, 1, tc.NONE, 1, "<"), (16, 3, tc.LZW, 2, ">")],
                         ids=["8bit_uncompressed", "16bit_be_lzw_predictor2_rgb"])
def test_finish_kernel_takes_a_second_trip_over_the_rows(det, tmp_path, bits, samples, compression, predictor, order):
    """The finish kernel's grid is capped at eight workgroups per CU, four waves each, one row per wave and trip: every
    full-size call loops, no other shape of this file does.  Two frames of 17 x (16 CUs + 100): one full trip and 200 rows
    of a second one, which begins in the middle of the second frame."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows_per_trip = 8 * cus * 4
    W, H, B = 17, 16 * cus + 100, 2
    assert rows_per_trip < B * H < 2 * rows_per_trip and H < rows_per_trip     # two trips, the last one ragged
    imgs = [tc.random_image(W, H, samples, bits, seed=40 + k) for k in range(B)]
    datas = [tc.encode(img, order=order, compression=compression, predictor=predictor, rows_per_strip=128)[0] for img in imgs]
    got, status, strip_status = _decode(det, datas)
    assert status.tolist() == [0] * B and not strip_status.any()
    for k in range(B):
        want = tc.grey_of(imgs[k], 2 if samples >= 3 else 1)
        assert got[k].dtype == want.dtype and np.array_equal(got[k], want), k
        assert np.array_equal(_high(want), _host(tmp_path, datas[k])), k


def test_decode_batch_refuses_bad_descriptors(det):
    import ctypes
    import torch
    from mrgingham_amd import _lib
    img = tc.random_image(17, 4, 1, 8)
    data = tc.encode(img)[0]
    lay = mrgingham_amd.tiff_layout(data)
    files = torch.zeros((1, 256), dtype=torch.uint8, device="cuda")
    strips = torch.from_numpy(lay.strips.view(np.uint8).copy()).cuda()
    ns = torch.ones(1, dtype=torch.int32, device="cuda")
    out = torch.full((1, 4, 17), 9, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), 5, dtype=torch.int32, device="cuda")

    def call(info, files_ptr=None, pitch=256, strips_pitch=1, stride=17, ctx=None):
        return det.L.mrgingham_amd_tiff_decode_batch(det.ctx if ctx is None else ctx, files.data_ptr() if files_ptr is None else files_ptr, pitch,
                                                     strips.data_ptr(), strips_pitch, ns.data_ptr(), 1, ctypes.byref(info), out.data_ptr(),
                                                     4 * 17, stride, status.data_ptr(), None, None)
    good = _lib.TiffInfo(*lay.key())
    for field, value in (("bits", 12), ("samples", 5), ("photometric", 3), ("compression", 32773), ("predictor", 3), ("width", 0), ("height", 40000)):
        bad = _lib.TiffInfo(*lay.key())
        setattr(bad, field, value)
        assert call(bad) == -1, field
    assert call(good, pitch=250) == -1 and call(good, files_ptr=files.data_ptr() + 4) == -1
    assert call(good, strips_pitch=0) == -1 and call(good, stride=16) == -1
    torch.cuda.synchronize()
    assert (out == 9).all() and status.tolist() == [5]          # nothing written
    # a strip record that does not fit its file's area: status -1 and a zero frame, no fault
    wild = lay.strips.copy()
    wild["offset"] = 250
    strips.copy_(torch.from_numpy(wild.view(np.uint8).copy()))
    assert call(good) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [-1] and not out.any()


# ---- crafted LZW on the device --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.broken_lzw_strips()))
def test_a_broken_lzw_strip_costs_a_status_and_a_zero_frame(det, tmp_path, name):
    """The strips test_tiff_io.py has taken through the shared decoder under the sanitizers: status -1 and a zero-filled
    frame, exactly as the host decoder judges the file, and the neighbouring frames of the batch intact."""
    good = tc.noise()
    other = np.ascontiguousarray(good[::-1])
    broken = tc.encode(good, compression=tc.LZW, strip_bytes=[tc.broken_lzw_strips()[name]])[0]
    assert _host(tmp_path, broken) is None
    datas = [tc.encode(good, compression=tc.LZW)[0], broken, tc.encode(other, compression=tc.LZW)[0]]
    got, status, strip_status = _decode(det, datas)
    assert status.tolist() == [0, -1, 0] and strip_status[:, 0].tolist()[0] == 0 and strip_status[1, 0] != 0
    assert np.array_equal(got[0], good) and not got[1].any() and np.array_equal(got[2], other)


# ---- read_tiffs -----------------------------------------------------------------------------------------------------------
W0, H0 = 45, 37


@pytest.fixture(scope="module")
def tiff_files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tiffs"))
    paths, source = {}, {}

    def put(name, img, **kw):
        paths[name] = os.path.join(d, name + ".tif")
        tc.write(paths[name], img, **kw)
        source[name] = tc.grey_of(img, kw.get("photometric", 2 if img.ndim == 3 and img.shape[2] >= 3 else 1))
    put("lzw", tc.random_image(W0, H0, 1, 8, seed=1), compression=tc.LZW, predictor=2, rows_per_strip=4)
    put("rgb", tc.random_image(W0, H0, 3, 8, seed=2), order=">", rows_per_strip=5, reverse=True)
    put("other_size", tc.random_image(W0 + 1, H0, 1, 8, seed=3), compression=tc.LZW)
    put("packbits", tc.random_image(W0, H0, 1, 8, seed=4), compression=tc.PACKBITS, rows_per_strip=8)
    put("deep", tc.random_image(W0, H0, 1, 16, seed=5), compression=tc.LZW, predictor=2, order=">")
    put("deep_rgb", tc.random_image(W0, H0, 3, 16, seed=6), rows_per_strip=7)
    put("deep_deflate", tc.random_image(W0, H0, 2, 16, seed=7), compression=tc.ADOBE_DEFLATE, predictor=2)
    paths["truncated"] = os.path.join(d, "truncated.tif")
    with open(paths["truncated"], "wb") as f:
        f.write(open(paths["lzw"], "rb").read()[:-30])
    paths["broken_strip"] = os.path.join(d, "broken_strip.tif")
    img = tc.random_image(W0, H0, 1, 8, seed=8)
    good_strip = tc.lzw_encode(img.tobytes())
    with open(paths["broken_strip"], "wb") as f:
        f.write(tc.encode(img, compression=tc.LZW, strip_bytes=[good_strip[:len(good_strip) // 2]])[0])
    paths["missing"] = os.path.join(d, "missing.tif")
    return paths, source


EIGHT = ["lzw", "rgb", "other_size", "packbits", "truncated", "missing", "deep", "broken_strip"]
EIGHT_STATUS = [0, 0, -2, 0, -1, -1, -2, -1]


@pytest.mark.parametrize("nthreads,chunk", [(1, 0), (0, 0), (4, 3)], ids=["one_thread", "all_threads", "chunks_of_3"])
def test_read_tiffs_8bit_list(det, tiff_files, nthreads, chunk):
    """Two good files, one of another size, a PackBits file the host threads decode inside the batch, a truncated file, a
    missing path, a 16-bit file in an 8-bit call -- and a file whose one LZW strip is cut short, which only the device
    finds out."""
    paths, source = tiff_files
    det.set_option("tiff_chunk_frames", chunk)
    try:
        frames, status = det.read_tiffs([paths[n] for n in EIGHT], nthreads=nthreads)
    finally:
        det.set_option("tiff_chunk_frames", 0)
    assert status.tolist() == EIGHT_STATUS
    got = frames.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (len(EIGHT), H0, W0)
    for f, name in enumerate(EIGHT):
        if EIGHT_STATUS[f] == 0:
            assert np.array_equal(got[f], mrgingham_amd.read_image(paths[name])), name
            assert np.array_equal(got[f], source[name]), name
        else:
            assert mrgingham_amd.read_image(paths[name]) is None or EIGHT_STATUS[f] == -2
            assert not got[f].any(), name


def test_read_tiffs_16bit_list(det, tiff_files):
    paths, source = tiff_files
    names = ["deep", "deep_rgb", "lzw", "deep_deflate", "missing"]
    frames, status = det.read_tiffs([paths[n] for n in names], nthreads=2)
    assert status.tolist() == [0, 0, -2, 0, -1]
    got = frames.cpu().numpy()
    assert got.dtype == np.uint16 and got.shape == (5, H0, W0)
    for f, name in enumerate(names):
        if status[f] == 0:
            assert np.array_equal(got[f], source[name]), name
        else:
            assert not got[f].any(), name
    frames, status = det.read_tiffs([paths["missing"]])
    assert tuple(frames.shape) == (1, 0, 0) and status.tolist() == [-1]


def test_a_strip_above_tiff_lzw_max_strip_keeps_the_host_threads(det, tiff_files):
    paths, source = tiff_files
    det.set_option("tiff_lzw_max_strip", 4 * W0 - 1)            # the file's strips decode to 4 * W0 bytes
    try:
        frames, status = det.read_tiffs([paths["lzw"], paths["rgb"]])
    finally:
        det.set_option("tiff_lzw_max_strip", 64 << 10)               # (the default)
    assert status.tolist() == [0, 0]
    assert np.array_equal(frames[0].cpu().numpy(), source["lzw"]) and np.array_equal(frames[1].cpu().numpy(), source["rgb"])


# ---- find_boards_files ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def board_files(tmp_path_factory):
    files = files_cases.write_all(tmp_path_factory.mktemp("files"))
    board = files_cases.board_pixels()
    d = os.path.dirname(files["board.pgm"])

    def put(name, img, **kw):
        files[name] = os.path.join(d, name)
        tc.write(files[name], img, **kw)
    put("board_lzw.tif", board, compression=tc.LZW, predictor=2, rows_per_strip=16)
    put("board_none.tif", board, order=">", rows_per_strip=100, reverse=True, odd=True)
    put("board_rgb.tif", np.stack([board] * 3, axis=-1), compression=tc.LZW, rows_per_strip=8)      # r = g = b: its grey is the board
    put("board_packbits.tif", board, compression=tc.PACKBITS)
    put("board16.tif", board.astype(np.uint16) * 257, compression=tc.LZW, predictor=2, order=">", rows_per_strip=16)
    paths = [files["board_lzw.tif"], files["board.pgm"], files["board_none.tif"], files[files_cases.BOARD], files["board16.tif"],
             files["board16.pgm"], files["board_rgb.tif"], files["missing"], files["board_packbits.tif"], files["board_lzw.tif"]]
    return files, paths


@pytest.fixture(scope="module")
def board_runs(board_files, tmp_path_factory):
    _, paths = board_files
    runs = [{"id": f"{tiff}_{deep}", "paths": paths, "kw": {"batch": 4, "nthreads": 4, "tiff": tiff, "deep": deep}}
            for tiff in ("host", "device") for deep in ("one", "chunks")]
    return run_child(str(tmp_path_factory.mktemp("board_runs")), {"runs": runs})


@pytest.mark.parametrize("deep", ["one", "chunks"])
def test_find_boards_files_tiff_device_equals_host_and_the_same_pixels_as_pgm(board_files, board_runs, deep):
    files, paths = board_files
    out = board_runs
    for what in ("status", "found", "levels"):
        assert np.array_equal(out[f"device_{deep}_{what}"], out[f"host_{deep}_{what}"]), what
    assert np.array_equal(out[f"device_{deep}_boards"], out[f"host_{deep}_boards"], equal_nan=True)
    pgm8, pgm16 = paths.index(files["board.pgm"]), paths.index(files["board16.pgm"])
    for tiff in ("host", "device"):
        rid = f"{tiff}_{deep}"
        assert out[rid + "_status"].tolist() == [0 if "missing" not in p else -1 for p in paths]
        assert out[rid + "_found"][pgm8] >= 0 and out[rid + "_found"][pgm16] >= 0          # (the files bear boards)
        for i, p in enumerate(paths):
            if not p.endswith(".tif"):
                continue
            ref = pgm16 if p.endswith("board16.tif") else pgm8
            assert out[rid + "_found"][i] == out[rid + "_found"][ref], (rid, p)
            assert np.array_equal(out[rid + "_boards"][i], out[rid + "_boards"][ref]), (rid, p)     # double for double
            assert np.array_equal(out[rid + "_levels"][i], out[rid + "_levels"][ref]), (rid, p)
        stats = dict(zip(STATS, out[rid + "_stats"]))
        assert stats["files_device_loader"] + stats["files_host_decoded"] + stats["files_one_image"] + stats["files_unreadable"] == len(paths)
        tif8 = sum(1 for p in paths if p.endswith(".tif") and "16" not in os.path.basename(p))
        deep_files = 2 if deep == "chunks" else 0                   # board16.tif and board16.pgm
        assert stats["files_one_image"] == 2 - deep_files and stats["files_unreadable"] == 1
        if tiff == "device":      # JPEG, the TIFF files (the PackBits one is decoded by the loader's threads inside its batch), 16-bit PGM
            assert stats["files_device_loader"] == 1 + tif8 + deep_files and stats["files_host_decoded"] == 1
        else:                     # TIFF files behave as PGM and PNG files do
            assert stats["files_device_loader"] == 1 + deep_files // 2 and stats["files_host_decoded"] == 1 + tif8 + deep_files // 2


def test_tool_prints_the_same_vnlog_for_tif_as_for_pgm(board_files, tmp_path):
    files, _ = board_files
    names = ["board_lzw", "board_none", "board_rgb", "board_packbits", "board16"]
    tifs = [files[n + ".tif"] for n in names]
    pgms = []
    for n in names:
        p = str(tmp_path / (n + ".pgm"))
        with open(p, "wb") as f:
            f.write(open(files["board16.pgm" if n == "board16" else "board.pgm"], "rb").read())
        pgms.append(p)

    def records(r, paths):
        assert r.returncode == 0, r.stderr
        order, rec, _ = parse_vnlog(r.stdout)
        assert order == paths
        return [[line.split(" ", 1)[1] for line in rec[p]] for p in paths]
    want = records(run_tool("--jobs", "1", *pgms), pgms)        # (one worker: records in list order)
    assert all(len(r) == 100 for r in want)
    assert records(run_tool("--jobs", "1", *tifs), tifs) == want
    assert records(run_tool("--jobs", "4", "--batch", "64", "--tiff-lzw", "device", "--deep-batch", "chunks", *tifs), tifs) == want
    assert records(run_tool("--jobs", "4", "--batch", "64", *tifs), tifs) == want
    r = run_tool("--tiff-lzw", "device", *tifs)
    assert r.returncode == 1 and "--tiff-lzw is only accepted with --batch" in r.stderr
