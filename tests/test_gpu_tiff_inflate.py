"""Deflate TIFF strips on the device (Detector.tiff_decode on layouts with a Deflate limit, Detector.read_tiffs(deflate=
"device"), find_boards_files(tiff_deflate="device"), the tool's --tiff-deflate): one lane per strip through the text of
csrc/tiff_inflate.h.  The yardstick is read_image -- zlib -- on the same file plus the array written into it; no tolerance.
The streams are the lists of tests/tiff_inflate_cases.py, the ones test_tiff_inflate.py walks under the sanitizers."""
import os

import numpy as np
import pytest

import mrgingham_amd
from mrgingham_amd import _lib
from tests import files_cases, tiff_cases as tc, tiff_inflate_cases as ic
from tests.test_gpu_files import STATS, parse_vnlog, run_child, run_tool

pytestmark = pytest.mark.gpu

LANES = _lib.lib().mrgingham_amd_tiff_inflate_lanes()
MAX = 1 << 20


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
    layouts = [mrgingham_amd.tiff_layout(d, deflate_max_strip=MAX) for d in datas]
    assert all(l is not None and l.taken for l in layouts)
    frames, status, strip_status = det.tiff_decode(datas, layouts=layouts, **kw)
    return frames.cpu().numpy(), status, strip_status


def test_block_kinds(det, tmp_path):
    """Four 300 x 300 files of one strip in one call -- dynamic blocks with matches 32400 bytes back and repeat codes 16 and
    18, the same at level 9, one run of length-258 copies at distance 1, stored blocks -- and 40 x 6 files of one row per
    strip, fixed blocks; the walker says that each kind is there."""
    datas, imgs = [], []
    seen = {}
    for name, img, level in ic.block_kind_images():
        data, streams = ic.deflate_file(img, level)
        seen[name] = ic.walk(streams[0])
        assert seen[name]["out"] == img.tobytes()
        datas.append(data)
        imgs.append(img)
    assert seen["ramp"]["kinds"] == {2} and seen["ramp"]["blocks"] == 2 and {16, 18} <= seen["ramp"]["repeats"]
    assert seen["ramp"]["max_distance"] > 32400 and seen["ramp_over_8"]["kinds"] == {2} and seen["ramp_over_8"]["max_distance"] > 32000
    assert seen["constant"]["max_length"] == 258 and seen["constant"]["max_distance"] == 1 and seen["constant"]["overlap"]
    assert seen["noise"]["kinds"] == {0} and seen["noise"]["blocks"] > 1
    got, status, strip_status = _decode(det, datas)
    assert status.tolist() == [0] * 4 and not strip_status.any()
    for k in range(4):
        assert np.array_equal(got[k], imgs[k]) and np.array_equal(got[k], _host(tmp_path, datas[k])), k
    rows = ic.fixed_block_rows()
    variants = [rows, np.ascontiguousarray(rows[::-1])]
    datas = []
    for img in variants:
        data, streams = ic.deflate_file(img, rows_per_strip=1)
        assert len(streams) == 6 and all(ic.walk(s)["kinds"] == {1} for s in streams)
        datas.append(data)
    got, status, strip_status = _decode(det, datas)
    assert status.tolist() == [0, 0] and not strip_status.any()
    for k in range(2):
        assert np.array_equal(got[k], variants[k]) and np.array_equal(got[k], _host(tmp_path, datas[k])), k


def _strips_33x200(seed, **kw):
    img = ic.ramp_noise(200, 33, seed=seed)
    data, streams = ic.deflate_file(img, rows_per_strip=3, **kw)
    assert len(streams) == 67 and ic.walk(streams[0])["kinds"] != {0} and ic.walk(streams[-1])["kinds"] != {0}
    return img, data


def test_more_strips_than_a_wave_and_than_the_lanes_in_flight(det, tmp_path):
    """67 strips a frame, more than a wave has lanes, the last one short; strips in reverse file order and at odd offsets;
    three frames with the test hook at 64 lanes, and at the shipped lane count enough frames to exceed it."""
    a, da = _strips_33x200(4, reverse=True, odd=True)
    b, db = _strips_33x200(5)
    assert np.array_equal(_host(tmp_path, da), a) and np.array_equal(_host(tmp_path, db), b)
    det.set_option("tiff_deflate_lanes", 64)
    try:
        got, status, strip_status = _decode(det, [da, db, da])
    finally:
        det.set_option("tiff_deflate_lanes", 0)
    assert status.tolist() == [0, 0, 0] and not strip_status.any()
    assert np.array_equal(got[0], a) and np.array_equal(got[1], b) and np.array_equal(got[2], a)
    a, b = ic.ramp_noise(1200, 17, seed=6), ic.ramp_noise(1200, 17, seed=7)
    da, _ = ic.deflate_file(a, rows_per_strip=1)                  # 1200 strips a frame
    db, _ = ic.deflate_file(b, rows_per_strip=1, reverse=True)
    n = (LANES // 1200 + 3) // 2 * 2
    assert n * 1200 > LANES and n < 300
    got, status, _ = _decode(det, [da, db] * (n // 2))
    assert not status.any()
    assert (got[0::2] == a).all() and (got[1::2] == b).all()


def test_finish_kernel_behind_the_inflate_launch(det, tmp_path):
    """Width 67, 5 rows: 8 / 16 bit x 1 .. 4 samples x predictor 1 / 2 x both byte orders, compression 8 and 32946 taking
    turns, WhiteIsZero on the grey ones; out with a wider stride and a sentinel that must survive."""
    import torch
    W, H, B, n = 67, 5, 2, 0
    for bits in (8, 16):
        for samples in (1, 2, 3, 4):
            for pred in (1, 2):
                for order in "<>":
                    kw = dict(order=order, predictor=pred, compression=tc.ADOBE_DEFLATE if n % 2 else tc.DEFLATE,
                              rows_per_strip=[None, 2, 1, 3][n % 4], odd=n % 3 == 0, reverse=n % 5 == 0)
                    photo = 2 if samples >= 3 else 1
                    if samples <= 2 and (n // 2) % 2 == 0:
                        photo = 0
                    kw["photometric"] = photo
                    imgs = [tc.random_image(W, H, samples, bits, seed=100 * n + k) // (1 if k else 16) for k in range(B)]
                    datas = [tc.encode(img, **kw)[0] for img in imgs]
                    sentinel = 0xA5 if bits == 8 else 0xA5C3
                    big = torch.from_numpy(np.full((B, H + 2, W + 5), sentinel, np.uint8 if bits == 8 else np.uint16)).cuda()
                    layouts = [mrgingham_amd.tiff_layout(d, deflate_max_strip=MAX) for d in datas]
                    got, status, _ = det.tiff_decode(datas, layouts=layouts, out=big[:, :H, :])
                    label = (bits, samples, pred, order, kw)
                    assert status.tolist() == [0] * B, label
                    whole = big.cpu().numpy()
                    for k in range(B):
                        want = tc.grey_of(imgs[k], photo)
                        assert np.array_equal(whole[k, :H, :W], want), label
                        assert np.array_equal(_high(want), _host(tmp_path, datas[k])), label
                    assert (whole[:, :H, W:] == sentinel).all() and (whole[:, H:, :] == sentinel).all(), label
                    n += 1
    assert n == 32


@pytest.mark.parametrize("name", sorted(ic.crafted_accepted()))
def test_a_crafted_stream_zlib_accepts(det, tmp_path, name):
    stream, payload, shape = ic.crafted_accepted()[name]
    data = ic.craft_file(stream, shape)
    want = _host(tmp_path, data)
    assert want is not None and want.tobytes() == payload
    got, status, strip_status = _decode(det, [data])
    assert status.tolist() == [0] and strip_status.tolist() == [[0]]
    assert np.array_equal(got[0], want)


@pytest.mark.parametrize("name", sorted(ic.broken_streams()))
def test_a_broken_stream_costs_a_status_and_a_zero_frame(det, tmp_path, name):
    """In the middle of a batch of three: status -1, the strip's reason, a zero frame -- as zlib judges the file -- and
    the neighbours intact."""
    w, h = ic.CRAFT_SHAPE
    good = ic.ramp_noise(h, w)
    other = tc.noise()
    broken = ic.craft_file(ic.broken_streams()[name])
    assert _host(tmp_path, broken) is None
    datas = [tc.encode(good, compression=tc.ADOBE_DEFLATE)[0], broken, tc.encode(other, compression=tc.ADOBE_DEFLATE)[0]]
    got, status, strip_status = _decode(det, datas)
    assert status.tolist() == [0, -1, 0] and strip_status[0, 0] == 0 and strip_status[1, 0] != 0 and strip_status[2, 0] == 0
    assert np.array_equal(got[0], good) and not got[1].any() and np.array_equal(got[2], other)


def test_check_kernel_refuses_deflate_strip_records_beyond_the_limits(det, tmp_path):
    """Records tiff_layout never hands out, given to mrgingham_amd_tiff_decode_batch directly: a strip of more bytes than
    decoded + decoded / 8 + 512 -- a good stream that runs on through 6000 empty blocks, which zlib accepts -- and a strip
    that decodes to more than 1 MiB.  Status -1 and a zero frame, the neighbour intact."""
    import ctypes
    import torch
    w, h = ic.CRAFT_SHAPE
    img = ic.ramp_noise(h, w)
    long_one = ic.craft_file(ic.with_empty_blocks(img.tobytes(), 6000))
    assert np.array_equal(_host(tmp_path, long_one), img)
    assert not mrgingham_amd.tiff_layout(long_one, deflate_max_strip=MAX).taken
    good = tc.encode(img, compression=tc.ADOBE_DEFLATE)[0]
    layouts = [mrgingham_amd.tiff_layout(good, deflate_max_strip=MAX), mrgingham_amd.tiff_layout(long_one)]
    layouts[1].taken = True                                          # (what a caller with a table of its own can do)
    frames, status, strip_status = det.tiff_decode([good, long_one], layouts=layouts)
    got = frames.cpu().numpy()
    assert status.tolist() == [0, -1] and not strip_status.any()     # (no lane ran on it: the check kernel's verdict)
    assert np.array_equal(got[0], img) and not got[1].any()
    # rows x rowbytes above 1 MiB
    W, H = 32767, 33
    assert W * H > 1 << 20
    lay = mrgingham_amd.tiff_layout(tc.encode(np.zeros((H, 16), np.uint8), compression=tc.ADOBE_DEFLATE)[0], deflate_max_strip=MAX)
    info = _lib.TiffInfo(*lay.key())
    info.width = W
    files = torch.zeros((1, 256), dtype=torch.uint8, device="cuda")
    strips = torch.from_numpy(lay.strips.view(np.uint8).copy()).cuda()
    ns = torch.ones(1, dtype=torch.int32, device="cuda")
    out = torch.full((1, H, W), 9, dtype=torch.uint8, device="cuda")
    st = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    sst = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    assert det.L.mrgingham_amd_tiff_decode_batch(det.ctx, files.data_ptr(), 256, strips.data_ptr(), 1, ns.data_ptr(), 1, ctypes.byref(info),
                                                 out.data_ptr(), H * W, W, st.data_ptr(), sst.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert st.tolist() == [-1] and sst.tolist() == [0] and not out.any()


def test_decode_batch_goes_on_refusing_packbits(det):
    import ctypes
    import torch
    img = ic.ramp_noise(4, 17)
    lay = mrgingham_amd.tiff_layout(tc.encode(img, compression=tc.ADOBE_DEFLATE)[0], deflate_max_strip=MAX)
    files = torch.zeros((1, 256), dtype=torch.uint8, device="cuda")
    strips = torch.from_numpy(lay.strips.view(np.uint8).copy()).cuda()
    ns = torch.ones(1, dtype=torch.int32, device="cuda")
    out = torch.full((1, 4, 17), 9, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    for compression, rc in ((32773, -1), (7, -1), (8, 0), (32946, 0)):
        info = _lib.TiffInfo(*lay.key())
        info.compression = compression
        assert det.L.mrgingham_amd_tiff_decode_batch(det.ctx, files.data_ptr(), 256, strips.data_ptr(), 1, ns.data_ptr(), 1, ctypes.byref(info),
                                                     out.data_ptr(), 4 * 17, 17, status.data_ptr(), None, None) == rc, compression
        torch.cuda.synchronize()
        if rc:
            assert (out == 9).all() and status.tolist() == [5]
        else:                                                            # (a file of zeros is no zlib stream: a zero frame)
            assert status.tolist() == [-1] and not out.any()


# ---- read_tiffs -----------------------------------------------------------------------------------------------------------
W0, H0 = 45, 37


@pytest.fixture(scope="module")
def tiff_files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tiffs"))
    paths, source = {}, {}

    def put(name, img, **kw):
        paths[name] = os.path.join(d, name + ".tif")
        tc.write(paths[name], img, **kw)
        source[name] = tc.grey_of(img, 1)
    put("deflate", ic.ramp_noise(H0, W0, seed=1), compression=tc.ADOBE_DEFLATE, predictor=2, rows_per_strip=4)
    put("deflate_be", ic.ramp_noise(H0, W0, seed=2), compression=tc.DEFLATE, order=">", rows_per_strip=5, reverse=True, odd=True)
    put("other_size", ic.ramp_noise(H0, W0 + 1, seed=3), compression=tc.ADOBE_DEFLATE)
    put("lzw", tc.random_image(W0, H0, 1, 8, seed=4), compression=tc.LZW, rows_per_strip=6)
    put("packbits", tc.random_image(W0, H0, 1, 8, seed=5), compression=tc.PACKBITS, rows_per_strip=8)
    paths["truncated"] = os.path.join(d, "truncated.tif")
    with open(paths["truncated"], "wb") as f:
        f.write(open(paths["deflate"], "rb").read()[:-30])
    paths["cut_strip"] = os.path.join(d, "cut_strip.tif")
    img = ic.ramp_noise(H0, W0, seed=6)
    z = ic.deflate(img.tobytes())
    with open(paths["cut_strip"], "wb") as f:
        f.write(tc.encode(img, compression=tc.ADOBE_DEFLATE, strip_bytes=[z[:len(z) // 2]])[0])
    paths["missing"] = os.path.join(d, "missing.tif")
    return paths, source


LIST = ["deflate", "other_size", "deflate_be", "lzw", "packbits", "truncated", "missing", "cut_strip", "deflate"]
LIST_STATUS = [0, -2, 0, 0, 0, -1, -1, -1, 0]


@pytest.mark.parametrize("nthreads,chunk", [(1, 0), (0, 0), (4, 3)], ids=["one_thread", "all_threads", "chunks_of_3"])
def test_read_tiffs_deflate_device_equals_host(det, tiff_files, nthreads, chunk):
    """Good Deflate files, one of another size, an LZW file, a PackBits file, a truncated file, a missing path and a file
    whose one Deflate strip is cut, which only the device finds out: statuses and bytes as with deflate="host"."""
    paths, source = tiff_files
    names = [paths[n] for n in LIST]
    det.set_option("tiff_chunk_frames", chunk)
    try:
        frames, status = det.read_tiffs(names, nthreads=nthreads, deflate="device")
        host_frames, host_status = det.read_tiffs(names, nthreads=nthreads, deflate="host")
    finally:
        det.set_option("tiff_chunk_frames", 0)
    assert status.tolist() == LIST_STATUS and host_status.tolist() == LIST_STATUS
    got, want = frames.cpu().numpy(), host_frames.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (len(LIST), H0, W0) and np.array_equal(got, want)
    for f, name in enumerate(LIST):
        if LIST_STATUS[f] == 0:
            assert np.array_equal(got[f], source[name]) and np.array_equal(got[f], mrgingham_amd.read_image(paths[name])), name
        else:
            assert not got[f].any(), name
    assert mrgingham_amd.read_image(paths["cut_strip"]) is None


def test_read_tiffs_leaves_the_option_as_it_was(det, tiff_files):
    """deflate= holds for its call; without it the detector's option decides (the cut strip tells: both routes refuse it,
    so the bytes are the yardstick, and the option's value is read back from what the call leaves behind)."""
    paths, source = tiff_files
    names = [paths["deflate"], paths["cut_strip"]]
    for before in (1, 0):
        det.set_option("tiff_deflate", before)
        try:
            for deflate in ("host", "device", None):
                frames, status = det.read_tiffs(names, deflate=deflate)
                assert status.tolist() == [0, -1] and np.array_equal(frames[0].cpu().numpy(), source["deflate"])
                assert det._options["tiff_deflate"] == before
        finally:
            det.set_option("tiff_deflate", 0)


def test_a_strip_above_tiff_deflate_max_strip_keeps_the_host_threads(det, tiff_files):
    paths, source = tiff_files
    det.set_option("tiff_deflate_max_strip", 4 * W0 - 1)            # the file's strips decode to 4 * W0 bytes
    try:
        frames, status = det.read_tiffs([paths["deflate"], paths["deflate_be"], paths["cut_strip"]], deflate="device")
    finally:
        det.set_option("tiff_deflate_max_strip", 8 << 10)               # (the default)
    assert status.tolist() == [0, 0, -1]
    assert np.array_equal(frames[0].cpu().numpy(), source["deflate"]) and np.array_equal(frames[1].cpu().numpy(), source["deflate_be"])
    det.set_option("tiff_deflate_max_strip", 0)                     # no Deflate file is taken
    try:
        frames, status = det.read_tiffs([paths["deflate"]], deflate="device")
    finally:
        det.set_option("tiff_deflate_max_strip", 8 << 10)               # (the default)
    assert status.tolist() == [0] and np.array_equal(frames[0].cpu().numpy(), source["deflate"])


# ---- find_boards_files ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def board_files(tmp_path_factory):
    files = files_cases.write_all(tmp_path_factory.mktemp("files"))
    board = files_cases.board_pixels()
    d = os.path.dirname(files["board.pgm"])

    def put(name, img, **kw):
        files[name] = os.path.join(d, name)
        tc.write(files[name], img, **kw)
    put("board_deflate.tif", board, compression=tc.ADOBE_DEFLATE, predictor=2, rows_per_strip=16)
    put("board_deflate_be.tif", board, compression=tc.DEFLATE, order=">", predictor=2, rows_per_strip=16, reverse=True, odd=True)
    put("board_deflate_8rows.tif", board, compression=tc.ADOBE_DEFLATE, predictor=2, rows_per_strip=8)   # (strips below the default limit)
    put("board16_deflate_4rows.tif", board.astype(np.uint16) * 257, compression=tc.DEFLATE, predictor=2, rows_per_strip=4)
    put("board_lzw.tif", board, compression=tc.LZW, rows_per_strip=16)
    put("board_packbits.tif", board, compression=tc.PACKBITS)
    put("board16_deflate.tif", board.astype(np.uint16) * 257, compression=tc.ADOBE_DEFLATE, predictor=2, order=">", rows_per_strip=16)
    paths = [files["board_deflate.tif"], files["board.pgm"], files["board_lzw.tif"], files[files_cases.BOARD], files["board16_deflate.tif"],
             files["board16.pgm"], files["board_deflate_be.tif"], files["missing"], files["board_packbits.tif"], files["board_deflate_8rows.tif"],
             files["board16_deflate_4rows.tif"], files["board_deflate.tif"]]
    return files, paths


@pytest.fixture(scope="module")
def board_runs(board_files, tmp_path_factory):
    _, paths = board_files
    runs = [{"id": where, "paths": paths, "kw": {"batch": 4, "nthreads": 4, "tiff": "device", "deep": "chunks", "tiff_deflate": where}}
            for where in ("host", "device")]
    return run_child(str(tmp_path_factory.mktemp("board_runs")), {"runs": runs})


def test_find_boards_files_deflate_device_equals_host_and_the_same_pixels_as_pgm(board_files, board_runs):
    """The board is 640 x 480, so the files of 16 rows per strip decode to 10240 (16 bit: 20480) bytes a strip, above the 8 KiB
    default of "tiff_deflate_max_strip": the loader's host threads inflate them in the "device" run as in the "host" run, and
    for them the comparison between the runs holds trivially.  Only board_deflate_8rows.tif and board16_deflate_4rows.tif
    (5120 bytes a strip) reach the inflate kernel here, and in the tool test below."""
    files, paths = board_files
    out = board_runs
    for what in ("status", "found", "levels"):
        assert np.array_equal(out[f"device_{what}"], out[f"host_{what}"]), what
    assert np.array_equal(out["device_boards"], out["host_boards"], equal_nan=True)
    pgm8, pgm16 = paths.index(files["board.pgm"]), paths.index(files["board16.pgm"])
    for rid in ("host", "device"):
        assert out[rid + "_status"].tolist() == [0 if "missing" not in p else -1 for p in paths]
        assert out[rid + "_found"][pgm8] >= 0 and out[rid + "_found"][pgm16] >= 0          # (the files bear boards)
        for i, p in enumerate(paths):
            if not p.endswith(".tif"):
                continue
            ref = pgm16 if "board16" in p else pgm8
            assert out[rid + "_found"][i] == out[rid + "_found"][ref], (rid, p)
            assert np.array_equal(out[rid + "_boards"][i], out[rid + "_boards"][ref]), (rid, p)     # double for double
            assert np.array_equal(out[rid + "_levels"][i], out[rid + "_levels"][ref]), (rid, p)
        stats = dict(zip(STATS, out[rid + "_stats"]))
        assert stats["files_device_loader"] + stats["files_host_decoded"] + stats["files_one_image"] + stats["files_unreadable"] == len(paths)
        assert stats["files_unreadable"] == 1 and stats["files_one_image"] == 0


def test_tool_prints_the_same_vnlog_with_and_without_tiff_deflate_device(board_files, tmp_path):
    files, _ = board_files
    names = ["board_deflate", "board_deflate_be", "board_deflate_8rows", "board_lzw", "board_packbits", "board16_deflate", "board16_deflate_4rows"]
    tifs = [files[n + ".tif"] for n in names]

    def records(r):
        assert r.returncode == 0, r.stderr
        order, rec, _ = parse_vnlog(r.stdout)
        assert order == tifs
        return [[line.split(" ", 1)[1] for line in rec[p]] for p in tifs]
    want = records(run_tool("--jobs", "4", "--batch", "64", "--tiff-lzw", "device", "--deep-batch", "chunks", *tifs))
    assert all(len(r) == 100 for r in want)
    assert records(run_tool("--jobs", "4", "--batch", "64", "--tiff-lzw", "device", "--tiff-deflate", "device", "--deep-batch", "chunks", *tifs)) == want
    r = run_tool("--batch", "64", "--tiff-deflate", "device", *tifs)
    assert r.returncode == 1 and "--tiff-deflate device is only accepted with --tiff-lzw device" in r.stderr
