"""PNG files into device frames (Detector.png_reconstruct, Detector.read_pngs, find_boards_files(png="device"), the
tool's --png-reconstruct): the row filters undone and colour reduced to grey on the device.  PNG is lossless, so the
yardstick is the array the test wrote into the file (tests/png_cases.py; the grey formula in numpy for colour), and
read_image for 8-bit files.  No tolerance anywhere.

The shapes sit on the seams of the kernel's schedule: R rows in flight and segments of S pixels
(mrgingham_amd.png_reconstruct_geometry).  Nothing is larger than about 4200 x 520."""
import os

import numpy as np
import pytest

import mrgingham_amd
from tests import files_cases, png_cases
from tests.test_gpu_files import CLI, STATS, assert_equals_reference, parse_vnlog, run_child, run_tool

pytestmark = pytest.mark.gpu

R, S = mrgingham_amd.png_reconstruct_geometry()
WIDTHS = (1, S - 1, S, S + 1, 2 * S + 3)
HEIGHTS = (1, 2, R - 1, R, R + 1, 2 * R + 5)
FILTERS = ("rotate", ("random", 1), ("random", 2), 0, 1, 2, 3, 4)


def _cases():
    cases = []
    # every width against every height; pixel sizes and filter patterns take turns (8 of each, coprime strides: all
    # six bpp values, the rotation, both seeds and every fixed type come up)
    n = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            cases.append((w, h) + png_cases.TAKEN[n % 8] + (FILTERS[(3 * n + n // 8) % 8],))
            n += 1
    # every filter type on row 0 (the row above is zero) and on the first bpp bytes of a row, at every bpp; then one
    # type on all rows of more than one round, for each of the five
    for ft in range(5):
        for ct, bits in png_cases.TAKEN:
            cases.append((S + 1, 1, ct, bits, ft))
        cases.append((2 * S + 3, R + 1, png_cases.TAKEN[ft][0], png_cases.TAKEN[ft][1], ft))
        cases.append((S - 1, 2 * R + 5, png_cases.TAKEN[7 - ft][0], png_cases.TAKEN[7 - ft][1], ft))
    # fewer segments than rows in flight, and more
    for ct, bits in ((2, 8), (0, 16), (6, 16)):
        cases.append((3, 2 * R + 5, ct, bits, ("random", 3)))
    for ct, bits in ((0, 8), (2, 8), (6, 16)):
        cases.append(((R + 2) * S + 1, 3, ct, bits, "rotate"))
    return cases


def _id(case):
    w, h, ct, bits, filters = case
    f = filters if isinstance(filters, (int, str)) else f"random{filters[1]}"
    return f"{w}x{h}_type{ct}_{bits}bit_{f}"


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector()
    yield d
    d.close()


def _reconstruct(det, imgs, ct, bits, filters, out=None):
    import torch
    scan = np.stack([png_cases.scanlines(img, ct, bits, f) for img, f in zip(imgs, filters)])
    h, w = imgs[0].shape[:2]
    got = det.png_reconstruct(torch.from_numpy(scan).cuda(), h, w, bits, ct, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_kernel_equals_the_source_array(det, case):
    w, h, ct, bits, filters = case
    img = png_cases.random_image(w, h, ct, bits, seed=w + h)
    got = _reconstruct(det, [img], ct, bits, [filters])
    assert got.dtype == (np.uint8 if bits == 8 else np.uint16) and got.shape == (1, h, w)
    assert np.array_equal(got[0], png_cases.grey_of(img, ct))


def test_the_cases_cover_what_they_should():
    cases = _cases()
    assert {png_cases.bpp_of(c[2], c[3]) for c in cases} == {1, 2, 3, 4, 6, 8}
    assert {(c[0], c[1]) for c in cases} >= {(w, h) for w in WIDTHS for h in HEIGHTS}
    assert {c[4] for c in cases} >= {"rotate", ("random", 1), ("random", 2), 0, 1, 2, 3, 4}
    for ft in range(5):                                            # row 0 under every filter type, at every bpp
        assert {png_cases.bpp_of(c[2], c[3]) for c in cases if png_cases.row_filters(c[1], c[4])[0] == ft} == {1, 2, 3, 4, 6, 8}
        assert any(c[4] == ft and c[1] > R for c in cases)         # ... and one type on all rows of more than one round


@pytest.mark.parametrize("ct,bits", [(2, 8), (4, 16)])
def test_a_batch_whose_filter_patterns_differ_per_frame(det, ct, bits):
    w, h = 2 * S + 3, R + 1
    imgs = [png_cases.random_image(w, h, ct, bits, seed=10 + f) for f in range(5)]
    got = _reconstruct(det, imgs, ct, bits, ["rotate", ("random", 5), 4, ("random", 6), 3])
    for f in range(5):
        assert np.array_equal(got[f], png_cases.grey_of(imgs[f], ct)), f


@pytest.mark.parametrize("ct,bits", [(2, 8), (0, 8), (6, 16)])
def test_strided_output_leaves_everything_else_alone(det, ct, bits):
    import torch
    w, h, stride, rows = 2 * S + 3, R + 1, 2 * S + 3 + 7, R + 1 + 2
    imgs = [png_cases.random_image(w, h, ct, bits, seed=20 + f) for f in range(3)]
    dtype, sentinel = (torch.uint8, 0xA5) if bits == 8 else (torch.uint16, 0xA5A5)
    big = torch.full((3, rows, stride), sentinel, dtype=dtype, device="cuda")
    _reconstruct(det, imgs, ct, bits, ["rotate", 4, ("random", 2)], out=big[:, :h, :])
    back = big.cpu().numpy()
    for f in range(3):
        assert np.array_equal(back[f, :h, :w], png_cases.grey_of(imgs[f], ct)), f
    assert (back[:, :h, w:] == sentinel).all() and (back[:, h:, :] == sentinel).all()


def test_bad_arguments_are_refused_with_nothing_written(det):
    import torch
    w, h, ct, bits = S + 1, 5, 2, 8
    img = png_cases.random_image(w, h, ct, bits)
    scan = torch.from_numpy(np.concatenate([png_cases.scanlines(img, ct, bits).reshape(-1), np.zeros(8, np.uint8)])).cuda()
    out = torch.full((h, w), 0x5A, dtype=torch.uint8, device="cuda")
    pitch = (w * 3 + 1) * h

    def call(d_scan=None, scan_pitch=pitch, n=1, width=w, height=h, bits=bits, ct=ct, d_out=None, frame_pitch=w * h, stride=w, ctx=None):
        return det.L.mrgingham_amd_png_reconstruct_batch(det.ctx if ctx is None else ctx, scan.data_ptr() if d_scan is None else d_scan,
                                                         scan_pitch, n, width, height, bits, ct, out.data_ptr() if d_out is None else d_out,
                                                         frame_pitch, stride, None)
    bad = [dict(n=-1), dict(width=-1), dict(height=-1), dict(stride=w - 1), dict(frame_pitch=-1), dict(scan_pitch=pitch - 1),
           dict(bits=12), dict(bits=4), dict(ct=3), dict(ct=1), dict(ct=7), dict(d_scan=scan.data_ptr() + 1), dict(d_scan=0),
           dict(d_out=0), dict(width=32768, stride=32768, scan_pitch=1 << 40), dict(height=32768, scan_pitch=1 << 40)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert det.L.mrgingham_amd_png_reconstruct_batch(None, scan.data_ptr(), pitch, 1, w, h, bits, ct, out.data_ptr(), w * h, w, None) == -1
    out16 = torch.zeros(w * h + 1, dtype=torch.uint16, device="cuda")
    assert call(bits=16, ct=0, scan_pitch=(w * 2 + 1) * h + 64, d_out=out16.data_ptr() + 1) == -1      # 16-bit frames at an odd address
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A).all()
    assert call(n=0) == 0 and call(width=0, stride=0) == 0                                      # nothing to do is not an error
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), png_cases.grey_of(img, ct))


# ---- read_pngs --------------------------------------------------------------------------------------------------------
W0, H0 = 37, 29


def _palette_case(w, h, seed=5):
    rng = np.random.default_rng(seed)
    palette = rng.integers(0, 256, (40, 3)).astype(np.uint8)
    return rng.integers(0, 40, (h, w)).astype(np.uint8), palette


@pytest.fixture(scope="module")
def png_files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pngs"))
    paths, source = {}, {}

    def put(name, img, ct, bits, **kw):
        paths[name] = os.path.join(d, name + ".png")
        png_cases.write(paths[name], img, ct, bits, **kw)
        source[name] = None if ct == 3 else png_cases.grey_of(img, ct)
    for k, (ct, bits) in enumerate(png_cases.TAKEN):
        put(f"type{ct}_{bits}", png_cases.random_image(W0, H0, ct, bits, seed=30 + k), ct, bits, filters=("random", k), nidat=1 + k % 3)
    idx, palette = _palette_case(W0, H0)
    put("palette", idx, 3, 8, palette=palette)
    put("other_size", png_cases.random_image(W0 + 1, H0, 0, 8), 0, 8)
    put("other_size16", png_cases.random_image(W0, H0 + 1, 0, 16), 0, 16)
    paths["truncated"] = os.path.join(d, "truncated.png")
    with open(paths["truncated"], "wb") as f:
        f.write(open(paths["type2_8"], "rb").read()[:-40])
    paths["missing"] = os.path.join(d, "missing.png")
    return paths, source


EIGHT = ["type0_8", "type2_8", "type4_8", "type6_8", "palette", "other_size", "type0_16", "truncated", "missing"]
EIGHT_STATUS = [0, 0, 0, 0, 0, -2, -2, -1, -1]
SIXTEEN = ["type0_16", "type2_16", "type2_8", "type4_16", "type6_16", "other_size16", "missing"]
SIXTEEN_STATUS = [0, 0, -2, 0, 0, -2, -1]


@pytest.mark.parametrize("nthreads,chunk", [(1, 0), (0, 0), (4, 2)], ids=["one_thread", "all_threads", "chunks_of_2"])
def test_read_pngs_8bit_list(det, png_files, nthreads, chunk):
    paths, source = png_files
    det.set_option("png_chunk_frames", chunk)                    # 2: a list longer than one internal chunk (five of them)
    try:
        frames, status = det.read_pngs([paths[n] for n in EIGHT], nthreads=nthreads)
    finally:
        det.set_option("png_chunk_frames", 0)
    assert status.tolist() == EIGHT_STATUS
    got = frames.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (len(EIGHT), H0, W0)
    for f, name in enumerate(EIGHT):
        if EIGHT_STATUS[f] == 0:
            assert np.array_equal(got[f], mrgingham_amd.read_image(paths[name])), name
            if source[name] is not None:
                assert np.array_equal(got[f], source[name]), name
        else:
            assert mrgingham_amd.read_image(paths[name]) is None or EIGHT_STATUS[f] == -2
            assert not got[f].any(), name


@pytest.mark.parametrize("nthreads,chunk", [(1, 0), (0, 3)], ids=["one_thread", "chunks_of_3"])
def test_read_pngs_16bit_list(det, png_files, nthreads, chunk):
    paths, source = png_files
    det.set_option("png_chunk_frames", chunk)
    try:
        frames, status = det.read_pngs([paths[n] for n in SIXTEEN], nthreads=nthreads)
    finally:
        det.set_option("png_chunk_frames", 0)
    assert status.tolist() == SIXTEEN_STATUS
    got = frames.cpu().numpy()
    assert got.dtype == np.uint16 and got.shape == (len(SIXTEEN), H0, W0)
    for f, name in enumerate(SIXTEEN):
        if SIXTEEN_STATUS[f] == 0:
            assert np.array_equal(got[f], source[name]), name
        else:
            assert not got[f].any(), name


def test_read_pngs_without_a_readable_header(det, png_files):
    paths, _ = png_files
    frames, status = det.read_pngs([paths["missing"], paths["truncated"][:-4] + "_none.png"])
    assert tuple(frames.shape) == (2, 0, 0) and status.tolist() == [-1, -1]
    frames, status = det.read_pngs([])
    assert tuple(frames.shape) == (0, 0, 0) and len(status) == 0


# ---- find_boards_files ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def board_files(tmp_path_factory):
    files = files_cases.write_all(tmp_path_factory.mktemp("files"))
    board = files_cases.board_pixels()
    d = os.path.dirname(files["board.png"])
    files["board_rgb.png"] = os.path.join(d, "board_rgb.png")          # r = g = b: its grey is the board
    png_cases.write(files["board_rgb.png"], np.stack([board] * 3, axis=-1), 2, 8, filters=("random", 4), nidat=3)
    files["board_palette.png"] = os.path.join(d, "board_palette.png")  # the palette is the grey ramp
    png_cases.write(files["board_palette.png"], board, 3, 8, palette=np.stack([np.arange(256)] * 3, axis=-1))
    paths = files_cases.mixed_list(files)
    paths = paths[:5] + [files["board_rgb.png"]] + paths[5:17] + [files["board_palette.png"]] + paths[17:]
    return files, paths


@pytest.fixture(scope="module")
def board_runs(board_files, tmp_path_factory):
    _, paths = board_files
    runs = [{"id": f"{png}_{batch}", "paths": paths, "kw": {"batch": batch, "nthreads": 4, "png": png}, "ref": True}
            for png in ("host", "device") for batch in (4, 64)]
    return run_child(str(tmp_path_factory.mktemp("board_runs")), {"runs": runs})


@pytest.mark.parametrize("batch", [4, 64])
def test_find_boards_files_png_device_equals_host_and_the_one_image_path(board_files, board_runs, batch):
    files, paths = board_files
    out = board_runs
    for png in ("host", "device"):
        assert_equals_reference(out, f"{png}_{batch}", len(paths))
    for what in ("status", "found", "levels"):
        assert np.array_equal(out[f"device_{batch}_{what}"], out[f"host_{batch}_{what}"]), what
    assert np.array_equal(out[f"device_{batch}_boards"], out[f"host_{batch}_boards"], equal_nan=True)
    found = out[f"device_{batch}_found"]
    assert (found[[i for i, p in enumerate(paths) if os.path.basename(p).startswith("board")]] >= 0).all()   # (the PNG files bear boards)
    ok = out[f"device_{batch}_status"] == 0
    jpgs = sum(1 for p, k in zip(paths, ok) if k and p.endswith(".jpg"))
    pgms = sum(1 for p in paths if p.endswith("board.pgm"))
    device = dict(zip(STATS, out[f"device_{batch}_stats"]))
    host = dict(zip(STATS, out[f"host_{batch}_stats"]))
    assert device["files_device_loader"] == jpgs + sum(1 for p in paths if p.endswith(("board.png", "board_rgb.png")))
    assert device["files_host_decoded"] == pgms + sum(1 for p in paths if p.endswith("board_palette.png"))
    assert host["files_device_loader"] == jpgs
    assert host["files_host_decoded"] == pgms + sum(1 for p in paths if p.endswith(".png"))
    for stats in (device, host):
        assert stats["files_one_image"] == sum(1 for p in paths if p.endswith("board16.pgm"))
        assert stats["files_device_loader"] + stats["files_host_decoded"] + stats["files_one_image"] + stats["files_unreadable"] == len(paths)


def test_tool_png_reconstruct_device_prints_the_same_vnlog(board_files):
    files, paths = board_files
    readable = [p for p in dict.fromkeys(paths) if "missing" not in p and "progressive" not in p]
    host = run_tool("--jobs", "4", "--batch", "8", *readable)
    device = run_tool("--jobs", "4", "--batch", "8", "--png-reconstruct", "device", *readable)
    assert host.returncode == 0 and device.returncode == 0, host.stderr + device.stderr
    order, records, comments = parse_vnlog(device.stdout)
    assert (order, records) == parse_vnlog(host.stdout)[:2]          # (the comments name the command line)
    assert comments[-1] == "# filename x y level"
    assert order == readable and len(records[files["board_rgb.png"]]) == 100 and os.access(CLI, os.X_OK)
