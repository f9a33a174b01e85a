"""Baseline JPEG on the device: the inverse-DCT kernel (mrgingham_amd_jpeg_idct_batch) against the fixtures of
tests/golden/jpeg_golden.npz and against the numpy restatement of its arithmetic, the batch loader
(mrgingham_amd_read_jpegs_batch) against the host decoder, and a .jpg through the detector and the tool.  Every
comparison is byte equality."""
import ctypes
import os

import numpy as np
import pytest

import mrgingham_amd
from test_cli import _parse, _run, _write_pgm
from test_jpeg_io import case, cases, idct_blocks, plane_of

pytestmark = pytest.mark.gpu

ERR_ARG = -1


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector()
    yield d
    d.close()


def _dev(det, a):
    t = det.torch
    if a.dtype == np.uint16:                                       # (moved as its int16 image: the same bits)
        return t.from_numpy(a.view(np.int16).copy()).to(det.device).view(t.uint16)
    return t.from_numpy(np.ascontiguousarray(a)).to(det.device)


def _idct_of_case(det, c, **kw):
    coef, quant, (h, w) = mrgingham_amd.jpeg_coefficients(c.data)
    return det.jpeg_idct(_dev(det, coef[None]), _dev(det, quant[None]), h, w, **kw)


@pytest.mark.parametrize("prefix", ["noise_8x8_grey",            # one block
                                    "noise_17x9_grey",           # cut in x and in y
                                    "noise_17x9_420",
                                    "noise_31x33_420",           # blocks_* padded past ceil(side / 8)
                                    "sof1_patched_31x33_420",
                                    "noise_264x16_420",          # 33 blocks per row (34 stored): across the seam of a workgroup
                                    "noise_520x8_grey",          # 65 blocks per row: three workgroups
                                    "qtable16_53x37_grey",
                                    "board_640x480_grey"])
def test_jpeg_idct_equals_libjpeg_on_fixtures(det, prefix):
    c = case(prefix)
    got = _idct_of_case(det, c).cpu().numpy()
    assert got.shape == (1,) + c.luma.shape and np.array_equal(got[0], c.luma)


def test_jpeg_idct_on_every_fixture(det):
    for c in cases():
        if c.readable:
            assert np.array_equal(_idct_of_case(det, c).cpu().numpy()[0], c.luma), c.name


def test_jpeg_idct_batch_of_three_tables(det):
    three = [case("noise_48x64_grey"), case("noise_48x64_444"), case("noise_48x64_420")]
    parts = [mrgingham_amd.jpeg_coefficients(c.data) for c in three]
    assert all(p[0].shape == (8, 6, 64) for p in parts)
    quant = np.stack([p[1] for p in parts])
    assert len({q.tobytes() for q in quant}) == 3                   # three different tables
    got = det.jpeg_idct(_dev(det, np.stack([p[0] for p in parts])), _dev(det, quant), 64, 48).cpu().numpy()
    for f, c in enumerate(three):
        assert np.array_equal(got[f], c.luma), c.name


@pytest.mark.parametrize("prefix", ["noise_17x9_420", "noise_53x37_444", "noise_264x16_420"])
def test_jpeg_idct_leaves_the_bytes_between_width_and_stride(det, prefix):
    t = det.torch
    c = case(prefix)
    h, w = c.luma.shape
    full = t.full((1, h, w + 3), 0xA5, dtype=t.uint8, device=det.device)
    view = _idct_of_case(det, c, out=full)
    assert view.data_ptr() == full.data_ptr()
    got = full.cpu().numpy()
    assert np.array_equal(got[0, :, :w], c.luma) and (got[0, :, w:] == 0xA5).all()
    # ... and what lies behind the last frame row (a buffer with room after it)
    flat = t.full((h * w + 64,), 0x5A, dtype=t.uint8, device=det.device)
    _idct_of_case(det, c, out=flat[:h * w].view(1, h, w))
    assert (flat[h * w:].cpu().numpy() == 0x5A).all() and np.array_equal(flat[:h * w].cpu().numpy().reshape(h, w), c.luma)


def test_jpeg_idct_wraps_like_the_numpy_restatement_on_crafted_input(det):
    rng = np.random.RandomState(5)
    coef = rng.randint(-32768, 32768, size=(2, 4, 8, 64)).astype(np.int16)         # 64 blocks of anything
    coef[0, 0, 0, :4] = [-32768, 32767, -32768, 32767]
    quant = rng.randint(0, 65536, size=(2, 64)).astype(np.uint16)
    quant[0, :4] = [65535, 65535, 1, 0]
    got = det.jpeg_idct(_dev(det, coef), _dev(det, quant), 32, 64).cpu().numpy()
    for f in range(2):
        assert np.array_equal(got[f], plane_of(coef[f], quant[f], 32, 64)), f
    assert got.min() == 0 and got.max() == 255 and len(np.unique(got)) > 2          # (wrapped sums mostly saturate; not all do)


def test_jpeg_idct_dc_only_blocks_saturate(det):
    """DC-only blocks give flat planes.  +-2047 x 16 stays inside 32 bits and saturates the way libjpeg does: all 255 /
    all 0.  +-2047 x 255 does not: d0 << 13 = +-4.28e9 leaves int32, and under the modulo-2^32 rule of the transform the
    planes are still all 0 / all 255, with the signs exchanged -- on the device exactly as in the numpy restatement."""
    coef = np.zeros((4, 1, 3, 64), np.int16)
    coef[:, :, :, 0] = np.array([2047, -2047, 2047, -2047], np.int16)[:, None, None]
    quant = np.repeat(np.array([16, 16, 255, 255], np.uint16)[:, None], 64, axis=1)
    got = det.jpeg_idct(_dev(det, coef), _dev(det, quant), 8, 24).cpu().numpy()
    for f, flat in enumerate([255, 0, 0, 255]):
        assert (got[f] == flat).all(), f
        assert (idct_blocks(coef[f], quant[f]) == flat).all(), f


def test_jpeg_idct_argument_errors_write_nothing(det):
    t, L = det.torch, det.L
    coef = t.zeros((1, 2, 2, 64), dtype=t.int16, device=det.device)                 # zero coefficients would give 128
    quant = t.ones((1, 64), dtype=t.int16, device=det.device)
    out = t.full((1, 16, 16), 7, dtype=t.uint8, device=det.device)

    def call(coef_p=coef.data_ptr(), pitch=256, quant_p=quant.data_ptr(), n=1, w=16, h=16, bw=2, bh=2, out_p=out.data_ptr(),
             fp=256, stride=16, ctx=det.ctx):
        return L.mrgingham_amd_jpeg_idct_batch(ctx, coef_p, pitch, quant_p, n, w, h, bw, bh, out_p, fp, stride, None)

    for bad in (dict(w=-1), dict(h=-16), dict(n=-1), dict(bw=1), dict(bh=1), dict(w=17), dict(stride=15), dict(coef_p=None),
                dict(quant_p=None), dict(out_p=None), dict(ctx=None), dict(pitch=255), dict(pitch=128), dict(fp=-1),
                dict(w=40000, bw=5000, stride=40000), dict(coef_p=coef.data_ptr() + 2)):
        assert call(**bad) == ERR_ARG, bad
    t.cuda.synchronize()
    assert (out == 7).all()
    assert call() == 0
    t.cuda.synchronize()
    assert (out == 128).all()
    assert call(n=0) == 0 and call(w=0, h=0) == 0


@pytest.fixture(scope="module")
def seven_files(tmp_path_factory):
    """Five 48 x 64 fixtures with a progressive file and a file of another size in the middle."""
    d = tmp_path_factory.mktemp("jpegs")
    picks = [case("noise_48x64_grey"), case("checker_48x64_444"), case("progressive_48x64"), case("noise_48x64_422"),
             case("noise_16x16_444"), case("noise_48x64_420"), case("white_48x64_420")]
    paths = []
    for i, c in enumerate(picks):
        p = str(d / f"{i}_{c.name}.jpg")
        with open(p, "wb") as f:
            f.write(c.data)
        paths.append(p)
    return paths


@pytest.mark.parametrize("nthreads", [1, 4])
@pytest.mark.parametrize("chunk", [0, 1, 2, 3])
def test_read_jpegs_statuses_zero_fill_and_host_parity(det, seven_files, chunk, nthreads):
    det.set_option("jpeg_chunk_frames", chunk)
    try:
        frames, status = det.read_jpegs(seven_files, nthreads=nthreads)
    finally:
        det.set_option("jpeg_chunk_frames", 0)
    assert status.dtype == np.int32 and status.tolist() == [0, 0, -1, 0, -2, 0, 0]
    got = frames.cpu().numpy()
    assert got.shape == (7, 64, 48)
    for f, p in enumerate(seven_files):
        if status[f] != 0:
            assert (got[f] == 0).all(), f
        else:
            assert np.array_equal(got[f], mrgingham_amd.read_image(p)), p


def test_read_jpegs_loader_boundary(det, seven_files):
    t, L = det.torch, det.L
    before = det.scratch_bytes()
    out = t.full((2, 64, 48 + 5), 9, dtype=t.uint8, device=det.device)               # strided frames, sentinel columns
    names = (ctypes.c_char_p * 2)(os.fsencode(seven_files[0]), os.fsencode(str(seven_files[0]) + ".missing"))
    status = np.full(2, 5, np.int32)
    args = (names, 2, 48, 64, out.data_ptr(), 64 * 53, 53, 2, status.ctypes.data)
    assert L.mrgingham_amd_read_jpegs_batch(det.ctx, *args) == 0
    got = out.cpu().numpy()
    assert status.tolist() == [0, -1] and (got[:, :, 48:] == 9).all() and (got[1, :, :48] == 0).all()
    assert np.array_equal(got[0, :, :48], case("noise_48x64_grey").luma)
    assert det.scratch_bytes() >= before and det.scratch_bytes() > 0                  # the coefficient buffers are counted
    for bad in ((names, -1, 48, 64, out.data_ptr(), 64 * 53, 53, 2, status.ctypes.data),
                (names, 2, 0, 64, out.data_ptr(), 64 * 53, 53, 2, status.ctypes.data),
                (names, 2, 48, 64, out.data_ptr(), 64 * 53, 47, 2, status.ctypes.data),
                (None, 2, 48, 64, out.data_ptr(), 64 * 53, 53, 2, status.ctypes.data),
                (names, 2, 48, 64, None, 64 * 53, 53, 2, status.ctypes.data),
                (names, 2, 48, 64, out.data_ptr(), 64 * 53, 53, 2, None)):
        assert L.mrgingham_amd_read_jpegs_batch(det.ctx, *bad) == ERR_ARG
    assert L.mrgingham_amd_read_jpegs_batch(None, *args) == ERR_ARG
    out.fill_(9)                                                                      # a NULL entry in the list: refused up front
    status[:] = 5
    holed = (ctypes.c_char_p * 2)(os.fsencode(seven_files[0]), None)
    assert L.mrgingham_amd_read_jpegs_batch(det.ctx, holed, *args[1:]) == ERR_ARG
    assert (out == 9).all() and status.tolist() == [5, 5]
    frames, st = det.read_jpegs([str(seven_files[0]) + ".missing"])
    assert tuple(frames.shape) == (1, 0, 0) and st.tolist() == [-1]


def test_board_jpeg_through_the_detector_and_the_tool(det, tmp_path):
    c = case("board_640x480")
    f = str(tmp_path / "board.jpg")
    with open(f, "wb") as fh:
        fh.write(c.data)
    frames, status = det.read_jpegs([f] * 4)
    assert status.tolist() == [0, 0, 0, 0]
    boards, found = det.find_boards(frames)
    host = mrgingham_amd.read_image(f)
    want = mrgingham_amd.find_board(host)
    assert want is not None and want.shape == (100, 2)
    assert (found >= 0).all()
    for k in range(4):
        assert np.array_equal(boards[k], want), k                                     # double for double
    pgm = str(tmp_path / "board.pgm")
    _write_pgm(pgm, host)
    a, b = _run(f), _run(pgm)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout.splitlines()[1:] == [ln.replace(pgm, f) for ln in b.stdout.splitlines()[1:]]   # ([0]: the command line)
    assert len(_parse(a.stdout)[f]) == 100
