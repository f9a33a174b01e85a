"""Restart intervals Huffman-decoded on the device, one lane each (csrc/jpeg_huff.hip: mrgingham_amd_jpeg_entropy_batch and
mrgingham_amd_read_jpegs_batch under option "jpeg_entropy"), against the host decoder on the fixtures of
tests/golden/jpeg_rst_golden.npz and jpeg_golden.npz and on the corruptions of test_jpeg_scan.py.  Every comparison is
equality."""
import ctypes
import os

import numpy as np
import pytest

import mrgingham_amd
from test_jpeg_io import case, cases
from test_jpeg_scan import corruptions, rst_case, rst_cases

pytestmark = pytest.mark.gpu

ERR_ARG = -1


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector()
    yield d
    d.close()


def _padded(side):
    return max(-(-side // (8 * h)) * h for h in (1, 2, 3, 4))


def _check_decoded(coef, quant, f, data, name):
    want, wq, _ = mrgingham_amd.jpeg_coefficients(data)
    bh, bw = want.shape[:2]
    assert np.array_equal(coef[f, :bh, :bw], want), name
    assert np.array_equal(quant[f], wq), name


def _quant_np(det, quant):
    return quant.view(det.torch.int16).cpu().numpy().view(np.uint16)


def _groups():
    """Every fixture of both files that has restart intervals, by size: {(h, w): [case]}; the 48 x 64 group also gets the
    file without DRI, the progressive file and a 16 x 16 file."""
    out = {}
    for c in cases() + rst_cases():
        if c.readable and mrgingham_amd.jpeg_restart_intervals(c.data)[0]:
            out.setdefault((c.height, c.width), []).append(c)
    out[(64, 48)] += [rst_case("nodri_48x64"), case("progressive_48x64"), case("noise_16x16_444")]
    return out


@pytest.mark.parametrize("memset", [0, 1])
def test_jpeg_entropy_equals_the_host_decoder_on_every_dri_fixture(det, memset):
    groups = _groups()
    special = {"nodri_48x64": -3, "progressive_48x64": -1, "noise_16x16": -2}
    assert len(groups) >= 9 and sum(len(g) for g in groups.values()) >= 15 + 20 + 3
    det.set_option("jpeg_entropy_memset", memset)
    try:
        for (h, w), group in groups.items():
            coef, quant, status = det.jpeg_entropy([c.data for c in group], h, w)
            assert tuple(coef.shape) == (len(group), _padded(h), _padded(w), 64) and status.dtype == np.int32
            coef, quant = coef.cpu().numpy(), _quant_np(det, quant)
            for f, c in enumerate(group):
                want = next((v for k, v in special.items() if (h, w) == (64, 48) and c.name.startswith(k)), 0)
                assert status[f] == want, (c.name, status[f])
                if want == 0:
                    _check_decoded(coef, quant, f, c.data, c.name)
                else:
                    assert not coef[f].any() and not quant[f].any(), c.name
    finally:
        det.set_option("jpeg_entropy_memset", 0)
    assert (64, 48) in groups and [c.name[:5] for c in groups[(64, 48)][-3:]] == ["nodri", "progr", "noise"]


def test_jpeg_entropy_max_interval_routes_longer_intervals_to_the_host(det):
    three = [rst_case("noise_31x33_420"), rst_case("noise_53x37_420"), rst_case("noise_264x16_420")]
    assert [mrgingham_amd.jpeg_restart_intervals(c.data)[0] for c in three] == [4, 5, 7]
    one = rst_case("noise_31x33_422")                                         # DRI 1 passes any limit
    for c in three:
        det.set_option("jpeg_entropy_max_interval", 1)
        try:
            coef, quant, status = det.jpeg_entropy([c.data], c.height, c.width)
            assert status.tolist() == [-3] and not coef.any().item(), c.name
            if c.height == one.height:
                assert det.jpeg_entropy([one.data], one.height, one.width)[2].tolist() == [0]
        finally:
            det.set_option("jpeg_entropy_max_interval", 1024)
        coef, quant, status = det.jpeg_entropy([c.data], c.height, c.width)
        assert status.tolist() == [0], c.name
        _check_decoded(coef.cpu().numpy(), _quant_np(det, quant), 0, c.data, c.name)
    with pytest.raises(ValueError):
        det.set_option("jpeg_entropy_max_interval", 0)
    with pytest.raises(ValueError):
        det.set_option("jpeg_entropy", 2)


@pytest.fixture(scope="module")
def mixed_files(tmp_path_factory):
    """48 x 64: restart intervals in three samplings, a file without them, a progressive file, a 16 x 16 file, a missing path."""
    d = tmp_path_factory.mktemp("jpegs_rst")
    picks = [rst_case("noise_48x64_grey"), rst_case("noise_48x64_444_q100"), rst_case("nodri_48x64"), case("progressive_48x64"),
             rst_case("rows_48x64_420"), case("noise_16x16_444"), rst_case("optimize_48x64_420"), rst_case("black_48x64")]
    paths = []
    for i, c in enumerate(picks):
        p = str(d / f"{i}_{c.name}.jpg")
        with open(p, "wb") as f:
            f.write(c.data)
        paths.append(p)
    paths.insert(5, str(d / "missing.jpg"))
    picks.insert(5, None)
    return paths, picks


@pytest.fixture(scope="module")
def host_frames(det, mixed_files):
    frames, status = det.read_jpegs(mixed_files[0], nthreads=2)
    return frames.cpu().numpy(), status


@pytest.mark.parametrize("nthreads", [1, 4])
@pytest.mark.parametrize("chunk", [0, 1, 2, 3])
def test_read_jpegs_device_entropy_equals_host_entropy(det, mixed_files, host_frames, chunk, nthreads):
    paths, picks = mixed_files
    det.set_option("jpeg_chunk_frames", chunk)
    try:
        frames, status = det.read_jpegs(paths, nthreads=nthreads, entropy="device")
    finally:
        det.set_option("jpeg_chunk_frames", 0)
    assert det._options["jpeg_entropy"] == 0                                   # restored
    want = [0, 0, 0, -1, 0, -1, -2, 0, 0]
    assert status.dtype == np.int32 and status.tolist() == want == host_frames[1].tolist()
    got = frames.cpu().numpy()
    assert got.shape == (9, 64, 48) and np.array_equal(got, host_frames[0])
    for f, c in enumerate(picks):
        assert np.array_equal(got[f], c.luma) if want[f] == 0 else not got[f].any(), f


def test_read_jpegs_device_entropy_loader_boundary(det, mixed_files):
    t, L = det.torch, det.L
    paths, _ = mixed_files
    out = t.full((3 * 64 * 53 + 64,), 9, dtype=t.uint8, device=det.device)           # strided frames, sentinel columns, room behind
    names = (ctypes.c_char_p * 3)(os.fsencode(paths[0]), os.fsencode(paths[5]), os.fsencode(paths[4]))
    status = np.full(3, 5, np.int32)
    det.set_option("jpeg_entropy", 1)
    try:
        assert L.mrgingham_amd_read_jpegs_batch(det.ctx, names, 3, 48, 64, out.data_ptr(), 64 * 53, 53, 2, status.ctypes.data) == 0
        assert L.mrgingham_amd_read_jpegs_batch(det.ctx, None, 3, 48, 64, out.data_ptr(), 64 * 53, 53, 2, status.ctypes.data) == ERR_ARG
    finally:
        det.set_option("jpeg_entropy", 0)
    got = out.cpu().numpy()
    assert (got[3 * 64 * 53:] == 9).all()
    got = got[:3 * 64 * 53].reshape(3, 64, 53)
    assert status.tolist() == [0, -1, 0] and (got[:, :, 48:] == 9).all() and (got[1, :, :48] == 0).all()
    assert np.array_equal(got[0, :, :48], rst_case("noise_48x64_grey").luma)
    assert np.array_equal(got[2, :, :48], rst_case("rows_48x64_420").luma)


@pytest.mark.parametrize("prefix", ["noise_136x136_grey", "noise_31x33_420"])
def test_corrupted_intervals_cost_a_status_and_agree_with_the_host(det, prefix):
    """The corruptions test_jpeg_scan.py runs through the same decoder text on the host, in ONE device call per fixture:
    the device accepts exactly the files the host decoder accepts, with the same coefficients."""
    c = rst_case(prefix)
    datas = [c.data] + [d for _, d in corruptions(c)]
    host = [mrgingham_amd.jpeg_coefficients(d) for d in datas]
    host = [r if r is not None and r[2] == (c.height, c.width) else None for r in host]      # (the size bytes are not touched)
    coef, quant, status = det.jpeg_entropy(datas, c.height, c.width)
    assert set(status.tolist()) == {0, -1} and status[0] == 0
    assert np.array_equal(status == 0, np.array([r is not None for r in host]))
    coef, quant = coef.cpu().numpy(), _quant_np(det, quant)
    for f, r in enumerate(host):
        if r is None:
            assert not coef[f].any() and not quant[f].any(), f
        else:
            assert np.array_equal(coef[f, :c.blocks_h, :c.blocks_w], r[0]) and np.array_equal(quant[f], r[1]), f
    assert 0 < (status == 0).mean() < 1


def test_jpeg_entropy_argument_errors_write_nothing(det):
    t, L = det.torch, det.L
    c = rst_case("noise_31x33_422")
    assert (c.blocks_h, c.blocks_w) == (5, 4)                                   # (an area of 8 x 4 blocks holds it)
    coef = t.full((1, 8, 4, 64), 7, dtype=t.int16, device=det.device)
    quant = t.full((1, 64), 7, dtype=t.int16, device=det.device)
    status = np.full(1, 5, np.int32)
    ptrs, sizes = (ctypes.c_char_p * 1)(c.data), (ctypes.c_size_t * 1)(len(c.data))

    def call(ctx=det.ctx, data=ptrs, nbytes=sizes, n=1, w=31, h=33, coef_p=coef.data_ptr(), pitch=8 * 4 * 64, bw=4, bh=8,
             quant_p=quant.data_ptr(), st=status.ctypes.data):
        return L.mrgingham_amd_jpeg_entropy_batch(ctx, data, nbytes, n, w, h, coef_p, pitch, bw, bh, quant_p, st)

    null = (ctypes.c_char_p * 1)(None)
    for bad in (dict(ctx=None), dict(data=None), dict(nbytes=None), dict(n=-1), dict(w=0), dict(h=-33), dict(coef_p=None),
                dict(quant_p=None), dict(st=None), dict(bw=3), dict(bh=4), dict(pitch=8 * 4 * 64 - 8), dict(pitch=8 * 4 * 64 + 4),
                dict(coef_p=coef.data_ptr() + 2), dict(w=40000, bw=5000), dict(data=null)):
        assert call(**bad) == ERR_ARG, bad
    t.cuda.synchronize()
    assert (coef == 7).all() and (quant == 7).all() and status.tolist() == [5]
    assert call(n=0) == 0 and status.tolist() == [5]
    assert call() == 0 and status.tolist() == [0]
    _check_decoded(coef.cpu().numpy(), _quant_np(det, quant.view(t.uint16)), 0, c.data, c.name)
    assert call(w=32) == 0 and status.tolist() == [-2] and not coef.any().item()        # another size: zeroed


def test_board_with_restart_rows_through_the_device_decoder_and_the_detector(det, tmp_path):
    c = rst_case("board_640x480")
    assert mrgingham_amd.jpeg_restart_intervals(c.data)[0] == 80 and len(mrgingham_amd.jpeg_restart_intervals(c.data)[1]) == 60
    f = str(tmp_path / "board_rst.jpg")
    with open(f, "wb") as fh:
        fh.write(c.data)
    frames, status = det.read_jpegs([f] * 4, entropy="device")
    assert status.tolist() == [0, 0, 0, 0]
    host = mrgingham_amd.read_image(f)
    assert np.array_equal(frames[3].cpu().numpy(), host)
    boards, found = det.find_boards(frames)
    want = mrgingham_amd.find_board(host)
    assert want is not None and want.shape == (100, 2) and (found >= 0).all()
    for k in range(4):
        assert np.array_equal(boards[k], want), k                                     # double for double
