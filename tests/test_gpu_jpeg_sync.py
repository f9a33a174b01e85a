"""Files without restart intervals Huffman-decoded on the device by self-synchronising subsequences
(csrc/jpeg_huff_sync.hip: mrgingham_amd_jpeg_entropy_batch and mrgingham_amd_read_jpegs_batch under option "jpeg_sync"),
against the host decoder on the fixtures of the three golden files and on the corruptions of test_jpeg_sync.py.  Every
comparison is equality."""
import json
import os

import numpy as np
import pytest

import mrgingham_amd
from test_jpeg_io import case
from test_jpeg_scan import rst_case
from test_jpeg_sync import REALISTIC, nodri_cases, sync_case, sync_corruptions

pytestmark = pytest.mark.gpu

DEFAULT_SUBSEQUENCE = 128        # the measured choice (profiles/jpeg_sync_bench.json)


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector()
    yield d
    d.close()


@pytest.fixture
def options(det):
    """set(name, value) for the test; the defaults are back afterwards."""
    yield det.set_option
    det.set_option("jpeg_sync_subsequence", DEFAULT_SUBSEQUENCE)
    det.set_option("jpeg_sync_max_rounds", 0)
    det.set_option("jpeg_chunk_frames", 0)


_host = {}


def host_of(data):
    """jpeg_coefficients of a file, computed once."""
    if data not in _host:
        _host[data] = mrgingham_amd.jpeg_coefficients(data)
    return _host[data]


def _quant_np(det, quant):
    return quant.view(det.torch.int16).cpu().numpy().view(np.uint16)


def _check(det, datas, height, width, want_status, **kw):
    """One jpeg_entropy(sync=True) call: the statuses, and per file the host decoder's coefficients and table (status 0) or
    zeros."""
    coef, quant, status = det.jpeg_entropy(datas, height, width, sync=True, **kw)
    assert status.dtype == np.int32 and status.tolist() == list(want_status), status.tolist()
    coef, quant = coef.cpu().numpy(), _quant_np(det, quant)
    for f, data in enumerate(datas):
        if want_status[f] == 0:
            want, wq, _ = host_of(data)
            bh, bw = want.shape[:2]
            assert np.array_equal(coef[f, :bh, :bw], want) and np.array_equal(quant[f], wq), f
        else:
            assert not coef[f].any() and not quant[f].any(), f


def _groups():
    out = {}
    for c in nodri_cases():
        out.setdefault((c.height, c.width), []).append(c)
    return out


@pytest.mark.parametrize("subsequence", [8, 32, None])
def test_jpeg_sync_equals_the_host_decoder_on_every_file_without_restart_intervals(det, options, subsequence):
    groups = _groups()
    assert len(groups) >= 9 and sum(len(g) for g in groups.values()) >= 21 + 9 and len(groups[(64, 48)]) >= 5
    if subsequence:
        options("jpeg_sync_subsequence", subsequence)
    options("jpeg_sync_max_rounds", 4096)
    for (h, w), group in groups.items():
        datas, want = [c.data for c in group], [0] * len(group)
        if (h, w) == (64, 48):       # the other routes, in the same batch
            datas += [case("progressive_48x64").data, case("noise_16x16_444").data, rst_case("noise_48x64_grey").data,
                      rst_case("rows_48x64_420").data]
            want += [-1, -2, 0, 0]
        _check(det, datas, h, w, want)
    # without the option nothing has changed
    c = rst_case("nodri_48x64")
    coef, quant, status = det.jpeg_entropy([c.data], c.height, c.width)
    assert status.tolist() == [-3] and not coef.any().item() and det._options["jpeg_sync"] == 0


@pytest.mark.parametrize("prefix", ["noise_48x64_444_q95_r0", "nodri_48x64_420_q75_dri0"])
def test_jpeg_sync_cap_counts_the_rounds_the_host_counts(det, options, prefix):
    c = next(c for c in nodri_cases() if c.name.startswith(prefix))
    rounds, n = mrgingham_amd.jpeg_sync_rounds(c.data, 32)
    assert 16 < rounds < n
    options("jpeg_sync_subsequence", 32)
    options("jpeg_sync_max_rounds", rounds - 1)
    _check(det, [c.data, c.data], c.height, c.width, [-3, -3])
    options("jpeg_sync_max_rounds", rounds)
    _check(det, [c.data, c.data], c.height, c.width, [0, 0])


def test_jpeg_sync_defaults_take_every_realistic_file(det):
    assert det._options.get("jpeg_sync_subsequence", 128) == DEFAULT_SUBSEQUENCE and det._options.get("jpeg_sync_max_rounds", 0) == 0
    doc = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "jpeg_sync_bench.json")))
    rate = {int(S): leg["loader"]["threads_16"]["sync"]["frames_per_s_median"] for S, leg in doc["files"]["nodri420.jpg"]["subsequence"].items()}
    assert max(rate, key=rate.get) == DEFAULT_SUBSEQUENCE, rate                        # the default is the measured one
    small = [sync_case(name) for name in REALISTIC[:-1]]
    assert all((c.height, c.width) == (240, 320) for c in small)
    _check(det, [c.data for c in small], 240, 320, [0] * len(small))
    big = sync_case(REALISTIC[-1])
    _check(det, [big.data], big.height, big.width, [0])


@pytest.fixture(scope="module")
def mixed_files(tmp_path_factory):
    """48 x 64: no restart intervals in grey, 4:2:0 and 4:4:4, a file with them, the noise file that hardly synchronises, a
    progressive file, a 16 x 16 file, a missing path."""
    d = tmp_path_factory.mktemp("jpegs_sync")
    by_name = {c.name: c for c in nodri_cases()}
    picks = [by_name["white_48x64_grey_q100_r0"], by_name["nodri_48x64_420_q75_dri0"], by_name["noise_48x64_444_q95_r0"],
             rst_case("noise_48x64_grey"), sync_case("noise_48x64_grey_q100"), case("progressive_48x64"), case("noise_16x16_444"),
             by_name["white_48x64_420_q95_r0"]]
    paths = []
    for i, c in enumerate(picks):
        p = str(d / f"{i}_{c.name}.jpg")
        with open(p, "wb") as f:
            f.write(c.data)
        paths.append(p)
    paths.insert(6, str(d / "missing.jpg"))
    picks.insert(6, None)
    return paths, picks


@pytest.fixture(scope="module")
def host_frames(det, mixed_files):
    frames, status = det.read_jpegs(mixed_files[0], nthreads=2)
    return frames.cpu().numpy(), status


@pytest.mark.parametrize("cap", [0, 8])
@pytest.mark.parametrize("nthreads", [1, 4])
@pytest.mark.parametrize("chunk", [0, 1, 3])
def test_read_jpegs_sync_equals_host_entropy(det, options, mixed_files, host_frames, chunk, nthreads, cap):
    """At 32-byte subsequences.  cap 0: the default, within which every file of the list converges (the noise file too: 94
    rounds of 32 bytes are less than 8 KB).  cap 8: the three noise files are known not to have converged only when their chunk has passed the
    stream, and take the late way over the host threads."""
    paths, picks = mixed_files
    late = [mrgingham_amd.jpeg_sync_rounds(c.data, 32)[0] > 8 for c in (picks[1], picks[2], picks[4])]
    assert late == [True, True, True] and mrgingham_amd.jpeg_sync_rounds(picks[0].data, 32)[0] <= 8
    options("jpeg_chunk_frames", chunk)
    options("jpeg_sync_subsequence", 32)
    options("jpeg_sync_max_rounds", cap)
    frames, status = det.read_jpegs(paths, nthreads=nthreads, entropy="device", sync=True)
    assert det._options["jpeg_entropy"] == 0 and det._options["jpeg_sync"] == 0            # restored
    want = [0, 0, 0, 0, 0, -1, -1, -2, 0]
    assert status.dtype == np.int32 and status.tolist() == want == host_frames[1].tolist()
    got = frames.cpu().numpy()
    assert got.shape == (9, 64, 48) and np.array_equal(got, host_frames[0])
    for f, c in enumerate(picks):
        assert np.array_equal(got[f], c.luma) if want[f] == 0 else not got[f].any(), f


def test_read_jpegs_sync_late_fall_back_of_files_the_host_rejects(det, options, tmp_path):
    """At a cap of one round corrupted noise files do not converge, so the host threads decode them behind the chunk --
    and reject some: those are -1 and zero-filled, the others are the host path's frames."""
    c = sync_case("noise_48x64_grey_q100")
    made = sync_corruptions(c, per_kind=3)
    datas = [c.data] + [d for _, d in made]
    host = [mrgingham_amd.jpeg_coefficients(d) is not None for d in datas]
    assert host[0] and 2 <= sum(host) < len(host) and not any(host[7:10])                   # (the truncations are rejected)
    paths = []
    for i, d in enumerate(datas):
        paths.append(str(tmp_path / f"{i}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(d)
    want, want_status = det.read_jpegs(paths, nthreads=2)
    assert (want_status == 0).tolist() == host
    options("jpeg_sync_max_rounds", 1)
    for chunk in (0, 4):
        options("jpeg_chunk_frames", chunk)
        frames, status = det.read_jpegs(paths, nthreads=2, entropy="device", sync=True)
        assert status.tolist() == want_status.tolist() and np.array_equal(frames.cpu().numpy(), want.cpu().numpy())
        assert not frames[status != 0].any().item() and np.array_equal(frames[0].cpu().numpy(), c.luma)


def test_read_jpegs_sync_realistic_files(det, tmp_path):
    names = ["blend_320x240_grey_q90", "blend_320x240_420_q90", "blend_320x240_444_q95", "plain_320x240_420_q90"]
    paths = []
    for name in names:
        paths.append(str(tmp_path / f"{name}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(sync_case(name).data)
    frames, status = det.read_jpegs(paths, nthreads=2, entropy="device", sync=True)
    host, host_status = det.read_jpegs(paths, nthreads=2)
    assert status.tolist() == host_status.tolist() == [0, 0, 0, 0]
    assert np.array_equal(frames.cpu().numpy(), host.cpu().numpy())
    assert np.array_equal(frames[0].cpu().numpy(), sync_case(names[0]).luma)


@pytest.mark.parametrize("prefix", ["nodri_48x64_420_q75_dri0", "noise_48x64_grey_q100"])
def test_corrupted_files_cost_a_status_and_agree_with_the_host(det, options, prefix):
    """The corruptions test_jpeg_sync.py runs through the same decoder text on the host, in ONE device call per fixture:
    the device accepts exactly the files the host decoder accepts, with the same coefficients."""
    c = next(c for c in nodri_cases() if c.name.startswith(prefix))
    datas = [c.data] + [d for _, d in sync_corruptions(c)]
    assert len(datas) == 801
    host = [host_of(d) for d in datas]
    host = [r if r is not None and r[2] == (c.height, c.width) else None for r in host]      # (the size bytes are not touched)
    options("jpeg_sync_max_rounds", 4096)
    want = [0 if r is not None else -1 for r in host]
    assert want[0] == 0 and 0 < np.mean(want) + 1 < 1
    _check(det, datas, c.height, c.width, want)


def test_jpeg_sync_argument_errors(det, tmp_path):
    for name, bad in (("jpeg_sync", 2), ("jpeg_sync", -1), ("jpeg_sync_subsequence", 4), ("jpeg_sync_subsequence", 30),
                      ("jpeg_sync_subsequence", 1028), ("jpeg_sync_max_rounds", -1), ("jpeg_sync_max_rounds", 4097)):
        with pytest.raises(ValueError):
            det.set_option(name, bad)
    for name, good in (("jpeg_sync_subsequence", 1024), ("jpeg_sync_subsequence", 8), ("jpeg_sync_subsequence", 32),
                       ("jpeg_sync_max_rounds", 4096), ("jpeg_sync_max_rounds", 0), ("jpeg_sync", 1), ("jpeg_sync", 0)):
        det.set_option(name, good)
    p = str(tmp_path / "a.jpg")
    with open(p, "wb") as f:
        f.write(rst_case("nodri_48x64").data)
    with pytest.raises(ValueError):
        det.read_jpegs([p], entropy="host", sync=True)
    with pytest.raises(ValueError):
        det.read_jpegs([p], sync=True)
    frames, status = det.read_jpegs([p], entropy="device", sync=True)
    assert status.tolist() == [0] and np.array_equal(frames[0].cpu().numpy(), rst_case("nodri_48x64").luma)


def test_board_without_restart_markers_through_the_sync_decoder_and_the_chain(det, tmp_path):
    c = sync_case("blend_640x480_420_q90")
    f = str(tmp_path / "board_sync.jpg")
    with open(f, "wb") as fh:
        fh.write(c.data)
    frames, status = det.read_jpegs([f] * 4, entropy="device", sync=True)
    host, host_status = det.read_jpegs([f] * 4)
    assert status.tolist() == host_status.tolist() == [0, 0, 0, 0]
    assert np.array_equal(frames.cpu().numpy(), host.cpu().numpy())
    pts, lv, npts = det.chain(frames, 3, 4096)
    wpts, wlv, wnpts = det.chain(host, 3, 4096)
    n = npts.cpu().numpy()
    assert np.array_equal(n, wnpts.cpu().numpy()) and (n > 0).all() and (n == n[0]).all()
    for k in range(4):
        assert np.array_equal(pts[k, :n[k]].cpu().numpy(), wpts[k, :n[k]].cpu().numpy())
        assert np.array_equal(lv[k, :n[k]].cpu().numpy(), wlv[k, :n[k]].cpu().numpy())
