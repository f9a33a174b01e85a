"""The blob path over a batch of device-resident frames: Detector.blobs (mrgingham_amd_blobs_batch) and
Detector.find_boards(blobs=True) (mrgingham_amd_find_circle_grids_batch).  Expected values: oracle.find_blobs(img) per
frame, the sequential restatement (oracle/blobs_oracle.c), independent of the code under test.  Every comparison is
exact -- (x, y) * 1000 integers, values AND order -- and covers every frame of its batch."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import mrgingham_amd
from mrgingham_amd import _lib, synth
from oracle import oracle

from test_gpu_blobs import _random_scene, _shapes

pytestmark = pytest.mark.gpu

WORD_WIDTHS = [31, 32, 33, 63, 64, 65, 257]     # word boundaries of the bit planes


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector(0)
    yield d
    d.close()


def _dev(frames):
    return torch.from_numpy(np.ascontiguousarray(np.stack(frames))).cuda()


def _want(img):
    return oracle.find_blobs(img).astype(np.int64).reshape(-1, 2)


def _same(got, want, what):
    assert got.dtype == np.int32 and got.shape == (len(want), 2) and np.array_equal(got.astype(np.int64), want), what


def _scene(rng, h, w):
    """_random_scene, or for a frame of one row (which its noise generator cannot make) random runs of grey levels."""
    if h >= 2:
        return _random_scene(rng, h, w)
    row = np.empty((1, w), np.uint8)
    x = 0
    while x < w:
        n = rng.randrange(1, 40)
        row[0, x:x + n] = rng.choice([0, 30, 55, 95, 125, 160, 205, 255])
        x += n
    return row


def _mixed_frames():
    w, h = 640, 480
    return [synth.dots_frame(w, h, 10, 0).numpy(), synth.dots_frame(w, h, 7, 1).numpy(), synth.dots_frame(w, h, 5, 2).numpy(),
            _shapes(h, w), synth.noise_frame(w, h, 2, smooth=2).numpy(), np.zeros((h, w), np.uint8),
            np.full((h, w), 255, np.uint8), (np.indices((h, w)).sum(0) % 2 * 255).astype(np.uint8)]


@pytest.fixture(scope="module")
def mixed():
    frames = _mixed_frames()
    return frames, [_want(f) for f in frames]


def test_mixed_batch_no_cross_talk(det, mixed):
    frames, want = mixed
    got = det.blobs(_dev(frames))
    assert len(got) == len(frames)
    for f in range(len(frames)):
        _same(got[f], want[f], ("batch", f))
    assert sum(len(w) for w in want) > 100                       # (the circle grids ARE detected)
    got = det.blobs(_dev(frames[::-1]))
    for f in range(len(frames)):
        _same(got[len(frames) - 1 - f], want[f], ("reversed", f))
    for f in range(len(frames)):
        one = det.blobs(_dev(frames[f:f + 1]))
        assert len(one) == 1
        _same(one[0], want[f], ("alone", f))


def test_layout(det, mixed):
    frames, want = mixed
    B, (H, W) = len(frames), frames[0].shape
    big = torch.full((B, H + 9, W + 11), 77, dtype=torch.uint8, device="cuda")
    big[:, 3:3 + H, 5:5 + W] = _dev(frames)
    view = big[:, 3:3 + H, 5:5 + W]
    assert view.stride(1) > W and view.stride(0) > H * view.stride(1)
    got = det.blobs(view)
    for f in range(B):
        _same(got[f], want[f], ("slice", f))
    got = det.blobs(_dev(frames)[::2])
    assert len(got) == (B + 1) // 2
    for k, f in enumerate(range(0, B, 2)):
        _same(got[k], want[f], ("every second", f))
    assert det.blobs(torch.zeros((0, H, W), dtype=torch.uint8, device="cuda")) == []
    rng = random.Random(11)
    for w in WORD_WIDTHS:
        for h in (1, 2, 8, 97):
            scenes = [_scene(rng, h, w) for _ in range(4)]
            got = det.blobs(_dev(scenes))
            for f in range(4):
                _same(got[f], _want(scenes[f]), ("size", w, h, f))


def test_chunk_seams(det, mixed):
    frames, want = mixed
    frames, want = frames[:5], want[:5]
    try:
        for chunk in (1, 2, 3, 5, 0):
            det.set_option("blob_chunk_frames", chunk)
            det.blobs_stats()
            got = det.blobs(_dev(frames))
            for f in range(5):
                _same(got[f], want[f], ("chunk", chunk, f))
            assert det.blobs_stats()["chunks"] == (-(-5 // chunk) if chunk else 1)
    finally:
        det.set_option("blob_chunk_frames", 0)
    with pytest.raises(ValueError):
        det.set_option("blob_chunk_frames", -1)


def test_capacity_and_arguments(det):
    L = _lib.lib()
    frames = [synth.dots_frame(640, 480, g, s).numpy() for g, s in ((10, 0), (7, 1), (5, 2))]
    full = det.blobs(_dev(frames))
    want = [_want(f) for f in frames]
    for f in range(3):
        _same(full[f], want[f], f)
    dev = _dev(frames)
    fr, B, H, W = det._frames(dev)
    nmin = min(len(w) for w in want)
    assert nmin >= 25
    GUARD = -123456789
    for cap in (0, 1, nmin - 1):
        xy = np.full((B, cap + 3, 2), GUARD, np.int32)      # a dense [B, cap, 2] block in front, then a guard
        flat = xy.reshape(-1)
        counts = np.full(B + 2, GUARD, np.int32)
        rc = L.mrgingham_amd_blobs_batch(det.ctx, ctypes.byref(fr), flat.ctypes.data if cap else None, cap,
                                         counts.ctypes.data, 0)
        assert rc == 0
        assert counts[:B].tolist() == [len(w) for w in want] and (counts[B:] == GUARD).all()
        stored = flat[:B * cap * 2].reshape(B, cap, 2)
        for f in range(B):
            assert np.array_equal(stored[f].astype(np.int64), want[f][:cap]), (cap, f)
        assert (flat[B * cap * 2:] == GUARD).all()
    # bad arguments: MRGINGHAM_AMD_ERR_ARG and nothing written
    xy = np.full((B, 8, 2), GUARD, np.int32)
    counts = np.full(B, GUARD, np.int32)
    boards = np.full((B, 100, 2), -7.0)
    found = np.full(B, 55, np.int8)

    def blobs_rc(f, counts_ptr=counts.ctypes.data):
        return L.mrgingham_amd_blobs_batch(det.ctx, ctypes.byref(f), xy.ctypes.data, 8, counts_ptr, 0)

    def grids_rc(f, gridn=10):
        return L.mrgingham_amd_find_circle_grids_batch(det.ctx, ctypes.byref(f), gridn, boards.ctypes.data, found.ctypes.data, 0)
    narrow = _lib.Frames(fr.frames, fr.frame_pitch, B, W, H, W - 1)
    wide = _lib.Frames(fr.frames, fr.frame_pitch, B, 40000, H, 40000)
    negative = _lib.Frames(fr.frames, fr.frame_pitch, -1, W, H, W)
    assert blobs_rc(fr, None) == -1
    assert L.mrgingham_amd_blobs_batch(det.ctx, ctypes.byref(fr), None, 8, counts.ctypes.data, 0) == -1
    assert L.mrgingham_amd_blobs_batch(det.ctx, ctypes.byref(fr), xy.ctypes.data, -1, counts.ctypes.data, 0) == -1
    for bad in (narrow, wide, negative):
        assert blobs_rc(bad) == -1
        assert grids_rc(bad) == -1
    assert grids_rc(fr, gridn=1) == -1
    assert L.mrgingham_amd_find_circle_grids_batch(det.ctx, ctypes.byref(fr), 10, None, found.ctypes.data, 0) == -1
    assert L.mrgingham_amd_find_circle_grids_batch(det.ctx, ctypes.byref(fr), 10, boards.ctypes.data, None, 0) == -1
    assert (xy == GUARD).all() and (counts == GUARD).all() and (boards == -7.0).all() and (found == 55).all()
    # empty batches and empty frames succeed with zero counts
    empty = _lib.Frames(fr.frames, fr.frame_pitch, 0, W, H, W)
    assert blobs_rc(empty) == 0 and (counts == GUARD).all()
    flat0 = _lib.Frames(fr.frames, 0, B, 0, H, 0)
    assert blobs_rc(flat0) == 0 and (counts == 0).all() and (xy == GUARD).all()


def test_random_scenes_against_the_oracle(det):
    """Short by default; MRG_FUZZ_ITERS=300 for the long form."""
    rng = random.Random(int(os.environ.get("MRG_FUZZ_SEED", "5")))
    mismatches = 0
    iters = int(os.environ.get("MRG_FUZZ_ITERS", "12"))
    for it in range(iters):
        w, h = rng.randrange(8, 700), rng.randrange(8, 500)
        if rng.random() < 0.3:
            w = rng.choice(WORD_WIDTHS)
        scenes = [_random_scene(rng, h, w) for _ in range(8)]
        got = det.blobs(_dev(scenes))
        for f in range(8):
            want = _want(scenes[f])
            ok = got[f].shape == (len(want), 2) and np.array_equal(got[f].astype(np.int64), want)
            if not ok:
                mismatches += 1
                print("mismatch", it, f, w, h)
    print(f"blobs batch fuzz: {iters} iterations of 8 frames, {mismatches} mismatches")
    assert mismatches == 0


def test_large_frames(det):
    """~10^6 nodes per frame: node numbers of the later frames far beyond those of a single frame, arcs down a full
    frame edge in frames other than the first."""
    frames = [synth.dots_frame(4096, 3072, 10, 1).numpy(), synth.dots_frame(4096, 3072, 10, 2).numpy(),
              synth.board_frame(4096, 3072, 10, 4).numpy(), _random_scene(random.Random(77), 3072, 4096)]
    det.blobs_stats()
    got = det.blobs(_dev(frames))
    st = det.blobs_stats()
    assert st["chunks"] == 1 and st["nodes"] > 1e6
    for f in range(4):
        _same(got[f], _want(frames[f]), f)


def test_circle_grids(det):
    w, h, gridn = 800, 600, 10
    frames = [synth.dots_frame(w, h, gridn, s).numpy() for s in range(4)]
    frames += [synth.dots_frame(w, h, 7, 0).numpy(), np.full((h, w), 255, np.uint8), synth.noise_frame(w, h, 4, smooth=2).numpy()]
    dev = _dev(frames)
    boards, found = det.find_boards(dev, gridn=gridn, image_pyramid_level=0, blobs=True)
    assert boards.shape == (7, gridn * gridn, 2) and found.shape == (7,)
    for f, img in enumerate(frames):
        pts = oracle.find_blobs(img)
        want = mrgingham_amd.find_grid_from_points(pts, gridn)
        if want is None:
            assert found[f] == -1 and np.isnan(boards[f]).all(), f
        else:
            assert found[f] == 0 and np.array_equal(boards[f], want), f
        if f < 4:
            assert want is not None
            lat = synth.board_lattice(w, h, gridn, f).reshape(-1, 2)
            assert np.abs(boards[f] - lat).max() < 0.25
        if f in (4, 5):
            assert len(pts) < gridn * gridn and found[f] == -1
    for level in (-1, 1):
        with pytest.raises(RuntimeError, match="blob detector requires that image_pyramid_level == 0"):
            det.find_boards(dev, gridn=gridn, image_pyramid_level=level, blobs=True)
    chess = _dev([synth.board_frame(w, h, gridn, s).numpy() for s in range(3)])
    b0, f0 = det.find_boards(chess)
    b1, f1 = det.find_boards(chess, blobs=False)
    assert (f0 >= 0).all() and np.array_equal(f0, f1) and np.array_equal(b0, b1)


def test_interleaving_with_find_boards_jobs(det, mixed):
    frames, want = mixed
    chess = _dev([synth.board_frame(640, 480, 10, s).numpy() for s in range(3)])
    dots = _dev(frames[:4])
    b_alone, f_alone = det.find_boards(chess)
    job = det.find_boards_submit(chess)
    got = det.blobs(dots)
    boards, found = det.find_boards_collect(job)
    assert (f_alone >= 0).all() and np.array_equal(found, f_alone) and np.array_equal(boards, b_alone)
    for f in range(4):
        _same(got[f], want[f], f)
