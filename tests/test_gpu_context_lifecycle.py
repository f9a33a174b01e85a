"""The life of one context: what it holds of the device (Detector.scratch_bytes) from create to destroy, and a second
context in the same process behind it.  Every buffer, event and stream of a context is a member that frees itself, and
scratch_bytes is a running total that ensure() keeps: the total starts at zero, rises with the first call of every
family that owns context scratch, never falls, and stays where it is when the identical call is made again (no regrowth,
no double count).  Nothing here measures the device's free memory: the machines are shared and that number is not ours.

Two families need a word.  Detector.jpeg_idct works on the caller's tensors and owns no context scratch: its family is
the call itself plus read_jpegs, the entry point of the same file that does (the loader's chunk slots).  find_boards and
find_boards_submit / _collect size the level scratch and the job buffers of ONE scratch set per call, the set the job
takes: for them "a call" is as many consecutive calls as a context can rotate sets (three), so that every set has had
its turn before the repeat."""
import os

import numpy as np
import pytest

import mrgingham_amd
from mrgingham_amd import synth
from test_jpeg_io import case
from tests import png_cases

pytestmark = pytest.mark.gpu

SETS = 3          # scratch sets a context can rotate through (kMaxSets)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _chain(det, frames):
    """-> per frame (count, points, levels), the points and levels cut to the count"""
    pts, lv, npts = [t.cpu().numpy() for t in det.chain(frames, start_level=3, max_points=256)]
    return [(int(n), pts[f, :n].copy(), lv[f, :n].copy()) for f, n in enumerate(npts)]


def _same_chain(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a, b))


def test_scratch_total_over_the_life_of_a_context(tmp_path):
    import torch
    boards = _cuda(np.stack([synth.board_frame(640, 480, 10, s).numpy() for s in (0, 5)]))        # (the frames of smoke())
    larger = _cuda(np.stack([synth.board_frame(800, 600, 14, s).numpy() for s in (1, 2)]))
    deep = np.stack([boards[0].cpu().numpy().astype(np.uint16) * 16 + 300, boards[1].cpu().numpy().astype(np.uint16) * 257])
    deep = torch.from_numpy(deep.view(np.int16)).cuda().view(torch.uint16)
    dots = _cuda(np.stack([synth.dots_frame(320, 240, 5, s).numpy() for s in (1, 2)]))
    jpegs = [case("noise_48x64_grey"), case("noise_48x64_420")]
    parts = [mrgingham_amd.jpeg_coefficients(c.data) for c in jpegs]
    coef, quant = _cuda(np.stack([p[0] for p in parts])), _cuda(np.stack([p[1] for p in parts]).view(np.int16))
    jpeg_paths = []
    for c in jpegs:
        jpeg_paths.append(os.path.join(str(tmp_path), c.name + ".jpg"))
        with open(jpeg_paths[-1], "wb") as f:
            f.write(c.data)
    scan = _cuda(np.stack([png_cases.scanlines(png_cases.random_image(48, 64, 0, 8, seed=s), 0, 8) for s in (70, 71)]))

    det = mrgingham_amd.Detector()
    try:
        assert det.scratch_bytes() == 0
        det.set_kernel_timing(2)                      # the engine-clock probe alone: its two counters are context scratch
        clk = det.scratch_bytes()
        print(f"scratch_bytes: the clock probe {clk}")
        assert clk > 0
        det.set_kernel_timing(2)
        assert det.scratch_bytes() == clk

        def detect_refine():
            xy, counts = det.detect(larger, 2, capacity=256)
            pts, lv = (xy.to(torch.float64) / 1000.0).contiguous(), torch.full((2, 256), 2, dtype=torch.int8, device="cuda")
            det.refine(larger, 1, pts, lv, counts.clamp(max=256))
            det.refine(larger, 0, pts, lv, counts.clamp(max=256))

        def jpeg():
            det.jpeg_idct(coef, quant, 64, 48)
            frames, status = det.read_jpegs(jpeg_paths, nthreads=2)
            assert status.tolist() == [0, 0]

        def submit_collect():
            for _ in range(SETS):
                det.find_boards_collect(det.find_boards_submit(larger, gridn=14))

        first = []
        families = [("chain", lambda: first.append(_chain(det, boards))),
                    ("detect + refine", detect_refine),
                    ("preprocess uint8", lambda: det.preprocess(boards, clahe=True, blur_radius=1)),
                    ("preprocess uint16", lambda: det.preprocess(deep, clahe=True, blur_radius=1)),
                    ("blobs", lambda: det.blobs(dots, nthreads=2)),
                    ("jpeg_idct", jpeg),
                    ("png_reconstruct", lambda: det.png_reconstruct(scan, 64, 48, 8, 0)),
                    ("find_boards", lambda: [det.find_boards(boards, gridn=10, nthreads=2) for _ in range(SETS)]),
                    ("find_boards_submit + _collect", submit_collect)]
        total = clk
        for name, call in families:
            call()
            torch.cuda.synchronize()
            after = det.scratch_bytes()
            call()
            torch.cuda.synchronize()
            again = det.scratch_bytes()
            print(f"scratch_bytes: {name}: {total} -> {after}, the same call again {again}")
            assert after > total, name                # (which covers "has not fallen")
            assert again == after, name
            total = after

        # kernel timing on: the pairs around the level-0 launches are read once and recycled, not lost
        det.set_kernel_timing(1)
        timed = _chain(det, boards)
        ms, launches = det.chess_kernel_ms()
        assert launches > 0 and ms > 0
        assert det.chess_kernel_ms()[1] == 0
        assert _same_chain(first[0], timed)
        print(f"chain: {[n for n, _, _ in timed]} points, {launches} timed launches")
        assert min(n for n, _, _ in timed) > 0        # (the comparisons compare something)
    finally:
        det.close()

    second = mrgingham_amd.Detector()
    try:
        assert second.scratch_bytes() == 0
        assert _same_chain(first[0], _chain(second, boards))
    finally:
        second.close()
