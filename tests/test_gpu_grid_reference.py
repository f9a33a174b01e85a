"""GPU: the boards of Detector.find_boards against upstream's own find_grid.cc on the DEVICE's candidates.

For every frame of a few small batches: the candidate set the device detects at a pyramid level goes through
oracle.ref_find_grid (the unmodified upstream file over the stand-in Voronoi diagram, tests/test_oracle_grid.py), and
find_boards(refine=False) -- boards as the grid finder made them -- must report exactly upstream's board, double for
double, at the first level from 3 down where upstream finds one, and no board where upstream finds none at any level.
Needs oracle/_ref/libgrid_ref.so (built where the reference tree is; it travels with the tree) and never reads the
reference tree itself."""
import numpy as np
import pytest

import mrgingham_amd
from mrgingham_amd import synth
from oracle import oracle

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not oracle.have_reference_grid(), reason="oracle/_ref/libgrid_ref.so is not built")]


def _batches():
    plain = synth.board_frame(640, 480, 10, 0).numpy()
    yield "640x480", 10, [plain, synth.board_frame(640, 480, 10, 5).numpy(), np.ascontiguousarray(plain[::-1, ::-1]),
                          synth.noise_frame(640, 480, 1, smooth=1).numpy()], [True, True, True, False]
    yield "480x640", 10, [np.ascontiguousarray(np.rot90(synth.board_frame(640, 480, 10, 2).numpy()))], [True]
    yield "800x600", 14, [synth.board_frame(800, 600, 14, 1).numpy()], [True]
    yield "1280x960", 10, [synth.cluttered_board_frame(1280, 960, 10, 2).numpy(),
                           synth.board_frame(1280, 960, 10, 0).numpy()], [True, True]


def test_find_boards_equals_upstream_grid_finder_on_device_candidates():
    import torch
    det = mrgingham_amd.Detector(0)
    try:
        for name, gridn, imgs, has_board in _batches():
            frames = torch.from_numpy(np.stack(imgs)).cuda()
            boards, found, levels = det.find_boards(frames, gridn=gridn, refine=False, levels=True)
            cand = {}
            for L in (3, 2, 1, 0):
                xy, counts = det.detect(frames, L, capacity=8192)
                xy, counts = xy.cpu().numpy(), counts.cpu().numpy()
                assert (counts <= 8192).all()
                cand[L] = [xy[f, :counts[f]] for f in range(len(imgs))]
            for f in range(len(imgs)):
                want, want_level = None, -1
                for L in (3, 2, 1, 0):                               # the level loop of mrgingham.cc:116-139
                    want = oracle.ref_find_grid(cand[L][f], gridn)
                    if want is not None:
                        want_level = L
                        break
                assert found[f] == want_level, (name, f, int(found[f]), want_level)
                assert (want is not None) == has_board[f], (name, f)
                if want is None:
                    assert np.isnan(boards[f]).all(), (name, f)
                    continue
                assert np.array_equal(boards[f], want), (name, f)
                assert (levels[f] == want_level).all(), (name, f)
                # the single-level call at that level, and the host entry point on the same candidates
                b1, f1 = det.find_boards(frames[f:f + 1], gridn=gridn, image_pyramid_level=want_level, refine=False)
                assert f1[0] == want_level and np.array_equal(b1[0], want), (name, f)
                assert np.array_equal(mrgingham_amd.find_grid_from_points(cand[want_level][f], gridn), want), (name, f)
    finally:
        det.close()
