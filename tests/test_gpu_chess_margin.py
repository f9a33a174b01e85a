"""The rows of the zeroed 7-pixel frame and the whole-granule instantiations of the ChESS row loop (chess.hip).

The CLAMP kernels zero a frame row by giving it a smaller bias inside the response arithmetic (the saturating
subtraction that strips the bias then yields 0), and frames of whole 16 x 8 blocks run an instantiation without the
per-row tests (WHOLE).  Shapes where that can go wrong, each with inputs that put the strongest responses ON the frame
rows; response, detect and chain against the C oracle, bit for bit:
  64 x 24    every output row is a frame row or has one in its window
  272 x 40   the second strip ends after 16 of its 256 pixels; first and last segment only
  256 x 528  cut into 64-row segments (option chess_seg): first, interior and last segments in one frame
  640 x 483  a height that is no multiple of 8: the instantiation with the row tests, default and 128-row segments
"""
import numpy as np
import pytest
import torch

import mrgingham_amd
from oracle import oracle

pytestmark = pytest.mark.gpu

MARGIN = 7
CASES = [(64, 24, 0), (272, 40, 0), (256, 528, 64), (640, 483, 0), (640, 483, 128)]


def _stamps(w, h, extreme):
    """A 0/255 frame whose response, were the frame rows not zeroed, would be at the extreme a 0/255 image can reach
    (+1360: the eight ring samples above and below the pixel white, the eight to its sides black, one of the three
    centre pixels white; -4080: the whole ring white, the three centre pixels black) at pixels of rows 5, 6, h-7 and
    h-6 -- frame rows whose rings lie wholly inside the image -- every 16 columns."""
    img = np.zeros((h, w), np.uint8) if extreme > 0 else np.full((h, w), 255, np.uint8)
    for i, cx in enumerate(range(8, w - 5, 16)):
        for cy in (5 + (i & 1), h - 7 + (i & 1)):
            if extreme > 0:
                for dy in range(-5, 6):
                    for dx in range(-5, 6):
                        if abs(dy) > abs(dx) or dx == dy:
                            img[cy + dy, cx + dx] = 255
            else:
                img[cy, cx - 1:cx + 2] = 0
    return img


def _stamp_pixels(w, h):
    return [(5 + (i & 1), cx) for i, cx in enumerate(range(8, w - 5, 16))] + \
           [(h - 7 + (i & 1), cx) for i, cx in enumerate(range(8, w - 5, 16))]


def _inputs(w, h):
    """All 0, all 255, the two 0/255 patterns with the response extremes on the frame rows, 0/255 noise and uniform
    noise (seeded)."""
    rng = np.random.RandomState(1000 * w + h)
    return np.stack([
        np.zeros((h, w), np.uint8),
        np.full((h, w), 255, np.uint8),
        _stamps(w, h, +1),
        _stamps(w, h, -1),
        (rng.randint(0, 2, size=(h, w)) * 255).astype(np.uint8),
        rng.randint(0, 256, size=(h, w)).astype(np.uint8),
    ])


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector(0)
    yield d
    d.close()


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}x{c[1]}-seg{c[2]}")
def case(request, det):
    w, h, seg = request.param
    frames = _inputs(w, h)
    det.set_option("chess_seg", seg)
    det.set_option("chess_variant", 1)   # the response without a hot list through chess_v1_kernel as well
    yield w, h, frames, torch.from_numpy(frames).cuda()
    det.set_option("chess_seg", 0)
    det.set_option("chess_variant", 0)


def test_patterns_are_extreme_on_the_frame_rows():
    """What the two patterns are for: the same pixels in a frame grown by 8 black / white pixels on every side, where
    the rows are no longer frame rows, have the largest and the smallest response a 0/255 image can have."""
    w, h = 64, 24
    frames = _inputs(w, h)
    hi = oracle.chess_response_5(np.pad(frames[2], 8, constant_values=0), fill=0)[8:-8, 8:-8]
    lo = oracle.chess_response_5(np.pad(frames[3], 8, constant_values=255), fill=0)[8:-8, 8:-8]
    for (y, x) in _stamp_pixels(w, h):
        assert (y < MARGIN or y >= h - MARGIN) and hi[y, x] == 1360 and lo[y, x] == -4080, (y, x, hi[y, x], lo[y, x])


def test_response_rows_of_the_frame_are_zero_and_the_rest_matches(det, case):
    w, h, frames, d = case
    cl = det.chess_response(d, 0, clamp=True).cpu().numpy()
    raw = det.chess_response(d, 0, clamp=False).cpu().numpy()
    for f in range(len(frames)):
        ref = oracle.chess_response_5(frames[f], fill=0)
        assert np.array_equal(cl[f], np.maximum(ref, 0)), (w, h, f)
        assert np.array_equal(raw[f], ref), (w, h, f)
        assert np.array_equal(cl[f], oracle.clamped_response(frames[f], 0)[0]), (w, h, f)
    for a in (cl, raw):
        assert not a[:, :MARGIN].any() and not a[:, h - MARGIN:].any()
        assert not a[:, :, :MARGIN].any() and not a[:, :, w - MARGIN:].any()


@pytest.mark.parametrize("level", [0, 1])
def test_detect_matches_oracle_and_reports_nothing_in_the_frame(det, case, level):
    w, h, frames, d = case
    xy, counts = det.detect(d, level, capacity=32768)
    xy, counts = xy.cpu().numpy(), counts.cpu().numpy()
    lw, lh = mrgingham_amd.level_dims(w, h, level)
    for f in range(len(frames)):
        want = oracle.find_corners(frames[f], level)
        assert counts[f] == len(want), (w, h, level, f)
        got = xy[f, :counts[f]]
        assert np.array_equal(got, want), (w, h, level, f)
        # a point is the centroid of hot pixels: none of them in the frame means no centroid there either
        if len(got):
            py = (got[:, 1] / 1000.0 + 0.5) / (1 << level) - 0.5   # back to the level's rows (pixel centres, rounded to 1/1000)
            assert py.min() >= MARGIN - 1e-3 and py.max() <= lh - MARGIN - 1 + 1e-3, (w, h, level, f, py.min(), py.max())


def test_chain_matches_oracle(det, case):
    w, h, frames, d = case
    P = 32768
    pts, lv, npts = det.chain(d, start_level=3, max_points=P)
    for f in range(len(frames)):
        wp, wl = oracle.chain(frames[f], 3)
        n = int(npts[f])
        assert n == len(wp) and n <= P, (w, h, f, n, len(wp))
        assert np.array_equal(pts[f, :n].cpu().numpy(), wp), (w, h, f)
        assert np.array_equal(lv[f, :n].cpu().numpy(), wl), (w, h, f)
