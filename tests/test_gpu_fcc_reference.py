"""The HIP kernels after the ChESS response -- cc.hip, cc_lds.hip, cc_sparse.h, the tails of chain.hip -- against the
upstream find_chessboard_corners.cc ITSELF, not against the C restatement that was written alongside them.

The expected values come from oracle/_ref/libfcc_ref.so and libfcc_resp_ref.so (the upstream file compiled
unmodified by `make -C oracle ref`; the libraries travel with the tree, the sources do not).  Where they are absent,
the cases that tests/golden/fcc_kat.npz holds upstream's recorded answers for still run, against those; the rest skip.
Nothing here reads the upstream sources.

On images every comparison hands the reference the level image that the DEVICE produced (Detector.decimate): what is
compared is the component search and the coordinate scaling at every level, not the resize arithmetic.  Everything is
compared for equality: integers, order, levels, counts, and the refined doubles."""
import numpy as np
import pytest
import torch

import mrgingham_amd
from mrgingham_amd import synth
from oracle import oracle

import cc_cases
import fcc_cases

pytestmark = pytest.mark.gpu

LIVE = oracle.have_reference_fcc()
needs_live = pytest.mark.skipif(not LIVE, reason="oracle/_ref/libfcc_*.so not built and the case is not in fcc_kat.npz")


@pytest.fixture(scope="module")
def kat():
    entries = fcc_cases.load_kat()
    return {(m["kind"], m["name"], m.get("level", m.get("start"))): (m, f) for m, f in entries}


@pytest.fixture(scope="module", params=["lds", "global"])
def det(request):
    """Both implementations of the search, as in test_gpu_cc_rules.py."""
    d = mrgingham_amd.Detector(0)
    d.set_option("cc_lds", 1 if request.param == "lds" else 0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def plain():
    d = mrgingham_amd.Detector(0)
    yield d
    d.close()


def _same_refine(got, want):
    return got[2] == want[2] and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


# ----------------------------------------------------------------------------- on responses

def _want_detect(kat, name, d, img, level):
    if LIVE:
        return oracle.ref_cc_detect_on_response(d, img, level)
    m, f = kat[("detect_on_response", name, level)]
    assert np.array_equal(f["d"], d) and np.array_equal(f["img"], img), name      # the answer is for this input
    return f["out"]


def _want_refine(kat, name, pts, lv, d, img, level):
    if LIVE:
        return oracle.ref_cc_refine_on_response(pts, lv, d, img, level)
    m, f = kat[("refine_on_response", name, level)]
    assert np.array_equal(f["d"], d) and np.array_equal(f["pts"], pts) and np.array_equal(f["lv"], lv), name
    return f["out_pts"], f["out_lv"], m["n"]


def _detect(det, ds, imgs, level=0, capacity=4096):
    xy, cnt = det.cc_detect_on_response(torch.from_numpy(np.stack(ds)).cuda(), torch.from_numpy(np.stack(imgs)).cuda(),
                                        level=level, capacity=capacity)
    xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
    return [xy[f, :cnt[f]] for f in range(len(ds))]


def _refine(det, ptss, lvs, ds, imgs, level):
    """A batch: frame f has its own points (padded to the longest list)."""
    B, P = len(ds), max(1, max(len(lv) for lv in lvs))
    tp = torch.zeros((B, P, 2), dtype=torch.float64)
    tl = torch.zeros((B, P), dtype=torch.int8)
    for f in range(B):
        tp[f, :len(lvs[f])] = torch.from_numpy(np.asarray(ptss[f], np.float64).reshape(-1, 2))
        tl[f, :len(lvs[f])] = torch.from_numpy(np.asarray(lvs[f], np.int8))
    tp, tl = tp.cuda(), tl.cuda()
    n = torch.tensor([len(lv) for lv in lvs], dtype=torch.int32).cuda()
    nref = det.cc_refine_on_response(torch.from_numpy(np.stack(ds)).cuda(), torch.from_numpy(np.stack(imgs)).cuda(), level,
                                     tp, tl, n)
    tp, tl, nref = tp.cpu().numpy(), tl.cpu().numpy(), nref.cpu().numpy()
    return [(tp[f, :len(lvs[f])], tl[f, :len(lvs[f])], int(nref[f])) for f in range(B)]


def test_handbuilt_detect_cases_one_frame_at_a_time(det, kat):
    cases = fcc_cases.response_detect_cases()
    assert len(cases) >= 50
    for name, d, img, level, expected in cases:
        got = _detect(det, [d], [img], level=level)[0]
        assert np.array_equal(got, _want_detect(kat, name, d, img, level)), name
        if expected is not None:
            assert got.tolist() == expected, name


def test_handbuilt_detect_cases_as_batches(det, kat):
    """One batch per (shape, level): every 48x64 case at level 0 in one call, the large frames in another."""
    groups = {}
    for c in fcc_cases.response_detect_cases():
        groups.setdefault((c[1].shape, c[3]), []).append(c)
    assert max(len(g) for g in groups.values()) >= 40
    for (shape, level), cases in groups.items():
        got = _detect(det, [c[1] for c in cases], [c[2] for c in cases], level=level)
        for (name, d, img, _, _), g in zip(cases, got):
            assert np.array_equal(g, _want_detect(kat, name, d, img, level)), name


def test_large_frame_leaves_the_lds_search(kat):
    """More than 2048 hot pixels in one component: the search out of LDS hands the frame over, and says so."""
    d = mrgingham_amd.Detector(0)
    try:
        d.set_option("cc_lds", 1)
        name, resp, img, expected = cc_cases.large_detect_cases()[0]
        got = _detect(d, [resp], [img])[0]
        assert d.debug_paths(0, 1).tolist() == [0]
        assert np.array_equal(got, _want_detect(kat, name, resp, img, 0)) and len(got) == 1
    finally:
        d.close()


def test_handbuilt_refine_cases_one_frame_at_a_time(det, kat):
    for name, pts, lv, d, img, level, expected in fcc_cases.response_refine_cases():
        got = _refine(det, [pts], [lv], [d], [img], level)[0]
        assert _same_refine(got, _want_refine(kat, name, pts, lv, d, img, level)), name
        if expected is not None:
            ep, el, en = expected
            assert got[2] == en and got[1].tolist() == el and np.array_equal(got[0], ep), name


def test_handbuilt_refine_cases_as_batches(det, kat):
    groups = {}
    for c in fcc_cases.response_refine_cases():
        groups.setdefault(c[5], []).append(c)
    assert len(groups[0]) >= 7
    for level, cases in groups.items():
        got = _refine(det, [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases], level)
        for (name, pts, lv, d, img, _, _), g in zip(cases, got):
            assert _same_refine(g, _want_refine(kat, name, pts, lv, d, img, level)), name


@needs_live
@pytest.mark.parametrize("shape,nblobs,noise", [((48, 64), 12, 0.0), ((97, 129), 80, 0.01), ((64, 1001), 200, 0.003)])
def test_random_sparse_responses(det, shape, nblobs, noise):
    """Detection on the generator's frames as they are; refinement on the same with the 7-pixel frame cleared, as the
    upstream pipeline leaves it and as the device entry point makes it (fcc_cases.zero_ring)."""
    ds, imgs = fcc_cases.random_sparse_batch(shape, nblobs, noise, B=4)
    got = _detect(det, ds, imgs, capacity=8192)
    total = 0
    for f in range(len(ds)):
        want = oracle.ref_cc_detect_on_response(ds[f], imgs[f])
        assert np.array_equal(got[f], want), (shape, f, len(got[f]), len(want))
        total += len(want)
    assert total > 0
    for level in (0, 2):
        zs = [fcc_cases.zero_ring(d) for d in ds]
        pl = [fcc_cases.random_refine_points(np.random.RandomState(10 * level + f), zs[f], level) for f in range(len(zs))]
        got = _refine(det, [p for p, _ in pl], [l for _, l in pl], zs, imgs, level)
        nref = 0
        for f in range(len(zs)):
            want = oracle.ref_cc_refine_on_response(pl[f][0], pl[f][1], zs[f], imgs[f], level)
            assert _same_refine(got[f], want), (shape, level, f)
            nref += want[2]
        assert nref > 0


# ----------------------------------------------------------------------------- on images

def _device_levels(det, image):
    t = torch.from_numpy(np.ascontiguousarray(image)).cuda().unsqueeze(0)
    return {L: det.decimate(t, L)[0].cpu().numpy() for L in (1, 2, 3)}


def _images(kat):
    small = {k[1]: f["image"] for k, (m, f) in kat.items() if k[0] == "image"}          # stored inputs, 131x96 and smaller
    if not LIVE:
        return small
    return dict(small, **{"board6_333x240": synth.board_frame(333, 240, 6, 3).numpy(),
                          "smoothed_noise_333x240": synth.noise_frame(333, 240, 4, smooth=2).numpy(),
                          "board10_640x480": synth.board_frame(640, 480, 10, 0).numpy(),
                          "cluttered_640x480": synth.cluttered_board_frame(640, 480, 10, 2).numpy()})


def test_find_points_and_refine_points_equal_upstream_on_the_device_level_images(plain, kat):
    images = _images(kat)
    assert {im.shape for im in images.values()} >= ({(96, 131), (240, 333), (480, 640)} if LIVE else {(96, 131)})
    ncand = 0
    for name, image in images.items():
        levels = _device_levels(plain, image)
        want = {}
        for L in range(4):
            if LIVE:
                want[L] = oracle.ref_find_corners(image, L, levels.get(L))
            else:
                assert L == 0 or np.array_equal(levels[L], kat[("level_image", name, L)][1]["image"]), (name, L)
                want[L] = kat[("detect", name, L)][1]["out"]
            got = mrgingham_amd.find_points(image, image_pyramid_level=L)
            assert np.array_equal(np.round(got * 1000).astype(np.int64), want[L].astype(np.int64)), (name, "detect", L)
            ncand += len(want[L])
        for L in range(3):
            pts = want[L + 1].astype(np.float64) / 1000.0
            lv = np.full(len(pts), L + 1, np.int8)
            if LIVE:
                if len(lv) > 2:
                    lv[1] = L
                w = oracle.ref_refine_corners(pts, lv, image, L, levels.get(L))
            else:
                m, f = kat[("refine", name, L)]
                assert np.array_equal(f["pts"], pts)
                w = (f["out_pts"], f["out_lv"], m["n"])
            assert _same_refine(mrgingham_amd.refine_points(pts, lv, image, L), w), (name, "refine", L)
    assert ncand > 100


# ----------------------------------------------------------------------------- the chain

def _check_chain(det, frames, start, kat=None, names=None, max_points=1024):
    pts, lv, npts = det.chain(torch.from_numpy(frames).cuda(), start_level=start, max_points=max_points)
    pts, lv, npts = pts.cpu().numpy(), lv.cpu().numpy(), npts.cpu().numpy()
    total = 0
    for f in range(len(frames)):
        levels = _device_levels(det, frames[f])
        if LIVE:
            wp, wl = oracle.ref_chain(frames[f], start, levels)
        else:
            assert all(np.array_equal(levels[L], kat[("level_image", names[f], L)][1]["image"]) for L in (1, 2, 3))
            e = kat[("chain", names[f], start)][1]
            wp, wl = e["out_pts"], e["out_lv"]
        n = int(npts[f])
        assert n == len(wl), (f, start, n, len(wl))
        assert np.array_equal(lv[f, :n], wl) and np.array_equal(pts[f, :n], wp), (f, start)
        total += n
    return total


def _chain_frames():
    board = synth.board_frame(640, 480, 10, 0).numpy()
    cluttered = synth.cluttered_board_frame(640, 480, 10, 2).numpy()
    return board, cluttered


@needs_live
@pytest.mark.parametrize("start", [3, 2, 1])
def test_dense_chain_equals_upstream(start):
    board, cluttered = _chain_frames()
    det = mrgingham_amd.Detector(0)
    try:
        det.set_option("sparse_refine", 0)
        assert _check_chain(det, board[None], start) >= 60
        assert _check_chain(det, cluttered[None], start) > 0
        mixed = np.stack([board, cluttered, synth.board_frame(640, 480, 10, 5).numpy(), cluttered])
        _check_chain(det, mixed, start)
        assert det.chain_info()[1] >= 0                        # the dense schedule ran
    finally:
        det.close()


@needs_live
def test_sparse_chain_equals_upstream_and_the_sparse_kernels_ran():
    """640x480, 8 frames, start level 3, sparse_refine = 2: the smallest setting at which test_gpu_sparse.py shows the
    sparse kernels taking every frame.  The stats must say that they did -- a frame handed back to the dense kernels, or
    a call left to the dense schedule, fails this test even though its answer is the same."""
    det = mrgingham_amd.Detector(0)
    try:
        det.set_option("sparse_refine", 2)
        frames = synth.board_batch(8, 640, 480, gridn=10, seed0=300).numpy()
        det.sparse_fallbacks()
        assert _check_chain(det, frames, 3) >= 8 * 50
        assert det.sparse_fallbacks() == 0
        det.chain(torch.from_numpy(frames).cuda(), start_level=3, max_points=1024)
        assert det.chain_info()[1] == -1                       # the sparse schedule
        assert det.sparse_fallbacks() == 0
    finally:
        det.close()


def test_chain_on_the_stored_images_equals_upstreams_recorded_or_live_answers(kat):
    """The chains of fcc_kat.npz: these run with or without the reference build."""
    names = sorted(k[1] for k in kat if k[0] == "image")
    det = mrgingham_amd.Detector(0)
    try:
        det.set_option("sparse_refine", 0)
        total = 0
        for name in names:
            image = kat[("image", name, None)][1]["image"]
            for start in (3, 2, 1):
                total += _check_chain(det, image[None], start, kat, [name])
        assert total >= 30
    finally:
        det.close()
