"""What every launch path of the pixel stage hands to the component search -- level images, clamped responses, hot
lists, pixel -> index maps -- read straight after the pixel stream (Detector.pixel_products: the test hook
mrgingham_amd_debug_pixel_stage, no component search runs) and held to the contract of CompTables (csrc/common.h) by
tests/pixel_products.py, whose expectations are the CPU oracle's alone.  tests/test_pixel_products_checker.py shows that
the checker rejects every breach the end-to-end tests absorb.  Each case asserts through chain_info which launch ran.

Shapes: the smallest that cross the kernels' constants (256-pixel strips, 8-pixel groups, 8-row granules, the 32-row
ring, segments of >= 32 rows, 16 x 8 pyramid blocks, a level 3 of >= 15 pixels per side):
  512x256  fused level 0; levels 256x128, 128x64, 64x32 all take the merged launch; whole granules everywhere
  528x264  fused level 0 with a 16-pixel last strip; level 1 is 264x132: no merged launch, typed staging, ragged granule
  531x267  no fusion: the per-pixel pyramid kernel writes all three level images (half-to-even sizes) in one launch
  272x136  one full strip + 16 pixels; level 3 is 34x17, an interior of 3 rows
"""
import ctypes

import numpy as np
import pytest
import torch

import mrgingham_amd
from mrgingham_amd import synth
from oracle import oracle
from tests import cc_cases
from tests import pixel_products as pp

pytestmark = pytest.mark.gpu

KINDS = ("board", "noise", "checker")


def _checker(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return ((((x // 3) + (y // 3)) & 1) * 255).astype(np.uint8)


_FRAMES, _EXPECTED, _CHAINS = {}, {}, {}


def frame_of(kind, w, h):
    key = (kind, w, h)
    if key not in _FRAMES:
        if kind == "board":
            f = synth.board_frame(w, h, 10, 1).numpy()
        elif kind == "noise":
            f = np.random.default_rng(w * 131 + h).integers(0, 256, size=(h, w), dtype=np.uint8)
        else:
            f = _checker(w, h)
        f = np.ascontiguousarray(f)
        f.setflags(write=False)
        _FRAMES[key] = f
    return _FRAMES[key]


def expected(kind, w, h, level):
    """the oracle's (level image, clamped response): computed once per (frame, level), shared by every case"""
    key = (kind, w, h, level)
    if key not in _EXPECTED:
        _EXPECTED[key] = pp.expected_of(frame_of(kind, w, h), level)
    return _EXPECTED[key]


def oracle_chain(kind, w, h, start):
    key = (kind, w, h, start)
    if key not in _CHAINS:
        _CHAINS[key] = oracle.chain(frame_of(kind, w, h), start)
    return _CHAINS[key]


def _cuda(frames_np):
    return torch.from_numpy(np.ascontiguousarray(frames_np)).cuda()


def _batch(w, h, kinds=KINDS):
    return _cuda(np.stack([frame_of(k, w, h) for k in kinds]))


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector(0)
    d.set_option("hot_capacity_shift", 0)          # one table entry per pixel: the lists are compared exactly
    yield d
    d.close()


def check_all(products, w, h, levels, kinds=KINDS, lists=None):
    """every frame at every level of `levels`; `lists`: the levels whose response, list and map are products (all)"""
    counts = {}
    for L in levels:
        p = products[L]
        assert (p["w"], p["h"]) == oracle.level_dims(w, h, L)
        if lists is not None and L not in lists:
            assert "response" not in p and "hot_xy" not in p
            assert ("image" in p) == (L >= 1)
            for f, kind in enumerate(kinds if L >= 1 else ()):       # clause a. alone: the level image
                assert np.array_equal(p["image"][f], expected(kind, w, h, L)[0]), (L, kind)
            continue
        assert ("image" in p) == (L >= 1)
        for f, kind in enumerate(kinds):
            try:
                counts[L, kind] = pp.check_level(pp.frame_products(p, f), frame_of(kind, w, h), L, expected(kind, w, h, L))
            except pp.ProductError as e:
                raise AssertionError(f"{w}x{h} level {L}, {kind} frame: {e}") from e
    return counts


def hot_fractions(kind, w, h):
    hot, mask = pp.hot_groups(expected(kind, w, h, 0)[1])
    return float((mask != 0).mean()), int(hot.sum())


def test_frame_premises():
    """What the cases below rely on: the board frame is sparse, the 3-pixel checker dense (measured at 512x256: board
    4.0 % of the groups hot / 1 337 hot pixels, noise 22.6 % / 4 203, checker 61.9 % / 53 452)."""
    board, noise, checker = (hot_fractions(k, 512, 256) for k in KINDS)
    print("groups with a hot pixel, hot pixels:", board, noise, checker)
    assert board[0] < 0.10 and board[1] > 100
    assert checker[0] > 0.50
    assert board[0] < noise[0] < checker[0]
    assert checker[1] == 53452


# ------------------------------------------------------------------------------------------------- chain mode

SWEEPS = [("fuse_pyramid", 1), ("fuse_pyramid", 0), ("multi_level_launch", 0), ("multi_level_launch", 1), ("multi_level_launch", 2),
          ("chess_seg", 0), ("chess_seg", 32), ("chess_seg", 256), ("sparse_refine", 0), ("sparse_refine", 2)]
DEFAULTS = {"fuse_pyramid": 1, "multi_level_launch": 1, "chess_seg": 0, "sparse_refine": 1}


def expected_launch(w, h, option, value, aligned=True):
    """(fused, merged) of chain(start_level 3) as chain.hip documents the schedule: fusion wants frames of whole 16 x 8
    blocks on 16-byte boundaries and level 0 outside the merged launch; the merged launch wants every level in it 16
    pixels wide at least and a multiple of 16."""
    o = dict(DEFAULTS, **{option: value})
    if o["sparse_refine"] == 2:
        return 0, -1
    ml = o["multi_level_launch"]
    fused = int(bool(o["fuse_pyramid"]) and ml != 2 and w % 16 == 0 and h % 8 == 0 and aligned)
    lowest = 0 if ml == 2 else 1
    widths = [oracle.level_dims(w, h, L)[0] for L in range(lowest, 4)]
    merged = len(widths) if ml and all(x >= 16 and x % 16 == 0 for x in widths) else 0
    return fused, merged


@pytest.mark.parametrize("option,value", SWEEPS, ids=[f"{o}={v}" for o, v in SWEEPS])
@pytest.mark.parametrize("shape", [(512, 256), (528, 264)], ids=["512x256", "528x264"])
def test_chain_products_under_option_sweeps(det, shape, option, value):
    """One option away from the defaults at a time: fused or separate pyramid, one launch per level / levels 3..1 merged
    / all four merged, three segment heights, the dense schedule and the sparse one (whose `gentle` pyramid launch
    writes all three level images, and whose only pixel-stage response is the start level's)."""
    w, h = shape
    d = _batch(w, h)
    det.set_option(option, value)
    try:
        products = det.pixel_products(d, 3, "chain")
        info = det.chain_info()
    finally:
        det.set_option(option, DEFAULTS[option])
    assert info == expected_launch(w, h, option, value), (option, value, info)
    if shape == (512, 256):                                  # (the premises of the shape table, spelled out)
        assert info == {"fuse_pyramid": {0: (0, 3)}, "multi_level_launch": {0: (1, 0), 2: (0, 4)},
                        "sparse_refine": {2: (0, -1)}}.get(option, {}).get(value, (1, 3))
    else:
        assert info[1] <= 0                                  # level 1 is 264 wide: never merged
    check_all(products, w, h, range(4), lists=(3,) if info[1] == -1 else None)


def test_chain_products_on_a_ragged_shape(det):
    """531x267: no fusion, no merged launch; the per-pixel pyramid kernel writes 266x134, 133x67 and 66x33 in one launch;
    level 0 takes the typed staging (the width is no multiple of 16) with a ragged last group, granule and strip.  Again
    with 32-row segments."""
    w, h = 531, 267
    assert [oracle.level_dims(w, h, L) for L in (1, 2, 3)] == [(266, 134), (133, 67), (66, 33)]
    d = _batch(w, h)
    for seg in (0, 32):
        det.set_option("chess_seg", seg)
        try:
            products = det.pixel_products(d, 3, "chain")
        finally:
            det.set_option("chess_seg", 0)
        assert det.chain_info() == (0, 0)
        check_all(products, w, h, range(4))


def test_chain_products_on_one_strip_and_a_bit(det):
    """272x136: a full strip and a 16-pixel one, fused; level 1 is 136 wide (no merged launch); level 3 is 34x17."""
    w, h = 272, 136
    assert oracle.level_dims(w, h, 3) == (34, 17)
    products = det.pixel_products(_batch(w, h), 3, "chain")
    assert det.chain_info() == (1, 0)
    check_all(products, w, h, range(4))


def test_chain_products_with_a_decimated_level_4(det):
    """start_level 4 on 531x267: level 4 (33x17) comes from launch_decimate, levels 1..3 from the pyramid kernel."""
    w, h = 531, 267
    assert oracle.level_dims(w, h, 4) == (33, 17)
    products = det.pixel_products(_batch(w, h), 4, "chain")
    assert det.chain_info() == (0, 0)
    check_all(products, w, h, range(5))


@pytest.mark.parametrize("origin,fused", [(16, 1), (8, 0)], ids=["aligned", "off-by-8"])
def test_chain_products_on_strided_views(det, origin, fused):
    """Frames that are a window of a larger buffer.  Origin, row stride and frame pitch on 16-byte boundaries: fusion
    still applies.  An origin 8 bytes off: the fused kernel and the fast pyramid kernel must both refuse, and the
    per-pixel pyramid kernel and the response kernels take the window as it is."""
    w, h = 512, 256
    buf = torch.full((3, h + 8, w + 32), 77, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and buf.stride(1) % 16 == 0 and buf.stride(0) % 16 == 0
    view = buf[:, 4:4 + h, origin:origin + w]
    view.copy_(_batch(w, h))
    assert not view.is_contiguous() and view.data_ptr() % 16 == origin % 16
    products = det.pixel_products(view, 3, "chain")
    assert det.chain_info() == (fused, 3)
    check_all(products, w, h, range(4))
    assert bool((buf[:, :4] == 77).all()) and bool((buf[:, :, :origin] == 77).all())     # (the hook writes no frame)


# ------------------------------------------------------------------------------------------------- level mode

@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(528, 264), (531, 267)], ids=["528x264", "531x267"])
def test_level_products(det, shape, level):
    """What detect / refine queue for ONE level: launch_one_level_image (the pyramid kernel restricted to that level, fast
    or per-pixel) and that level's response launch on its own."""
    w, h = shape
    products = det.pixel_products(_batch(w, h), level, "level")
    assert sorted(products) == [level]
    check_all(products, w, h, (level,))


# ------------------------------------------------------------------------------------------------- response mode

def _check_response_mode(det, supplied):
    products = det.pixel_products(_cuda(supplied), mode="response")
    assert sorted(products) == [0] and "image" not in products[0]
    for f in range(len(supplied)):
        try:
            pp.check_products(pp.frame_products(products[0], f), None, pp.clamp_supplied_response(supplied[f]))
        except pp.ProductError as e:
            raise AssertionError(f"supplied response {f}: {e}") from e


def test_products_of_a_supplied_response(det):
    """launch_hot_from_response: hand-built responses around the thresholds with blobs on the margins and negative salt
    (203 wide: a ragged last group), and the oracle's own response of the checker frame (dense)."""
    rng = np.random.RandomState(11)
    _check_response_mode(det, np.stack([cc_cases.random_sparse_response(rng, 97, 203, 40, noise=n) for n in (0.0, 0.02, 0.3)]))
    _check_response_mode(det, np.stack([expected("checker", 512, 256, 0)[1], expected("board", 512, 256, 0)[1]]))


# ------------------------------------------------------------------------------------------------- collect_hot

def test_both_routes_of_the_hot_pixel_collection(det):
    """collect_hot (chess_hot.h) keeps a wave's first 192 group records in LDS and sends the rest straight to the list,
    one atomic per lane.  A workgroup works on a segment of rows of a 256-pixel strip, 32 groups per row, and each of its
    four waves owns a quarter of those rows.
      chess_seg 32:  a wave owns 8 rows = 256 groups.  On the board frame no WORKGROUP reaches 192 groups with a hot
                     pixel (asserted below from the oracle), so every record takes the LDS route.
      chess_seg 256: a wave owns 64 rows = 2048 groups.  On the checker frame 62 % of the groups have a hot pixel,
                     about 1300 per wave: whether a wave's quarter is two rows of every 8-row granule (what the
                     kernel does) or 64 rows on end, it passes 192 records in either strip (asserted below), and the
                     direct route runs in every workgroup.
    The test itself is black-box: frame x chess_seg, clauses d. to f. (and the rest) through check_level."""
    w, h = 512, 256
    board = pp.hot_groups(expected("board", w, h, 0)[1])[1] != 0
    checker = pp.hot_groups(expected("checker", w, h, 0)[1])[1] != 0
    per_workgroup = board.reshape(h // 32, 32, w // 256, 32).sum(axis=(1, 3))
    assert per_workgroup.max() < 192, per_workgroup.max()
    per_row = checker.reshape(h, w // 256, 32).sum(axis=2)                   # [row, strip]
    interleaved = per_row.reshape(h // 8, 4, 2, w // 256).sum(axis=(0, 2))   # [wave, strip]: rows 8 i + 2 wave + {0, 1}
    on_end = per_row.reshape(4, h // 4, w // 256).sum(axis=1)
    assert min(interleaved.min(), on_end.min()) > 2 * 192, (interleaved, on_end)
    for kind, seg in (("board", 32), ("checker", 256), ("checker", 32), ("board", 256)):
        det.set_option("chess_seg", seg)
        try:
            for fuse in (1, 0):                             # the fused level-0 kernel and the plain one
                det.set_option("fuse_pyramid", fuse)
                products = det.pixel_products(_batch(w, h, (kind,)), 3, "chain")
                assert det.chain_info() == (fuse, 3)
                check_all(products, w, h, range(4), kinds=(kind,))
        finally:
            det.set_option("chess_seg", 0)
            det.set_option("fuse_pyramid", 1)


# ------------------------------------------------------------------------------------------------- capacity, context

def _chain_equals_oracle(d, frames, kinds, w, h):
    """chain(frames, 3) on the frames the hook just ran on -- and, because a 64x32 level 3 yields no corner on any of
    them, on a board frame large enough to yield all 100 as well"""
    big = (1280, 960)
    for fr, ks, (fw, fh) in ((frames, kinds, (w, h)), (_batch(*big, ("board",)), ("board",), big)):
        pts, lv, npts = d.chain(fr, start_level=3, max_points=8192)
        for f, kind in enumerate(ks):
            wp, wl = oracle_chain(kind, fw, fh, 3)
            n = int(npts[f])
            assert n == len(wp), (kind, n, len(wp))
            assert np.array_equal(pts[f, :n].cpu().numpy(), wp) and np.array_equal(lv[f, :n].cpu().numpy(), wl), kind
    assert len(oracle_chain("board", *big, 3)[0]) >= 100 and (oracle_chain("board", *big, 3)[1] == 0).sum() >= 100


def test_overflowing_list_and_the_context_afterwards():
    """hot_capacity_shift 7 at 512x256 leaves 4096 entries per frame; the checker frame makes 53 452.  Clause g: what
    fits is held to a. - d. and f., hot_cnt is the oracle's count all the same, nothing spills into the board frame's
    tables behind it, which are exact.  Then back to shift 0: an ordinary chain on the same detector gives the
    oracle's corners -- the hook leaves the context whole."""
    w, h, kinds = 512, 256, ("checker", "board")
    d2 = mrgingham_amd.Detector(0)
    try:
        d2.set_option("hot_capacity_shift", 7)
        frames = _batch(w, h, kinds)
        products = d2.pixel_products(frames, 3, "chain")
        assert d2.chain_info() == (1, 3)
        p0 = products[0]
        assert p0["cap"] == 4096 and int(p0["hot_cnt"][0]) == 53452 and len(p0["hot_xy"][0]) == 4096
        assert int(p0["hot_cnt"][1]) == len(p0["hot_xy"][1]) < 4096
        counts = check_all(products, w, h, range(4), kinds=kinds)
        assert counts[0, "checker"] == 53452
        d2.set_option("hot_capacity_shift", 0)
        _chain_equals_oracle(d2, frames, kinds, w, h)
        check_all(d2.pixel_products(frames, 3, "chain"), w, h, range(4), kinds=kinds)      # and exact at shift 0
        _chain_equals_oracle(d2, frames, kinds, w, h)
    finally:
        d2.close()


def test_ordinary_calls_after_the_hook(det):
    """After every mode of the hook the same detector chains and detects like the oracle, and products that an ordinary
    call has overwritten are refused, not served stale."""
    w, h = 512, 256
    frames = _batch(w, h)
    det.pixel_products(frames, 3, "chain")
    _chain_equals_oracle(det, frames, KINDS, w, h)
    cap = ctypes.c_int32()
    assert det.L.mrgingham_amd_debug_pixel_products(det.ctx, 0, 0, None, None, None, ctypes.byref(cap), None, None) != 0
    det.pixel_products(frames, 2, "level")
    det.pixel_products(_cuda(np.stack([expected("board", w, h, 0)[1]])), mode="response")
    _chain_equals_oracle(det, frames, KINDS, w, h)
    xy, counts = det.detect(frames, 2, capacity=4096)
    for f, kind in enumerate(KINDS):
        want = oracle.find_corners(frame_of(kind, w, h), 2)
        assert int(counts[f]) == len(want) and np.array_equal(xy[f, :len(want)].cpu().numpy(), want), kind


# ------------------------------------------------------------------------------------------------- experiment builds

def test_experiment_kernels_hand_over_the_same_products(det):
    """Experiment builds (make EXPERIMENT=1, MRGINGHAM_AMD_LIB) carry 16-pixel-per-lane kernels for the fused level 0
    (chess_variant_hot 32) and for the merged / single small levels (16): the same contract.  The shipped library does
    not know the option."""
    try:
        det.set_option("chess_variant_hot", 48)
    except ValueError:
        pytest.skip("chess_variant_hot exists in experiment builds only")
    try:
        for (w, h) in ((512, 256), (528, 264)):
            products = det.pixel_products(_batch(w, h), 3, "chain")
            assert det.chain_info() == expected_launch(w, h, "chess_seg", 0)
            check_all(products, w, h, range(4))
    finally:
        det.set_option("chess_variant_hot", 0)
