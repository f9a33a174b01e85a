"""The C restatement of the component search (oracle/mrgingham_oracle.c) against the upstream
find_chessboard_corners.cc ITSELF (no GPU).

`make -C oracle ref` compiles the upstream file, unmodified and where it lies, into oracle/_ref/ (never committed):
libfcc_ref.so runs it on images with the upstream ChESS.c, libfcc_resp_ref.so runs its component search on responses
that the caller builds.  Above level 0 upstream's one OpenCV call is cv::resize, which in this build hands back the
level image the caller passes in, so what is pinned is the component search and the coordinate scaling at every
level, and the whole path at level 0 -- not the resize arithmetic.

Every comparison is equality: integers, order, levels, counts; refined doubles bit for bit.  The comparisons with the
live build skip where oracle/_ref is absent; the replay of tests/golden/fcc_kat.npz (upstream's recorded answers on
stored inputs) never does."""
import os

import numpy as np
import pytest

from mrgingham_amd import synth
from oracle import oracle

import cc_cases
import fcc_cases

live = pytest.mark.skipif(not oracle.have_reference_fcc(), reason="oracle/_ref/libfcc_*.so not built")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _same_refine(got, want):
    return got[2] == want[2] and np.array_equal(got[1], want[1]) and _same_bits(got[0], want[0])


# ----------------------------------------------------------------------------- on images (libfcc_ref.so)

def _frames():
    checker = (((np.arange(240).reshape(-1, 1) // 3 + np.arange(320).reshape(1, -1) // 3) & 1) * 200 + 20).astype(np.uint8)
    aspect = np.zeros((33, 32767), np.uint8)                    # the widest frame int16 coordinates hold
    aspect[:, :1280] = synth.board_frame(1280, 33, 10, 4).numpy()
    aspect[:, -640:] = synth.noise_frame(640, 33, 6, smooth=1).numpy()
    return {
        "board10_640x480": synth.board_frame(640, 480, 10, 0).numpy(),
        "board14_1280x960": synth.board_frame(1280, 960, 14, 1).numpy(),
        "cluttered_640x480": synth.cluttered_board_frame(640, 480, 10, 2).numpy(),
        "white_noise_411x299": synth.noise_frame(411, 299, 1).numpy(),
        "smoothed_noise_333x251": synth.noise_frame(333, 251, 2, smooth=2).numpy(),
        "ragged_board_1001x777": synth.board_frame(1001, 777, 8, 3).numpy(),
        "checker3px_320x240": checker,
        "aspect_32767x33": aspect,
    }


@pytest.fixture(scope="module")
def frames():
    return _frames()


FRAME_NAMES = ["board10_640x480", "board14_1280x960", "cluttered_640x480", "white_noise_411x299",
               "smoothed_noise_333x251", "ragged_board_1001x777", "checker3px_320x240", "aspect_32767x33"]


@live
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_images_detect_refine_and_chain_equal_upstream(frames, name):
    img = frames[name]
    found = {}
    for L in range(4):
        found[L] = oracle.find_corners(img, L)
        assert np.array_equal(found[L], oracle.ref_find_corners(img, L)), (name, "detect", L)
    for L in range(3):                                          # every single refine step, from upstream's own candidates
        pts = found[L + 1].astype(np.float64) / 1000.0
        lv = np.full(len(pts), L + 1, np.int8)
        if len(lv) > 2:
            lv[1] = L                                           # one point that is not refinable at this level
        assert _same_refine(oracle.refine_corners(pts, lv, img, L), oracle.ref_refine_corners(pts, lv, img, L)), (name, "refine", L)
    for start in (3, 2, 1):
        wp, wl = oracle.ref_chain(img, start)
        gp, gl = oracle.chain(img, start)
        assert np.array_equal(gl, wl) and _same_bits(gp, wp), (name, "chain", start)
    if name.startswith("board"):
        assert len(found[0]) >= 60 and len(found[2]) >= 30      # the comparison is of something


@live
def test_frames_are_what_the_comparison_needs(frames):
    assert list(frames) == FRAME_NAMES
    assert all(f.shape[0] <= 960 and f.shape[1] <= 1280 for n, f in frames.items() if n != "aspect_32767x33")
    assert frames["aspect_32767x33"].shape == (33, 32767)
    assert len(oracle.ref_find_corners(frames["aspect_32767x33"], 0)) > 0
    assert len(oracle.ref_find_corners(frames["checker3px_320x240"], 0)) > 100
    pts, lv = oracle.ref_chain(frames["board10_640x480"], 3)
    assert (lv == 0).sum() >= 50


@live
def test_error_returns_equal_upstream():
    """find_chessboard_corners.cc:433-441, :461-466: the restatement returns None exactly where upstream gives up."""
    img = synth.board_frame(160, 120, 10, 0).numpy()
    wide = np.zeros((120, 200), np.uint8)
    wide[:, :160] = img
    for image, level in [(img, -1), (img, 11), (wide[:, :160], 0), (wide[:, :160], 1), (np.zeros((10, 10), np.uint8), 0),
                         (img[:1], 0), (wide[:1, :160], 0)]:
        got, want = oracle.find_corners(image, level), oracle.ref_find_corners(image, level)
        assert (got is None) == (want is None), (image.shape, level)
        assert got is None or np.array_equal(got, want)


# ----------------------------------------------------------------------------- on responses (libfcc_resp_ref.so)

@live
def test_handbuilt_detect_cases_equal_upstream_and_their_hand_derived_values():
    cases = fcc_cases.response_detect_cases()
    assert len(cases) >= 50
    for name, d, img, level, expected in cases:
        want = oracle.ref_cc_detect_on_response(d, img, level)
        assert np.array_equal(oracle.cc_detect_on_response(d, img, level), want), name
        if expected is not None:
            assert want.tolist() == expected, name


@live
def test_handbuilt_refine_cases_equal_upstream_and_their_hand_derived_values():
    for name, pts, lv, d, img, level, expected in fcc_cases.response_refine_cases():
        want = oracle.ref_cc_refine_on_response(pts, lv, d, img, level)
        assert _same_refine(oracle.cc_refine_on_response(pts, lv, d, img, level), want), name
        if expected is not None:
            ep, el, en = expected
            assert want[2] == en and want[1].tolist() == el and np.array_equal(want[0], ep), name


def test_large_cases_are_large():
    (n1, d1, img1, e1), (n2, d2, _, e2) = cc_cases.large_detect_cases()
    assert (d1 > 15).sum() > 2048 and (d2 > 15).sum() > 2048
    assert len(oracle.cc_detect_on_response(d1, img1)) == 1 and e2 == []
    d = [c for c in cc_cases.detect_cases() if c[0].startswith("208-pixel")][0][1]
    assert (d > 15).sum() > 128


@live
@pytest.mark.parametrize("shape,nblobs,noise", [((48, 64), 12, 0.0), ((96, 131), 60, 0.002), ((97, 129), 80, 0.01),
                                                ((240, 333), 300, 0.004), ((64, 1001), 200, 0.003),
                                                ((600, 77), 150, 0.003), ((15, 15), 3, 0.1), ((16, 40), 6, 0.05)])
def test_random_sparse_responses_equal_upstream(shape, nblobs, noise):
    """The generator and the shapes of test_gpu_cc_rules.py: detection, then refinement about the hot pixels."""
    ds, imgs = fcc_cases.random_sparse_batch(shape, nblobs, noise, B=6)
    total = 0
    for f, (d, img) in enumerate(zip(ds, imgs)):
        want = oracle.ref_cc_detect_on_response(d, img)
        assert np.array_equal(oracle.cc_detect_on_response(d, img), want), (shape, f)
        total += len(want)
        if (d > 15).any():
            level = f % 3
            pts, lv = fcc_cases.random_refine_points(np.random.RandomState(f), d, level)
            assert _same_refine(oracle.cc_refine_on_response(pts, lv, d, img, level),
                                oracle.ref_cc_refine_on_response(pts, lv, d, img, level)), (shape, f, "refine")
    assert total > 0 or shape[0] < 48


@live
def test_dense_texture_equals_upstream():
    h, w = 64, 96
    d = np.random.RandomState(5).randint(16, 400, size=(h, w)).astype(np.int16)
    img = cc_cases.flat_img(h, w)
    want = oracle.ref_cc_detect_on_response(d, img)
    assert np.array_equal(oracle.cc_detect_on_response(d, img), want)
    pts, lv = fcc_cases.random_refine_points(np.random.RandomState(6), d, 0)
    assert _same_refine(oracle.cc_refine_on_response(pts, lv, d, img, 0), oracle.ref_cc_refine_on_response(pts, lv, d, img, 0))


# ----------------------------------------------------------------------------- which case meets which rule

# Every rule of find_chessboard_corners.cc:159-267 (the fill) and :329-397 (the seed loops), and the cases of
# cc_cases.py that meet it on purpose, by the beginning of their names.  "D:" a detect case, "R:" a refine case,
# "L:" a large detect case.
RULES = {
    ":162-163 coordinates outside the image are invalid": ["R:point at the image corner", "R:seeds about (int)(x+0.5)"],
    ":169 response > 15, strict": ["D:15 neither seeds nor extends", "D:16 > 15 but not"],
    ":27/:170 response > running max >> 4, strict": ["D:18 is not > 18", "D:19 > 18 joins", "D:peak 32767: 2047", "D:peak 32767: 2048"],
    ":170 the bar moves with the maximum met so far: taken before the peak": ["D:running max: small pixel accumulated BEFORE"],
    ":170 ... rejected after the peak": ["D:running max: big pixel first"],
    ":176 strict >: the first of equal maxima stays the peak": ["D:equal peaks: the first (seed, x=9)", "D:equal peaks: variance is high about the first",
                                                               "D:equal peaks: variance is high about the second"],
    ":183-186 weighted sums": ["D:two pixels: weighted centroid"],
    ":205 at least 2 pixels": ["D:single pixel: N < 2"],
    ":206 peak > 120, strict": ["D:peak 120 is not > 120", "D:peak 121 passes"],
    ":207/:52-53 window against the left side": ["D:variance window leaves the image at x_peak = 9", "D:variance window fits at x_peak = 10"],
    ":52-53 ... the right side": ["D:variance window fits at x_peak = w-11", "D:variance window leaves the image at x_peak = w-10"],
    ":52-53 ... the top": ["D:variance window leaves the image at y_peak = 9", "D:variance window fits at y_peak = 10"],
    ":52-53 ... the bottom": ["D:variance window fits at y_peak = h-11", "D:variance window leaves the image at y_peak = h-10"],
    ":69/:80/:87 truncated mean and variance, > 400 strict": ["D:variance exactly 400", "D:variance 400.51 truncates", "D:variance 401 passes",
                                                             "D:low-variance window rejects"],
    ":216-221 margin, column 7 / w-8": ["D:blob reaching column 7", "D:the same blob one column to the right", "D:blob reaching column w-8",
                                        "D:the same blob one column to the left"],
    ":216-221 margin, row 7 / h-8": ["D:blob reaching row 7", "D:the same blob one row down", "D:blob reaching row h-8", "D:the same blob one row up"],
    ":223/:243 a pixel pushed twice is taken once": ["D:2x2 block: duplicate pushes"],
    ":245 a rejected pixel is zeroed": ["D:16 > 15 but not", "D:touched component is dropped yet zeroes"],
    ":250/:259 a dropped component has consumed its pixels; a later seed finds the remainder": [
        "D:seed order: chain 100-1900-100-100", "D:touched component is dropped yet zeroes", "L:3841-pixel component reaching column 7"],
    ":252-255 stack order +x, -x, +y, -y": ["D:running max: small pixel accumulated BEFORE", "D:running max: big pixel first"],
    ":104/:127 the list grows past 128 entries": ["D:208-pixel component", "L:3840-pixel component inside the ring"],
    ":332-333 seeds only in [8, w-8) x [8, h-8)": ["D:column 7 alone is never a seed"],
    ":332-353 output in raster order of the seeds": ["D:three blobs: output in seed raster order"],
    ":319/:346-351 level scaling and x1000 rounding": ["D:two pixels: weighted centroid (:262-263), *1000 rounding (:350-351) @ level 1",
                                                      "D:two pixels: weighted centroid (:262-263), *1000 rounding (:350-351) @ level 3",
                                                      "D:three blobs: output in seed raster order @ level 3"],
    ":362 only points tagged level + 1": ["R:only points tagged level+1", "R:levels 0, 1, 3, -1 are skipped"],
    ":369-372 (int)(x + 0.5) truncates towards zero": ["R:seeds about (int)(x+0.5)", "R:wrapped negative seed truncates"],
    ":379-382 3x3 seeds": ["R:3x3 seed neighbourhood"],
    ":159/:124/:381-382 int seeds through int16_t parameters": ["R:seeds at +-65536+k and +-131072+k wrap"],
    ":358-396 the response mutates between points": ["R:the response mutates between points", "R:two points share one blob"],
    ":367-372/:390-393 full-resolution coordinates in, rescaled out, level and count updated": ["R:level 1: point given in full-resolution"],
}


def test_every_rule_has_a_case():
    names = (["D:" + c[0] for c in fcc_cases.response_detect_cases()] + ["L:" + c[0] for c in cc_cases.large_detect_cases()] +
             ["R:" + c[0] for c in fcc_cases.response_refine_cases()])
    assert len(RULES) >= 30
    for rule, prefixes in RULES.items():
        assert prefixes, rule
        for p in prefixes:
            assert any(n.startswith(p) for n in names), (rule, p)


# ----------------------------------------------------------------------------- known answers that travel

def _replay(fn_detect_resp, fn_refine_resp, fn_detect, fn_refine, fn_chain):
    kat = fcc_cases.load_kat()
    images = {m["name"]: f["image"] for m, f in kat if m["kind"] == "image"}
    levels = {(m["name"], m["level"]): f["image"] for m, f in kat if m["kind"] == "level_image"}
    count = {}
    for m, f in kat:
        kind, tag = m["kind"], (m["kind"], m["name"], m.get("level", m.get("start")))
        if kind == "detect_on_response":
            assert np.array_equal(fn_detect_resp(f["d"], f["img"], m["level"]), f["out"]), tag
        elif kind == "refine_on_response":
            assert _same_refine(fn_refine_resp(f["pts"], f["lv"], f["d"], f["img"], m["level"]), (f["out_pts"], f["out_lv"], m["n"])), tag
        elif kind == "detect":
            assert np.array_equal(fn_detect(images[m["name"]], m["level"], levels.get((m["name"], m["level"]))), f["out"]), tag
        elif kind == "refine":
            got = fn_refine(f["pts"], f["lv"], images[m["name"]], m["level"], levels.get((m["name"], m["level"])))
            assert _same_refine(got, (f["out_pts"], f["out_lv"], m["n"])), tag
        elif kind == "chain":
            gp, gl = fn_chain(images[m["name"]], m["start"], {L: levels[(m["name"], L)] for L in (1, 2, 3)})
            assert np.array_equal(gl, f["out_lv"]) and _same_bits(gp, f["out_pts"]), tag
        count[kind] = count.get(kind, 0) + 1
    return count, images, levels


def test_restatement_replays_upstreams_recorded_answers():
    """Never skipped: the stored inputs through oracle.*, against what upstream answered when the file was written."""
    count, images, levels = _replay(
        oracle.cc_detect_on_response, oracle.cc_refine_on_response,
        lambda image, level, _: oracle.find_corners(image, level),
        lambda pts, lv, image, level, _: oracle.refine_corners(pts, lv, image, level),
        lambda image, start, _: oracle.chain(image, start))
    assert count["detect_on_response"] >= 50 and count["refine_on_response"] >= 10
    assert count["detect"] == 4 * len(images) and count["refine"] == 3 * len(images) and count["chain"] == 3 * len(images)
    assert all(im.shape[0] <= 96 and im.shape[1] <= 131 for im in images.values())
    # the recorded answers were given on these level images; the restatement's own are the same
    for (name, level), li in levels.items():
        assert np.array_equal(oracle.decimate(images[name], level), li), (name, level)
    assert os.path.getsize(fcc_cases.GOLDEN) <= 128 * 1024


@live
def test_recorded_answers_are_not_stale():
    """The file against the live reference build, and its hand-built cases against cc_cases.py as it is today: a case
    added or changed there has to be recorded again (the images are stored and stand for themselves)."""
    _replay(oracle.ref_cc_detect_on_response, oracle.ref_cc_refine_on_response, oracle.ref_find_corners,
            oracle.ref_refine_corners, oracle.ref_chain)             # (on the stored level images)
    kat = fcc_cases.load_kat()
    stored = [(m["name"], m["level"]) for m, _ in kat if m["kind"] == "detect_on_response"]
    assert stored == [(c[0], c[3]) for c in fcc_cases.response_detect_cases()]
    for (m, f), c in zip([e for e in kat if e[0]["kind"] == "detect_on_response"], fcc_cases.response_detect_cases()):
        assert np.array_equal(f["d"], c[1]) and np.array_equal(f["img"], c[2]), m["name"]
    assert [m["name"] for m, _ in kat if m["kind"] == "refine_on_response"] == [c[0] for c in fcc_cases.response_refine_cases()]
    for (m, f), c in zip([e for e in kat if e[0]["kind"] == "refine_on_response"], fcc_cases.response_refine_cases()):
        assert np.array_equal(f["pts"], c[1]) and np.array_equal(f["lv"], c[2]) and np.array_equal(f["d"], c[3]), m["name"]
