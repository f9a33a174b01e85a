"""Every entry point that reads or writes caller-owned frames, on views whose bytes lie more than 2 and 4 GiB from the
base pointer (tests/far_views.py has the geometry and the decoys; tests/test_far_views_model.py shows on a host model
that a reader or writer cutting an offset to 32 bits fails these tests).

Expected values are those of the entry point's own GPU test -- the CPU oracle, the numpy statements of tests/*_cases.py,
the checker of tests/pixel_products.py -- on a dense host copy of the frames; every comparison is equality.  Each case
also compares with the same call on a contiguous device copy (so a failure says whether the view or the operation is at
fault), and reads the input windows (decoys included) back unchanged.  Writers: the true rows hold the expected bytes,
the guard bands and every alias window still hold the sentinel.

The buffer (far_views.BUFFER_BYTES, about 6 GiB, never filled or read back whole) is allocated once, serves uint8 and
uint16 views alike, and is freed at module teardown; a second one of the same size holds the far payload and the output
of bayer_grey.  There is no third.

CASES (entry point x geometry)
  readers, uint8: chess_response (level 0; chess_variant 0 / 1 / 16 x clamp off / on), detect (levels 0, 2), chain (from
    level 3; sparse_refine 0 / 1 / 2), refine (level 0), pixel_products (chain from 3; level 0; level 2), decimate
    (levels 1 .. 3), box_blur (radius 1, 2), preprocess (CLAHE on / off), blobs, find_boards
      x far frames, phase 0 and phase 5 (pixel-only entry points: 320x72 and 314x72; the others 640x480 boards / dots)
      x far rows, the seven strides below at width w and w - 6 (pixel-only: 64x56 and 58x56; the others 640 and 634 x 480)
  readers, uint16: preprocess (CLAHE on / off) x far frames phase 0, 2; bayer_grey at 8 and 16 bit, input AND output far
  writers: pgm_unpack 8 / 16 bit, pnm_unpack (RGB 8 / 16 bit), bmp_unpack (24 bit), raw_unpack (p12), jpeg_idct,
    png_reconstruct (RGB 8 bit, grey 16 bit), tiff_decode (LZW), read_pgms, read_bmps
      x far frames both phases, far rows at the stride past 2^32
  far payload: pgm_unpack (8 bit) and raw_unpack (p12) from a [3, 2^31 + 2^22] payload

FAR-ROWS STRIDES (bytes; S from far_views.seam_strides, the product each launch guard compares with 2^31 - 1)
  frames 56 rows high (pixel-only entry points), pitch S/2 up to 16 (S/4 at the last: S/2 does not fit the buffer)
    chess16_ok-         S 17895696  (h+64)S 2147483520 <   (h+8)S 1145324544 <   hS 1002158976 <   (h-1)S  984263280
    chess16_ok+         S 17895712  (h+64)S 2147485440 >=  (h+8)S 1145325568 <   hS 1002159872 <   (h-1)S  984264160
    w16/pyramid/multi-  S 33554416  (h+64)S 4026529920 >=  (h+8)S 2147482624 <   hS 1879047296 <   (h-1)S 1845492880
    w16/pyramid/multi+  S 33554432  (h+64)S 4026531840 >=  (h+8)S 2147483648 >=  hS 1879048192 <   (h-1)S 1845493760
    typed_ok-           S 38347920  (h+64)S 4601750400 >=  (h+8)S 2454266880 >=  hS 2147483520 <   (h-1)S 2109135600
    typed_ok+           S 38347936  (h+64)S 4601752320 >=  (h+8)S 2454267904 >=  hS 2147484416 >=  (h-1)S 2109136480
    past2^32            S 78090320  (h+64)S 9370838400 >=  (h+8)S 4997780480 >=  hS 4373057920 >=  (h-1)S 4294967600 >= 2^32
  frames 480 rows high
    chess16_ok-         S  3947568  (h+64)S 2147476992 <   (h+8)S 1926413184 <   hS 1894832640 <   (h-1)S 1890885072
    chess16_ok+         S  3947584  (h+64)S 2147485696 >=  (h+8)S 1926420992 <   hS 1894840320 <   (h-1)S 1890892736
    w16/pyramid/multi-  S  4400576  (h+64)S 2393913344 >=  (h+8)S 2147481088 <   hS 2112276480 <   (h-1)S 2107875904
    w16/pyramid/multi+  S  4400592  (h+64)S 2393922048 >=  (h+8)S 2147488896 >=  hS 2112284160 <   (h-1)S 2107883568
    typed_ok-           S  4473920  (h+64)S 2433812480 >=  (h+8)S 2183272960 >=  hS 2147481600 <   (h-1)S 2143007680
    typed_ok+           S  4473936  (h+64)S 2433821184 >=  (h+8)S 2183280768 >=  hS 2147489280 >=  (h-1)S 2143015344
    past2^32            S  8966544  (h+64)S 4877799936 >=  (h+8)S 4375673472 >=  hS 4303941120 >=  (h-1)S 4294974576 >= 2^32
  "<": the guard passes (chess_v16 / the 16-pixel staging, the fused pyramid and the merged launch / the typed staging
  may run); ">=": it fails and the fallback runs (chess_v1 / the typed staging, the separate pyramid pass and single
  launches / STAGE_GENERIC).  Only the last stride puts rows 2^31 bytes and more from the base: the other six take the
  seam alone, and chain_info is asserted to say which side ran."""
import ctypes

import numpy as np
import pytest
import torch

import mrgingham_amd
from mrgingham_amd import synth
from oracle import oracle
from tests import bayer_cases, bmp_cases, far_views as fv, files_cases, pixel_products as pp, png_cases, pnm_cases, raw_cases
from tests import tiff_cases as tc
from tests.test_jpeg_io import case as jpeg_case

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- the buffers

class Pool:
    """the far buffers of this module: "frames" and "second" (the far payload, the output of bayer_grey), never more"""

    def __init__(self):
        self.live = {}

    def get(self, name):
        assert name in ("frames", "second")
        if name not in self.live:
            self.live[name] = torch.empty(fv.BUFFER_BYTES, dtype=torch.uint8, device="cuda")
        return self.live[name]

    def release(self):
        self.live.clear()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.release()


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def det_exact():
    d = mrgingham_amd.Detector(0)
    d.set_option("hot_capacity_shift", 0)          # one table entry per pixel: the lists are compared exactly
    yield d
    d.close()


def _writer(buf):
    def write(at, data):
        buf[at:at + len(data)].copy_(torch.from_numpy(np.ascontiguousarray(data)))
    return write


def _reader(buf):
    return lambda at, n: buf[at:at + n].cpu().numpy()


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:                        # (moved as its int16 image: the same bits)
        return torch.tensor(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.tensor(a).cuda()


def _host(t):
    t = t.contiguous()
    return (t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.uint16 else t.cpu().numpy())


TORCH_OF = {1: torch.uint8, 2: torch.uint16}


def _place(pool, g, frames):
    """frames [B, h, w] onto the far view with their decoys -> (view, the plan to read back)"""
    buf = pool.get("frames")
    plan = fv.coalesce(fv.input_plan(g, frames))
    fv.apply_plan(_writer(buf), plan)
    return g.torch_view(buf, TORCH_OF[g.es]), plan


def _same(a, b, where=""):
    """equality of nested lists / tuples / dicts of arrays and numbers"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), where
        for k in a:
            _same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}/{k}")
    elif a is None or b is None:
        assert a is None and b is None, where
    else:
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), where


# ---------------------------------------------------------------------------------------------------- frames

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def _frames(kind, B, h, w):
    """boards and dots are made 640 wide and cut to w: what a crop out of a wider frame is"""
    def make():
        if kind == "board":
            return np.ascontiguousarray(synth.board_batch(B, 640, h, gridn=10, seed0=300).numpy()[:, :, :w])
        if kind == "dots":
            return np.ascontiguousarray(np.stack([synth.dots_frame(640, h, 5, seed=1 + f).numpy() for f in range(B)])[:, :, :w])
        return np.random.default_rng(h * 1000 + w).integers(0, 256, (B, h, w), dtype=np.uint8)
    return _cached(("frames", kind, B, h, w), make)


def _per_frame(key, frames, fn):
    """fn(frame) for every frame, computed once per (key, frame bytes' identity)"""
    return [_cached((key, frames.shape, f, frames[f, ::7, ::5].tobytes()), lambda f=f: fn(frames[f])) for f in range(len(frames))]


# ---------------------------------------------------------------------------------------------------- readers, uint8

def _with_option(det, name, value, default, call):
    det.set_option(name, value)
    try:
        return call()
    finally:
        det.set_option(name, default)


def run_chess_response(det, t, frames, g, info):
    return {(v, c): _with_option(det, "chess_variant", v, 0, lambda: _host(det.chess_response(t, 0, clamp=c)))
            for v in (0, 1, 16) for c in (False, True)}


def want_chess_response(frames):
    ref = np.stack(_per_frame("chess", frames, lambda f: oracle.chess_response_5(f, fill=0)))
    return {(v, c): (np.maximum(ref, 0) if c else ref) for v in (0, 1, 16) for c in (False, True)}


def run_detect(det, t, frames, g, info):
    out = {}
    for level in (0, 2):
        xy, counts = det.detect(t, level, capacity=4096)
        xy, counts = xy.cpu().numpy(), counts.cpu().numpy()
        out[level] = [xy[f, :counts[f]] for f in range(len(frames))]
    return out


def want_detect(frames):
    return {level: _per_frame(("corners", level), frames, lambda f: oracle.find_corners(f, level)) for level in (0, 2)}


SPARSE_REFINE = (0, 1, 2)          # every value set_option("sparse_refine") takes in the shipped library


def run_chain(det, t, frames, g, info):
    out = {}
    for sr in SPARSE_REFINE:
        def call():
            pts, lv, npts = det.chain(t, start_level=3, max_points=1024)
            info[sr] = det.chain_info()
            return pts.cpu().numpy(), lv.cpu().numpy(), npts.cpu().numpy()
        pts, lv, npts = _with_option(det, "sparse_refine", sr, 1, call)
        out[sr] = [(pts[f, :npts[f]], lv[f, :npts[f]]) for f in range(len(frames))]
    return out


def want_chain(frames):
    one = _per_frame("chain", frames, lambda f: oracle.chain(f, 3))
    assert sum(len(lv) for _, lv in one) >= 50 * len(frames)          # corners are found: the refinement read the frame
    return {sr: one for sr in SPARSE_REFINE}


def _refine_inputs(frames):
    cands = _per_frame(("corners", 1), frames, lambda f: oracle.find_corners(f, 1))
    P = max(1, max(len(c) for c in cands))
    pts = np.zeros((len(frames), P, 2), np.float64)
    for f, c in enumerate(cands):
        pts[f, :len(c)] = c.astype(np.float64) / 1000.0
    return pts, np.full((len(frames), P), 1, np.int8), np.array([len(c) for c in cands], np.int32)


def run_refine(det, t, frames, g, info):
    pts, lv, n = _refine_inputs(frames)
    d_pts, d_lv = torch.from_numpy(pts).cuda(), torch.from_numpy(lv).cuda()
    nref = det.refine(t, 0, d_pts, d_lv, torch.from_numpy(n).cuda()).cpu().numpy()
    d_pts, d_lv = d_pts.cpu().numpy(), d_lv.cpu().numpy()
    return [(d_pts[f, :n[f]], d_lv[f, :n[f]], int(nref[f])) for f in range(len(frames))]


def want_refine(frames):
    pts, lv, n = _refine_inputs(frames)
    assert n.min() >= 50
    out = [oracle.refine_corners(pts[f, :n[f]], lv[f, :n[f]], frames[f], 0) for f in range(len(frames))]
    assert all(o[2] > 0 for o in out)
    return [(o[0], o[1], int(o[2])) for o in out]


PRODUCT_MODES = (("chain", 3), ("level", 0), ("level", 2))


def run_pixel_products(det, t, frames, g, info):
    """through the existing checker (the oracle's level image and clamped response, the list and the map held to the
    contract); what is returned for the comparison with the dense copy is what does not depend on the order of atomics"""
    out = {}
    for mode, level in PRODUCT_MODES:
        products = det.pixel_products(t, level, mode)
        for L, p in products.items():
            for f in range(len(frames)):
                want = _cached(("pp", L, frames.shape, f, frames[f, ::7, ::5].tobytes()), lambda: pp.expected_of(frames[f], L))
                try:
                    pp.check_level(pp.frame_products(p, f), frames[f], L, want)
                except pp.ProductError as e:
                    raise AssertionError(f"{mode} {level}: level {L}, frame {f}: {e}") from e
            out[mode, level, L] = {k: ([np.sort(x) for x in v] if k == "hot_xy" else v) for k, v in p.items() if k != "gidx"}
    return out


def run_decimate(det, t, frames, g, info):
    return {L: _host(det.decimate(t, L)) for L in (1, 2, 3)}


def want_decimate(frames):
    return {L: np.stack(_per_frame(("decimate", L), frames, lambda f: oracle.decimate(f, L))) for L in (1, 2, 3)}


def run_box_blur(det, t, frames, g, info):
    return {r: _host(det.box_blur(t, r)) for r in (1, 2)}


def want_box_blur(frames):
    return {r: np.stack(_per_frame(("blur", r), frames, lambda f: oracle.box_blur(f, r))) for r in (1, 2)}


def run_preprocess(det, t, frames, g, info):
    return {c: _host(det.preprocess(t, clahe=c, blur_radius=1)) for c in (True, False)}


def want_preprocess(frames):
    fn = oracle.preprocess16 if frames.dtype == np.uint16 else oracle.preprocess
    return {c: np.stack(_per_frame(("pre", c), frames, lambda f: fn(f, clahe=c, blur_radius=1))) for c in (True, False)}


def run_blobs(det, t, frames, g, info):
    return det.blobs(t, nthreads=2)


def want_blobs(frames):
    out = _per_frame("blobs", frames, lambda f: oracle.find_blobs(f).astype(np.int32))
    assert all(len(o) >= 20 for o in out)
    return out


def run_find_boards(det, t, frames, g, info):
    boards, found = det.find_boards(t, gridn=10, nthreads=2)
    return [boards[f] if found[f] >= 0 else None for f in range(len(frames))]


def want_find_boards(frames):
    out = _per_frame("board", frames, lambda f: mrgingham_amd.find_board(np.ascontiguousarray(f), gridn=10))
    assert all(o is not None for o in out)
    return out


# entry point -> (frame kind, needs the large frames, run, expected or None where run checks for itself, detector fixture)
READERS = {
    "chess_response": ("noise", False, run_chess_response, want_chess_response, "det"),
    "detect": ("board", True, run_detect, want_detect, "det"),
    "chain": ("board", True, run_chain, want_chain, "det"),
    "refine": ("board", True, run_refine, want_refine, "det"),
    "pixel_products": ("board", True, run_pixel_products, None, "det_exact"),
    "decimate": ("noise", False, run_decimate, want_decimate, "det"),
    "box_blur": ("noise", False, run_box_blur, want_box_blur, "det"),
    "preprocess": ("noise", False, run_preprocess, want_preprocess, "det"),
    "blobs": ("dots", True, run_blobs, want_blobs, "det"),
    "find_boards": ("board", True, run_find_boards, want_find_boards, "det"),
}
LARGE, SMALL_ROWS, SMALL_FRAMES = (640, 480), (64, 56), (320, 72)
READER_GEOMETRIES = [("far-frames", ph, dw) for ph in fv.PHASES[1] for dw in (0, 6)] + [("far-rows", n, dw) for n in fv.FAR_ROWS for dw in (0, 6)]


def _reader_geometry(large, kind, which, dw):
    if kind == "far-frames":
        w, h = LARGE if large else SMALL_FRAMES
        return fv.far_frames(h, w - dw, 1, which)
    w, h = LARGE if large else SMALL_ROWS
    return fv.far_rows(h, w - dw, which)


def _expected_fused(g, view):
    """chess_pyramid_ok (chess.hip:955): whole 16 x 8 cells, everything on 16-byte boundaries, and the launch guard"""
    return int(g.w % 16 == 0 and g.h % 8 == 0 and g.stride % 16 == 0 and g.pitch % 16 == 0 and view.data_ptr() % 16 == 0
               and fv.guard_passes(g.h, g.stride, fv.V1_ROWS_AHEAD))


# (the large frames go onto the far frames at full width only: there the phase is what misaligns them)
READER_CASES = [(e, g) for e in READERS for g in READER_GEOMETRIES if not (READERS[e][1] and g[0] == "far-frames" and g[2])]


@pytest.mark.parametrize("entry,geometry", READER_CASES, ids=[f"{e}-{g[0]}-{g[1]}-w{'-6' if g[2] else ''}" for e, g in READER_CASES])
def test_reader_of_uint8_views(request, pool, entry, geometry):
    kind, large, run, want, fixture = READERS[entry]
    det = request.getfixturevalue(fixture)
    g = _reader_geometry(large, *geometry)
    frames = _frames(kind, g.B, g.h, g.w)
    view, plan = _place(pool, g, frames)
    assert view.data_ptr() == pool.get("frames").data_ptr() + g.origin and not view.is_contiguous()
    info_far, info_dense = {}, {}
    far = run(det, view, frames, g, info_far)
    dense = run(det, _dev(frames), frames, g, info_dense)
    if want is not None:
        _same(dense, want(frames), f"{entry}: the contiguous copy against the oracle")
    _same(far, dense, f"{entry} on {g.name}: the far view against the contiguous copy")
    assert fv.plan_mismatches(_reader(pool.get("frames")), plan) == []               # the frames and their decoys are as placed
    if entry == "chain":
        print(g.describe(), "chain_info far", info_far, "dense", info_dense)
        assert info_far[2] == (0, -1) and info_dense[2] == (0, -1)                   # the sparse schedule
        for sr in (0, 1):
            assert info_far[sr][0] == _expected_fused(g, view), (sr, info_far)       # the side of the guard that ran
            assert info_dense[sr][0] == int(g.w % 16 == 0 and g.h % 8 == 0)


# ---------------------------------------------------------------------------------------------------- readers, uint16

@pytest.mark.parametrize("phase", fv.PHASES[2])
def test_preprocess_of_uint16_far_frames(pool, det, phase):
    g = fv.far_frames(480, 640, 2, phase)
    boards = _frames("board", 3, 480, 640).astype(np.uint16)
    frames = _cached(("deep", phase), lambda: np.stack([boards[0] * 16 + 300, boards[1] * 257, boards[2] * 200 + 11]).astype(np.uint16))
    view, plan = _place(pool, g, frames)
    far = run_preprocess(det, view, frames, g, {})
    dense = run_preprocess(det, _dev(frames), frames, g, {})
    _same(dense, want_preprocess(frames), "preprocess16: the contiguous copy against the oracle")
    _same(far, dense, "preprocess16: the far view against the contiguous copy")
    assert fv.plan_mismatches(_reader(pool.get("frames")), plan) == []


@pytest.mark.parametrize("es,phase,pattern", [(1, 0, "rggb"), (1, 5, "gbrg"), (2, 0, "grbg"), (2, 2, "bggr")])
def test_bayer_grey_with_input_and_output_far(pool, det, es, phase, pattern):
    """the input in the first far buffer, the output in the second (the entry point refuses frames that interleave)"""
    h, w = 70, 130
    g = fv.far_frames(h, w, es, phase)
    frames = bayer_cases.random_frames(3, h, w, np.uint8 if es == 1 else np.uint16, seed=es + phase)
    want = np.stack([bayer_cases.grey(f, pattern) for f in frames]).astype(frames.dtype)
    out = pool.get("second")
    fv.apply_plan(_writer(out), fv.output_plan(g))
    view, plan = _place(pool, g, frames)
    det.bayer_grey(view, pattern, out=g.torch_view(out, TORCH_OF[es]))
    torch.cuda.synchronize()
    _same(_host(det.bayer_grey(_dev(frames), pattern)), want, "bayer_grey: the contiguous copy against the numpy statement")
    assert fv.plan_mismatches(_reader(out), fv.output_plan(g, want)) == []
    assert fv.plan_mismatches(_reader(pool.get("frames")), plan) == []
    with pytest.raises(RuntimeError, match="overlap"):                 # both in one buffer, 16 MiB apart: their extents interleave
        det.bayer_grey(view, pattern, out=fv.Geometry("beside", 3, h, w, es, g.origin + 2**24, g.pitch, g.stride).torch_view(pool.get("frames"), TORCH_OF[es]))


# ---------------------------------------------------------------------------------------------------- writers

def _payload16(raw, nbytes):
    """[B, nbytes] bytes -> [B, P] with P a multiple of 16, the tail 0xEE"""
    B = len(raw)
    out = np.full((B, (nbytes + 15) // 16 * 16), 0xEE, np.uint8)
    for f in range(B):
        out[f, :nbytes] = np.frombuffer(raw[f], np.uint8)[:nbytes] if isinstance(raw[f], bytes) else raw[f].reshape(-1)[:nbytes]
    return out


def w_pgm_unpack(bits):
    def make(B, h, w, tmp):
        nb = h * w * bits // 8
        pay = np.random.default_rng(bits).integers(0, 256, (B, (nb + 15) // 16 * 16), dtype=np.uint8)
        want = pay[:, :nb].reshape(B, h, w) if bits == 8 else pay[:, :nb].copy().view(">u2").astype(np.uint16).reshape(B, h, w)
        d_pay = _dev(pay)
        return (lambda det, out: det.pgm_unpack(d_pay, h, w, bits, out=out)), want
    return make


def w_pnm_unpack(bits):
    def make(B, h, w, tmp):
        samples = [pnm_cases.random_samples(w, h, bits, 3, seed=f) for f in range(B)]
        want = np.stack([pnm_cases.expected(s, bits, 3) for s in samples])
        d_pay = _dev(_payload16([pnm_cases.raster(s, bits) for s in samples], h * pnm_cases.row_bytes(w, bits, 3)))
        return (lambda det, out: det.pnm_unpack(d_pay, h, w, bits, 3, out=out)), want
    return make


def w_bmp_unpack(B, h, w, tmp):
    pixels = [bmp_cases.random_pixels(w, h, 24, seed=f) for f in range(B)]
    want = np.stack([bmp_cases.expected(p, 24) for p in pixels])
    d_pay = _dev(_payload16([bmp_cases.pack_rows(p, 24)[::-1].tobytes() for p in pixels], h * bmp_cases.row_bytes(w, 24)))   # bottom-up
    return (lambda det, out: det.bmp_unpack(d_pay, None, h, w, 24, out=out)), want


def w_raw_unpack(B, h, w, tmp):
    want = raw_cases.random_frames(B, h, w, "p12", seed=3)
    d_pay = _dev(raw_cases.payload(want, "p12"))
    return (lambda det, out: det.raw_unpack(d_pay, h, w, "p12", out=out)), want


JPEGS = ("noise_48x64_grey", "noise_48x64_444", "noise_48x64_420")        # 48 wide, 64 high: the fixtures of test_gpu_jpeg.py


def w_jpeg_idct(B, h, w, tmp):
    cases = [jpeg_case(n) for n in JPEGS[:B]]
    parts = [mrgingham_amd.jpeg_coefficients(c.data) for c in cases]
    assert all(p[2] == (h, w) for p in parts)
    d_coef, d_quant = _dev(np.stack([p[0] for p in parts])), _dev(np.stack([p[1] for p in parts]))
    return (lambda det, out: det.jpeg_idct(d_coef, d_quant, h, w, out=out)), np.stack([c.luma for c in cases])


def w_png_reconstruct(ct, bits):
    def make(B, h, w, tmp):
        imgs = [png_cases.random_image(w, h, ct, bits, seed=40 + f) for f in range(B)]
        want = np.stack([png_cases.grey_of(i, ct) for i in imgs])
        d_scan = _dev(np.stack([png_cases.scanlines(i, ct, bits, ("random", f)) for f, i in enumerate(imgs)]))
        return (lambda det, out: det.png_reconstruct(d_scan, h, w, bits, ct, out=out)), want
    return make


def w_tiff_decode(B, h, w, tmp):
    imgs = [tc.random_image(w, h, 1, 8, seed=50 + f) for f in range(B)]
    datas = [tc.encode(i, compression=tc.LZW, rows_per_strip=5)[0] for i in imgs]

    def call(det, out):
        frames, status, strip_status = det.tiff_decode(datas, out=out)
        assert status.tolist() == [0] * B and not strip_status.any()
        return frames
    return call, np.stack(imgs)


def _file_loader(entry_name, names, B, h, w, pass_bits):
    def call(det, out):
        if out is None:
            out = torch.zeros((B, h, w), dtype=torch.uint8, device="cuda")
        arr = (ctypes.c_char_p * B)(*names)
        status = np.full((B,), -1, dtype=np.int32)
        torch.cuda.synchronize()
        det._check(getattr(det.L, entry_name)(det.ctx, arr, B, w, h, *((8,) if pass_bits else ()), out.data_ptr(), out.stride(0),
                                              out.stride(1), 2, status.ctypes.data))
        assert status.tolist() == [0] * B
        return out
    return call


def w_read_pgms(B, h, w, tmp):
    want = np.random.default_rng(7).integers(0, 256, (B, h, w), dtype=np.uint8)
    names = []
    for f in range(B):
        files_cases.write_pgm(str(tmp / f"far{f}.pgm"), want[f])
        names.append(str(tmp / f"far{f}.pgm").encode())
    return _file_loader("mrgingham_amd_read_pgms_batch", names, B, h, w, True), want


def w_read_bmps(B, h, w, tmp):
    pixels = [bmp_cases.random_pixels(w, h, 24, seed=60 + f) for f in range(B)]
    names = []
    for f in range(B):
        (tmp / f"far{f}.bmp").write_bytes(bmp_cases.write(pixels[f], 24, top_down=bool(f & 1)))
        names.append(str(tmp / f"far{f}.bmp").encode())
    return _file_loader("mrgingham_amd_read_bmps_batch", names, B, h, w, False), np.stack([bmp_cases.expected(p, 24) for p in pixels])


# entry point -> (sample bytes, make(B, h, w, tmp_path) -> (call(det, out), expected [B, h, w]), fixed (h, w) or None)
WRITERS = {
    "pgm_unpack8": (1, w_pgm_unpack(8), None), "pgm_unpack16": (2, w_pgm_unpack(16), None),
    "pnm_unpack8": (1, w_pnm_unpack(8), None), "pnm_unpack16": (2, w_pnm_unpack(16), None),
    "bmp_unpack": (1, w_bmp_unpack, None), "raw_unpack": (2, w_raw_unpack, None),
    "jpeg_idct": (1, w_jpeg_idct, (64, 48)),
    "png_reconstruct8": (1, w_png_reconstruct(2, 8), None), "png_reconstruct16": (2, w_png_reconstruct(0, 16), None),
    "tiff_decode": (1, w_tiff_decode, None),
    "read_pgms": (1, w_read_pgms, None), "read_bmps": (1, w_read_bmps, None),
}
WRITER_GEOMETRIES = ["far-frames/first-phase", "far-frames/second-phase", "far-rows/past2^32"]


def _writer_geometry(es, shape, which):
    """whole 16-byte words on the aligned phase (64 wide), ragged heads and tails elsewhere (58 wide)"""
    if which == "far-frames/first-phase":
        h, w = shape or (56, 64)
        return fv.far_frames(h, w, es, fv.PHASES[es][0])
    h, w = shape or (56, 58)
    return fv.far_frames(h, w, es, fv.PHASES[es][1]) if which == "far-frames/second-phase" else fv.far_rows(h, w, "past2^32", es)


def _check_writer(pool, det, g, call, want):
    assert want.shape == (g.B, g.h, g.w) and want.dtype == (np.uint8 if g.es == 1 else np.uint16)
    buf = pool.get("frames")
    fv.apply_plan(_writer(buf), fv.output_plan(g))
    got = call(det, g.torch_view(buf, TORCH_OF[g.es]))
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() + g.origin
    _same(_host(call(det, None)), want, "the contiguous output against the expected frames")
    bad = fv.plan_mismatches(_reader(buf), fv.output_plan(g, want))
    assert bad == [], (g.describe(), "true rows, guard bands or alias windows differ at (window, byte)", bad[:4])


@pytest.mark.parametrize("geometry", WRITER_GEOMETRIES)
@pytest.mark.parametrize("entry", list(WRITERS))
def test_writer_into_far_views(pool, det, tmp_path, entry, geometry):
    es, make, shape = WRITERS[entry]
    g = _writer_geometry(es, shape, geometry)
    call, want = make(g.B, g.h, g.w, tmp_path)
    _check_writer(pool, det, g, call, want)


# ---------------------------------------------------------------------------------------------------- a far payload

@pytest.mark.parametrize("entry", ["pgm_unpack8", "raw_unpack"])
def test_unpack_from_a_far_payload(pool, det, entry):
    """Rows of a contiguous [3, 2^31 + 2^22] payload carry the frames: payload row 1 begins beyond 2^31 bytes, row 2 beyond
    2^32.  The payload begins at its allocation, so only the aliases inside it can hold a decoy (row 2 cut to 32 bits lies
    in row 0; row 1 taken as int32 lies below the allocation: pgm_unpack_kernel and RawRows::row multiply in 64 bits)."""
    B, h, w = 3, 56, 58
    P = fv.FAR_PITCH
    assert P % 16 == 0
    if entry == "pgm_unpack8":
        small = np.random.default_rng(9).integers(0, 256, (B, h * w), dtype=np.uint8)
        want = small.reshape(B, h, w)
        call = lambda pay, out: det.pgm_unpack(pay, h, w, 8, out=out)
        es = 1
    else:
        want = raw_cases.random_frames(B, h, w, "p12", seed=9)
        small = raw_cases.payload(want, "p12")
        call = lambda pay, out: det.raw_unpack(pay, h, w, "p12", out=out)
        es = 2
    n = small.shape[1]
    pay = pool.get("second")[:B * P]
    assert pay.data_ptr() % 16 == 0 and B * P <= fv.BUFFER_BYTES
    plan, inside = [], 0
    for f in range(B):
        plan.append((f * P, small[f]))
        for a in sorted({fv.TRUNCATIONS[k](f * P) for k in ("uint32", "int32")} - {f * P}):
            if 0 <= a and a + n <= B * P:
                assert all(a + n <= k * P or k * P + n <= a for k in range(B))        # apart from every true payload
                plan.append((a, ~small[f]))
                inside += 1
    assert inside == 1
    fv.apply_plan(_writer(pay), plan)
    g = fv.far_frames(h, w, es, fv.PHASES[es][1])
    _check_writer(pool, det, g, lambda det, out: call(pay.view(B, P) if out is not None else _dev(small), out), want)
    assert fv.plan_mismatches(_reader(pay), plan) == []
