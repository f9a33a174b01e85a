"""Cases of tests/test_gpu_scratch_fill.py: the frames, file lists and expected values of every entry point that is run
on filled scratch (set_option "scratch_fill" / "scratch_fill_now", the variable MRGINGHAM_AMD_SCRATCH_FILL; csrc/ctx.h).

Every expected value is the yardstick the entry point's own test uses -- the C oracle, the array a file was written from,
read_image on the same file, the luma plane of a committed JPEG fixture -- computed once per process and shared.  Nothing
here is computed by the code under test, and nothing is larger than 640 x 480."""
import functools
import os

import numpy as np

FILL_BYTES = (0x7F, 0xFF)     # large positive int16 / 2e9 counts / 1e306 doubles; -1 indices, NaN doubles, the largest sort key
W, H, GRIDN = 640, 480, 10
SETS = 3                      # option "scratch_sets" of the A-then-B sequences: a call is made this often, so every set sees it


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev16(a):
    """numpy uint16 -> device torch.uint16 (through int16: the copy does not depend on uint16 support)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def detector(byte, **options):
    """A fresh Detector whose every allocation is filled with `byte` (None: a plain one), with `options` set."""
    import mrgingham_amd
    det = mrgingham_amd.Detector(0)
    if byte is not None:
        det.set_option("scratch_fill", byte)
    for name, value in options.items():
        det.set_option(name, value)
    return det


def fill_now(det, byte):
    """Everything the context owns by now gets `byte` -- and it owns something, so the fill is not vacuous."""
    assert det.scratch_bytes() > 0
    det.set_option("scratch_fill_now", byte)


def first_use_then_reuse(byte, run, **options):
    """run(det, what) on a fresh filled Detector (first use of every buffer), and again after scratch_fill_now (reuse)."""
    det = detector(byte, **options)
    try:
        run(det, "first use")
        fill_now(det, byte)
        run(det, "reuse")
    finally:
        det.close()


def a_then_b(fill, call_a, check_b, **options):
    """call_a(det) SETS times, then check_b(det, what) SETS times on the same context; `fill`: None, or the byte of a
    scratch_fill_now in between."""
    det = detector(None, scratch_sets=SETS, **options)
    try:
        for _ in range(SETS):
            call_a(det)
        if fill is not None:
            fill_now(det, fill)
        for k in range(SETS):
            check_b(det, f"B call {k + 1} after A, fill {fill}")
    finally:
        det.close()


# ----------------------------------------------------------------------------------------------------------------------
# component search: detect, chain, refine, the two entry points on a caller's response
# ----------------------------------------------------------------------------------------------------------------------
class Search:
    """Frames [B, h, w] and what the oracle gives for them: detect[L][f] (int32 (n, 2)), chain[f] = (points, levels) from
    level 3, refine_in[f] / refine[f]: the level-1 candidates as points and their refinement at level 0, resp[f]: the
    clamped level-0 response, cc_detect[f] / cc_refine[f]: the search on that response."""

    def __init__(self, frames, detect_levels=(0, 2), on_response=True):
        from oracle import oracle
        self.frames = np.ascontiguousarray(frames)
        self.detect = {L: [oracle.find_corners(f, L) for f in self.frames] for L in detect_levels}
        self.chain = [oracle.chain(f, 3) for f in self.frames]
        self.refine_in, self.refine = [], []
        for f in self.frames:
            pts = oracle.find_corners(f, 1).astype(np.float64) / 1000.0
            lv = np.full(len(pts), 1, np.int8)
            self.refine_in.append((pts, lv))
            self.refine.append(oracle.refine_corners(pts, lv, f, 0))
        if on_response:
            self.resp = [oracle.clamped_response(f, 0)[0] for f in self.frames]
            self.cc_detect = [oracle.cc_detect_on_response(r, f, 0) for r, f in zip(self.resp, self.frames)]
            self.cc_refine = [oracle.cc_refine_on_response(p, l, r, f, 0)
                              for (p, l), r, f in zip(self.refine_in, self.resp, self.frames)]

    def points_batch(self):
        """the points of refine_in as one padded batch on the device -> (points, levels, npoints)"""
        import torch
        B, P = len(self.frames), max(1, max(len(l) for _, l in self.refine_in))
        tp = torch.zeros((B, P, 2), dtype=torch.float64)
        tl = torch.zeros((B, P), dtype=torch.int8)
        for f, (p, l) in enumerate(self.refine_in):
            tp[f, :len(l)] = torch.from_numpy(p)
            tl[f, :len(l)] = torch.from_numpy(l)
        return tp.cuda(), tl.cuda(), torch.tensor([len(l) for _, l in self.refine_in], dtype=torch.int32).cuda()


@functools.lru_cache(maxsize=None)
def search():
    """A board, a cluttered board, smoothed noise and an all-zero frame."""
    from mrgingham_amd import synth
    return Search(np.stack([synth.board_frame(W, H, GRIDN, 0).numpy(), synth.cluttered_board_frame(W, H, GRIDN, 2).numpy(),
                            synth.noise_frame(W, H, 4, smooth=2).numpy(), np.zeros((H, W), np.uint8)]))


def check_detect(det, s, level, what, capacity=8192):
    xy, counts = det.detect(dev(s.frames), level, capacity=capacity)
    xy, counts = xy.cpu().numpy(), counts.cpu().numpy()
    for f, want in enumerate(s.detect[level]):
        assert counts[f] == len(want) <= capacity, (what, "detect", level, f, int(counts[f]), len(want))
        assert np.array_equal(xy[f, :len(want)], want), (what, "detect", level, f)


def check_chain(det, s, what, max_points=1024):
    pts, lv, npts = det.chain(dev(s.frames), start_level=3, max_points=max_points)
    pts, lv, npts = pts.cpu().numpy(), lv.cpu().numpy(), npts.cpu().numpy()
    for f, (wp, wl) in enumerate(s.chain):
        assert npts[f] == len(wl) <= max_points, (what, "chain", f, int(npts[f]), len(wl))
        assert np.array_equal(lv[f, :len(wl)], wl) and np.array_equal(pts[f, :len(wl)], wp), (what, "chain", f)


def _check_refined(s, want, tp, tl, nref, what):
    tp, tl, nref = tp.cpu().numpy(), tl.cpu().numpy(), nref.cpu().numpy()
    for f, (wp, wl, wn) in enumerate(want):
        n = len(wl)
        assert nref[f] == wn, (what, f, int(nref[f]), wn)
        assert np.array_equal(tl[f, :n], wl) and np.array_equal(tp[f, :n], wp), (what, f)


def check_refine(det, s, what):
    tp, tl, n = s.points_batch()
    nref = det.refine(dev(s.frames), 0, tp, tl, n)
    _check_refined(s, s.refine, tp, tl, nref, (what, "refine"))


def check_on_response(det, s, what, capacity=8192):
    resp, imgs = dev(np.stack(s.resp)), dev(s.frames)
    xy, counts = det.cc_detect_on_response(resp, imgs, level=0, capacity=capacity)
    xy, counts = xy.cpu().numpy(), counts.cpu().numpy()
    for f, want in enumerate(s.cc_detect):
        assert counts[f] == len(want) <= capacity, (what, "cc_detect_on_response", f, int(counts[f]), len(want))
        assert np.array_equal(xy[f, :len(want)], want), (what, "cc_detect_on_response", f)
    tp, tl, n = s.points_batch()
    nref = det.cc_refine_on_response(resp, imgs, 0, tp, tl, n)
    _check_refined(s, s.cc_refine, tp, tl, nref, (what, "cc_refine_on_response"))


@functools.lru_cache(maxsize=None)
def leftover_search():
    """A: six full-size frames that leave the most behind (smoothed noise, cluttered boards).  B, two of them: three frames
    of the same size and three of half the size -- a clean board, an all-zero and a constant frame each."""
    from mrgingham_amd import synth
    a = np.stack([synth.noise_frame(W, H, 11, smooth=1).numpy(), synth.cluttered_board_frame(W, H, GRIDN, 5).numpy(),
                  synth.noise_frame(W, H, 12, smooth=2).numpy(), synth.cluttered_board_frame(W, H, GRIDN, 6).numpy(),
                  synth.noise_frame(W, H, 13, smooth=1).numpy(), synth.cluttered_board_frame(W, H, GRIDN, 7).numpy()])

    def clean(w, h, seed):
        return np.stack([synth.board_frame(w, h, GRIDN, seed, noise=False).numpy(), np.zeros((h, w), np.uint8), np.full((h, w), 128, np.uint8)])
    return a, Search(clean(W, H, 3), on_response=False), Search(clean(W // 2, H // 2, 4), on_response=False)


# ----------------------------------------------------------------------------------------------------------------------
# ChESS response
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chess_cases():
    """-> [(frames [3, h, w], level, variant or None, raw response per frame)]: level 2 through the context's level image
    with each response kernel forced (128 x 96), level 0 at a ragged size (97 wide, 130 tall)."""
    from oracle import oracle
    out = []
    for (w, h, level, variants) in ((128, 96, 2, (1, 16)), (97, 130, 0, (None,))):
        rng = np.random.RandomState(w * 3 + h)
        frames = rng.randint(0, 256, size=(3, h, w)).astype(np.uint8)
        want = [oracle.chess_response_5(oracle.decimate(f, level) if level else f, fill=0) for f in frames]
        out += [(frames, level, v, want) for v in variants]
    return out


def check_chess(det, what):
    for frames, level, variant, want in chess_cases():
        det.set_option("chess_variant", variant or 0)
        try:
            for clamp in (False, True):
                got = det.chess_response(dev(frames), level, clamp=clamp).cpu().numpy()
                for f in range(len(frames)):
                    assert np.array_equal(got[f], np.maximum(want[f], 0) if clamp else want[f]), (what, level, variant, clamp, f)
        finally:
            det.set_option("chess_variant", 0)


# ----------------------------------------------------------------------------------------------------------------------
# preprocessing
# ----------------------------------------------------------------------------------------------------------------------
def _pre_frames(w, h, seed):
    """a board with shading, smoothed noise, a constant frame: every tile histogram and both extrema differ"""
    from mrgingham_amd import synth
    yy, xx = np.mgrid[0:h, 0:w]
    shaded = (synth.board_frame(max(w, 64), max(h, 64), 4, seed).numpy()[:h, :w].astype(np.int64) * (xx + yy + 40) // (w + h + 40)).astype(np.uint8)
    return np.stack([shaded, synth.noise_frame(w, h, seed, smooth=1).numpy(), np.full((h, w), 77, np.uint8)])


@functools.lru_cache(maxsize=None)
def preprocess8_cases():
    """-> [(frames, {blur: expected per frame})]: 64 x 272 (the smallest fused geometry: W >= 32, tiles 34 rows tall), 64 x 271
    (padded tiles), 40 x 40 (the plain blend)."""
    from oracle import oracle
    out = []
    for (w, h, blurs) in ((64, 272, (1,)), (64, 271, (1,)), (40, 40, (0, 1, 2))):
        frames = _pre_frames(w, h, w + h)
        out.append((frames, {b: [oracle.preprocess(f, clahe=True, blur_radius=b) for f in frames] for b in blurs}))
    return out


def check_preprocess8(det, what, cases=None):
    for frames, want in (cases or preprocess8_cases()):
        d = dev(frames)
        for blur, w in want.items():
            got = det.preprocess(d, clahe=True, blur_radius=blur).cpu().numpy()
            for f in range(len(frames)):
                assert np.array_equal(got[f], w[f]), (what, "preprocess", frames.shape, blur, f)


def _range_frame(h, w, smin, R, rng):
    """values in [smin, smin + R - 1] with both ends present (as tests/test_gpu_preprocess16_paths.py makes them)"""
    smax = smin + R - 1
    f = rng.randint(smin, smax, (h, w))
    f[h // 4:h // 2, w // 3:w // 2] = rng.randint(smin, smax)
    f[(5 * h) // 16, w - 1] = smin
    f[h - 1, (3 * w) // 16] = smax
    return f.astype(np.uint16)


@functools.lru_cache(maxsize=None)
def preprocess16_cases():
    """-> [(frames uint16 [3, h, w], {blur: expected per frame})] at 64 x 64 and 72 x 50: value ranges 2 and 4097 (LDS
    histograms up to 4096 values, parts of 16 384 bins in global memory above) and 65536."""
    from oracle import oracle
    out = []
    for (w, h) in ((64, 64), (72, 50)):
        rng = np.random.RandomState(w * h)
        frames = np.stack([_range_frame(h, w, smin, R, rng) for smin, R in ((37, 2), (1000, 4097), (0, 65536))])
        base = [oracle.preprocess16(f, clahe=True, blur_radius=0) for f in frames]
        out.append((frames, {b: (base if b == 0 else [oracle.box_blur(x, b) for x in base]) for b in (0, 1, 2)}))
    return out


def check_preprocess16(det, what, cases=None):
    for frames, want in (cases or preprocess16_cases()):
        d = dev16(frames)
        for blur, w in want.items():
            got = det.preprocess(d, clahe=True, blur_radius=blur).cpu().numpy()
            for f in range(len(frames)):
                assert np.array_equal(got[f], w[f]), (what, "preprocess16", frames.shape, blur, f)


@functools.lru_cache(maxsize=None)
def leftover_preprocess():
    """A (8 and 16 bit): six frames of noise at 640 x 480.  B: three frames of 320 x 240 -- a clean board, an all-zero and a
    constant frame -- with their expected values."""
    from mrgingham_amd import synth
    from oracle import oracle
    a8 = np.stack([synth.noise_frame(W, H, 20 + k, smooth=k % 3).numpy() for k in range(6)])
    a16 = (a8.astype(np.uint16) * 257) ^ np.uint16(0x5a5a)
    w, h = W // 2, H // 2
    b8 = np.stack([synth.board_frame(w, h, GRIDN, 9, noise=False).numpy(), np.zeros((h, w), np.uint8), np.full((h, w), 128, np.uint8)])
    b16 = np.stack([b8[0].astype(np.uint16) * 16 + 300, np.zeros((h, w), np.uint16), np.full((h, w), 40000, np.uint16)])
    want8 = {1: [oracle.preprocess(f, clahe=True, blur_radius=1) for f in b8]}
    want16 = {1: [oracle.preprocess16(f, clahe=True, blur_radius=1) for f in b16]}
    return a8, a16, [(b8, want8)], [(b16, want16)]


# ----------------------------------------------------------------------------------------------------------------------
# blobs
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blob_case():
    """the hand-made shapes and a random scene of tests/test_gpu_blobs.py at 320 x 360, and an all-255 frame"""
    import random
    from oracle import oracle
    from test_gpu_blobs import _random_scene, _shapes
    frames = np.stack([_shapes(320, 360), _random_scene(random.Random(5), 320, 360), np.full((320, 360), 255, np.uint8)])
    return frames, [oracle.find_blobs(f) for f in frames]


@functools.lru_cache(maxsize=None)
def leftover_blobs():
    """A: four frames of smoothed noise (thousands of borders per threshold).  B: the shapes, an all-zero and a constant frame."""
    from mrgingham_amd import synth
    from oracle import oracle
    from test_gpu_blobs import _shapes
    a = np.stack([synth.noise_frame(360, 320, 30 + k, smooth=1 + k % 3).numpy() for k in range(4)])
    b = np.stack([_shapes(320, 360), np.zeros((320, 360), np.uint8), np.full((320, 360), 128, np.uint8)])
    return a, (b, [oracle.find_blobs(f) for f in b])


def check_blobs(det, what, case=None):
    frames, want = case or blob_case()
    got = det.blobs(dev(frames), nthreads=2)
    assert len(got) == len(want), what
    for f in range(len(want)):
        assert np.array_equal(np.asarray(got[f]).reshape(-1, 2), want[f]), (what, "blobs", f)


# ----------------------------------------------------------------------------------------------------------------------
# boards
# ----------------------------------------------------------------------------------------------------------------------
def mixed_batch(seed0):
    """_mixed_batch of tests/test_gpu_board.py at 640 x 480"""
    from test_gpu_board import _mixed_batch
    return _mixed_batch(seed0, W, H)


# ----------------------------------------------------------------------------------------------------------------------
# loaders
# ----------------------------------------------------------------------------------------------------------------------
class FileList:
    """One call of a loader: `paths`, the statuses it must give, per readable file the array it was written from (or None)
    -- read_image on the file is the other yardstick --, the sample depth of the frames, the Detector method and its
    keywords, the name of its chunk option."""

    def __init__(self, name, method, chunk_option, paths, status, source, bits=8, kw=None, options=None):
        self.name, self.method, self.chunk_option = name, method, chunk_option
        self.paths, self.status, self.source, self.bits = list(paths), list(status), list(source), bits
        self.kw, self.options = dict(kw or {}), dict(options or {})
        assert len(self.paths) == len(self.status) == len(self.source)
        assert -1 in self.status and self.status.count(0) >= 3      # an unreadable file; a full chunk of two and a partial one


def _put(directory, name, data):
    path = os.path.join(directory, name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def file_lists(directory):
    """Every loader list of the tests, written into `directory` -> {name: FileList}.  JPEG: the fixtures of
    tests/golden/jpeg_*_golden.npz (their luma planes are the expected frames); the others are written from arrays by the
    case helpers of their own tests."""
    import mrgingham_amd
    from test_jpeg_io import case
    from test_jpeg_scan import rst_case
    from tests import bmp_cases as bc, files_cases, png_cases, pnm_cases as pc, tiff_cases as tc, tiff_inflate_cases as ic
    directory = str(directory)
    out = {}

    # JPEG, 48 x 64: restart intervals in three samplings, a file without them, a progressive file (-1), a 16 x 16 file (-2)
    picks = [rst_case("noise_48x64_grey"), rst_case("noise_48x64_444_q100"), rst_case("nodri_48x64"), case("progressive_48x64"),
             rst_case("rows_48x64_420"), case("noise_16x16_444"), rst_case("optimize_48x64_420")]
    jp = [_put(directory, f"{i}_{c.name}.jpg", c.data) for i, c in enumerate(picks)]
    js, jl = [0, 0, 0, -1, 0, -2, 0], [c.luma for c in picks]
    jp.insert(5, os.path.join(directory, "missing.jpg")); js.insert(5, -1); jl.insert(5, None)
    for name, kw, options in (("jpeg_host", {}, {}), ("jpeg_device", {"entropy": "device"}, {"jpeg_entropy_memset": 0}),
                              ("jpeg_device_memset", {"entropy": "device"}, {"jpeg_entropy_memset": 1}),
                              ("jpeg_device_sync", {"entropy": "device", "sync": True}, {})):
        out[name] = FileList(name, "read_jpegs", "jpeg_chunk_frames", jp, js, jl, kw=kw, options=options)
    assert mrgingham_amd.jpeg_restart_intervals(picks[2].data)[0] == 0          # the file the sync decoder is for

    # PNG, 8 bit: every colour type the device takes, a palette file, one of another size, a truncated file
    w, h = 45, 37
    pp, ps, pl = [], [], []
    for k, ct in enumerate((0, 2, 4, 6)):
        img = png_cases.random_image(w, h, ct, 8, seed=30 + k)
        pp.append(os.path.join(directory, f"type{ct}_8.png"))
        png_cases.write(pp[-1], img, ct, 8, filters=("random", k), nidat=1 + k % 3)
        ps.append(0); pl.append(png_cases.grey_of(img, ct))
    pp.append(_put(directory, "truncated.png", open(pp[1], "rb").read()[:-40])); ps.append(-1); pl.append(None)
    pp.append(os.path.join(directory, "other_size.png"))
    png_cases.write(pp[-1], png_cases.random_image(w + 1, h, 0, 8), 0, 8); ps.append(-2); pl.append(None)
    pp.append(pp[0]); ps.append(0); pl.append(pl[0])
    out["png8"] = FileList("png8", "read_pngs", "png_chunk_frames", pp, ps, pl)
    # PNG, 16 bit
    pp, ps, pl = [], [], []
    for k, ct in enumerate((0, 2, 6)):
        img = png_cases.random_image(w, h, ct, 16, seed=40 + k)
        pp.append(os.path.join(directory, f"type{ct}_16.png"))
        png_cases.write(pp[-1], img, ct, 16, filters="rotate", nidat=2)
        ps.append(0); pl.append(png_cases.grey_of(img, ct))
    pp.insert(1, os.path.join(directory, "missing.png")); ps.insert(1, -1); pl.insert(1, None)
    out["png16"] = FileList("png16", "read_pngs", "png_chunk_frames", pp, ps, pl, bits=16)

    # PGM, 16 bit, 200 x 100: samples of every byte value, one short file, one 8-bit file
    rng = np.random.RandomState(7)
    gp, gs, gl = [], [], []
    for k in range(3):
        img = rng.randint(0, 65536, (100, 200)).astype(np.uint16)
        gp.append(os.path.join(directory, f"deep{k}.pgm"))
        files_cases.write_pgm(gp[-1], img, maxval=65535)
        gs.append(0); gl.append(img)
    gp.insert(1, _put(directory, "short16.pgm", open(gp[0], "rb").read()[:-1])); gs.insert(1, -1); gl.insert(1, None)
    gp.insert(3, os.path.join(directory, "flat.pgm"))
    files_cases.write_pgm(gp[3], rng.randint(0, 256, (100, 200)).astype(np.uint8)); gs.insert(3, -2); gl.insert(3, None)
    out["pgm16"] = FileList("pgm16", "read_pgms", "pgm_chunk_frames", gp, gs, gl, bits=16)

    # TIFF: LZW strips on the device, PackBits on the host threads inside the batch, a truncated file, a cut strip
    def tiff(name, img, **kw):
        path = os.path.join(directory, name + ".tif")
        tc.write(path, img, **kw)
        return path, tc.grey_of(img, kw.get("photometric", 2 if img.ndim == 3 and img.shape[2] >= 3 else 1))
    lzw = tiff("lzw", tc.random_image(w, h, 1, 8, seed=1), compression=tc.LZW, predictor=2, rows_per_strip=4)
    rgb = tiff("rgb", tc.random_image(w, h, 3, 8, seed=2), order=">", rows_per_strip=5, reverse=True)
    lzw2 = tiff("lzw2", tc.random_image(w, h, 1, 8, seed=9), compression=tc.LZW, rows_per_strip=6)
    packbits = tiff("packbits", tc.random_image(w, h, 1, 8, seed=4), compression=tc.PACKBITS, rows_per_strip=8)
    truncated = _put(directory, "truncated.tif", open(lzw[0], "rb").read()[:-30])
    img = tc.random_image(w, h, 1, 8, seed=8)
    strip = tc.lzw_encode(img.tobytes())
    broken = _put(directory, "broken_strip.tif", tc.encode(img, compression=tc.LZW, strip_bytes=[strip[:len(strip) // 2]])[0])
    files = [lzw, rgb, (truncated, None), lzw2, packbits, (broken, None), lzw]
    out["tiff_lzw"] = FileList("tiff_lzw", "read_tiffs", "tiff_chunk_frames", [p for p, _ in files], [0, 0, -1, 0, 0, -1, 0],
                               [s for _, s in files])
    dfl = tiff("deflate", ic.ramp_noise(h, w, seed=1), compression=tc.ADOBE_DEFLATE, predictor=2, rows_per_strip=4)
    dfl_be = tiff("deflate_be", ic.ramp_noise(h, w, seed=2), compression=tc.DEFLATE, order=">", rows_per_strip=5, reverse=True, odd=True)
    dfl3 = tiff("deflate3", ic.ramp_noise(h, w, seed=5), compression=tc.ADOBE_DEFLATE, rows_per_strip=7)
    img = ic.ramp_noise(h, w, seed=6)
    z = ic.deflate(img.tobytes())
    cut = _put(directory, "cut_strip.tif", tc.encode(img, compression=tc.ADOBE_DEFLATE, strip_bytes=[z[:len(z) // 2]])[0])
    files = [dfl, (cut, None), dfl_be, lzw, dfl3, (os.path.join(directory, "missing.tif"), None), dfl]
    out["tiff_deflate"] = FileList("tiff_deflate", "read_tiffs", "tiff_chunk_frames", [p for p, _ in files], [0, -1, 0, 0, 0, -1, 0],
                                   [s for _, s in files], kw={"deflate": "device"})

    # BMP, 65 x 7: every depth and both row orders, an RLE file (host threads inside the batch), a short file
    bw, bh = 65, 7
    pal256 = bc.random_palette(256, seed=1)

    def bmp(name, pixels, bits, palette=None, **kw):
        return _put(directory, name, bc.write(pixels, bits, palette, **kw)), bc.expected(pixels, bits, palette)
    rgbb = bmp("rgb.bmp", bc.random_pixels(bw, bh, 24, seed=7), 24)
    files = [bmp("grey8.bmp", bc.random_pixels(bw, bh, 8, seed=2), 8, bc.grey_ramp()),
             bmp("pal8.bmp", bc.random_pixels(bw, bh, 8, seed=4), 8, pal256, header=108), rgbb,
             (_put(directory, "short.bmp", open(rgbb[0], "rb").read()[:-1]), None),
             bmp("rgbx.bmp", bc.random_pixels(bw, bh, 32, seed=9), 32, bitfields=True),
             (_put(directory, "rle8.bmp", bc.write_rle8(bw, bh, bc.rle8_encode(bc.random_pixels(bw, bh, 8, seed=14, top=3)), pal256)), None),
             bmp("one.bmp", bc.random_pixels(bw, bh, 1, seed=10), 1, bc.random_palette(2, seed=11)),
             bmp("four_td.bmp", bc.random_pixels(bw, bh, 4, seed=12), 4, bc.random_palette(16, seed=13), top_down=True)]
    out["bmp"] = FileList("bmp", "read_bmps", "bmp_chunk_frames", [p for p, _ in files], [0, 0, 0, -1, 0, 0, 0, 0], [s for _, s in files])

    # Netpbm, 65 x 7: every 8-bit layout of tests/pnm_cases.py, a short file, a P6 file (not read)
    files = []
    for k, layout in enumerate(l for l in pc.LAYOUTS if l[2] != 16):
        data, want, _ = pc.write_layout(layout, bw, bh, seed=20 + k)
        files.append((_put(directory, layout[0] + ".pnm", data), want, 0))
    files.insert(2, (_put(directory, "short.pam", open(files[0][0], "rb").read()[:-1]), None, -1))
    files.insert(5, (_put(directory, "colour.ppm", pc.write(pc.random_samples(bw, bh, 8, 3, seed=41), 6, 8)), None, -1))
    out["pnm"] = FileList("pnm", "read_pnms", "pnm_chunk_frames", [p for p, _, _ in files], [s for _, _, s in files], [w_ for _, w_, _ in files])
    return out


def check_file_list(det, fl, chunk, what):
    """The loader over the list with chunks of `chunk` files (0: by the budget): statuses, the frames of the readable files
    against the arrays they were written from and against read_image, zero frames for the others."""
    import mrgingham_amd
    for name, value in fl.options.items():
        det.set_option(name, value)
    det.set_option(fl.chunk_option, chunk)
    try:
        frames, status = getattr(det, fl.method)(fl.paths, nthreads=2, **fl.kw)
    finally:
        det.set_option(fl.chunk_option, 0)
        for name in fl.options:
            det.set_option(name, 0)
    assert status.tolist() == fl.status, (what, fl.name, chunk, status.tolist())
    got = frames.cpu().numpy()
    assert got.dtype == (np.uint16 if fl.bits == 16 else np.uint8) and len(got) == len(fl.paths), (what, fl.name)
    for f, path in enumerate(fl.paths):
        if fl.status[f] != 0:
            assert not got[f].any(), (what, fl.name, chunk, path)
            continue
        host = mrgingham_amd.read_image(path)                    # (of 16-bit samples: the high bytes)
        assert host is not None and np.array_equal(got[f] >> 8 if fl.bits == 16 else got[f], host), (what, fl.name, chunk, path)
        if fl.source[f] is not None:
            assert np.array_equal(got[f], fl.source[f]), (what, fl.name, chunk, path)


def leftover_file_lists(directory):
    """A and B of every loader: A = the readable files of its list, each twice (full staging areas in both slots); B = the
    list itself cut to its first four files, the unreadable one among them where there is one."""
    out = {}
    for name, fl in file_lists(directory).items():
        good = [(p, s) for p, st, s in zip(fl.paths, fl.status, fl.source) if st == 0]
        a = [p for p, _ in good] * 2
        b = FileList.__new__(FileList)
        b.__dict__.update(fl.__dict__)
        k = max(4, fl.status.index(-1) + 1)
        b.paths, b.status, b.source = fl.paths[:k], fl.status[:k], fl.source[:k]
        out[name] = (fl, a, b)
    return out
