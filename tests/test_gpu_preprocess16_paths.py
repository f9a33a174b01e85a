"""The 16-bit batch path (csrc/preprocess16_batch.hip, Detector.preprocess on uint16) against oracle_preprocess16 where its
kernels change behaviour: the histogram classes at their range edges (R = smax - smin + 1: LDS slabs of 16-bit counters
up to 4 096, parts of 16 384 bins above), the slab size of the small class, the 16-byte and element loads, and the
seams between the chunks of frames a batch is processed in -- with option "preprocess_fused" 1 and 0 (the one-image
kernels, chunked the same way)."""
import concurrent.futures

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RANGES = (1, 2, 4095, 4096, 4097, 16384, 16385, 16386, 32768, 32769, 49152, 49153, 65535, 65536)
CHUNK = 42   # frames per chunk today: kPreprocess16TableBudget / (64 tiles x 65 536 entries x 6 B); the tests do not rely on it


def _dev(a):
    """numpy uint16 -> device torch.uint16 (through int16: the copy does not depend on uint16 support)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def _range_frame(H, W, smin, R, rng):
    """Values in [smin, smin + R - 1], both ends present: the minimum in the last column, the maximum as ONE pixel in the
    last row (another tile), so the top part of a parts-class frame holds a single bin of a single pixel; a flat block
    gives some tiles a bin that is clipped."""
    smax = smin + R - 1
    f = rng.randint(smin, smax, (H, W)) if R > 1 else np.full((H, W), smin, np.int64)
    f[H // 4:H // 2, W // 3:W // 2] = rng.randint(smin, smax) if R > 1 else smin
    f[(5 * H) // 16, W - 1] = smin
    f[H - 1, (3 * W) // 16] = smax
    return f.astype(np.uint16)


def _range_cases():
    """(smin, R) for every range edge, the minimum at 0, at a small offset and at the top of the 16-bit scale."""
    out = []
    for R in RANGES:
        for smin in dict.fromkeys((0, min(37, 65536 - R), 65536 - R)):
            out.append((smin, R))
    return out


def _oracle16(frames, clahe, blurs):
    """oracle_preprocess16 of every frame (once) and its blurs, on at most 8 threads (ctypes releases the GIL)."""
    from oracle import oracle
    oracle.lib()
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        base = list(pool.map(lambda f: oracle.preprocess16(f, clahe=clahe, blur_radius=0), frames))
        out = {b: (base if b == 0 else list(pool.map(lambda x: oracle.box_blur(x, b), base))) for b in blurs}
    return out


def _check(got, want, what):
    for i in range(len(want)):
        if not np.array_equal(got[i], want[i]):
            d = np.argwhere(got[i] != want[i])
            y, x = d[0]
            pytest.fail(f"{what} frame {i}: {len(d)} pixels differ, first at (x {x}, y {y}) {got[i][y, x]} != "
                        f"{want[i][y, x]}, max |diff| {int(np.abs(got[i].astype(int) - want[i]).max())}")


def _run(det, dev, clahe, blur, fused):
    import torch
    det.set_option("preprocess_fused", fused)
    got = det.preprocess(dev, clahe=clahe, blur_radius=blur)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("W,H", [
    (1024, 768),    # tiles 128 x 96: 16-byte loads in every kernel
    (1000, 1000),   # tiles 125 wide: 16-byte loads in the extrema pass, element loads in the histograms
    (601, 333),     # ragged: both sides padded, reflected samples
])
def test_range_classes_at_their_edges(W, H):
    """Every range edge of the histogram classes, with the extrema placed apart, as one mixed batch and each frame alone."""
    import mrgingham_amd
    cases = _range_cases()
    rng = np.random.RandomState(W + H)
    frames = np.stack([_range_frame(H, W, smin, R, rng) for smin, R in cases])
    for i, (smin, R) in enumerate(cases):
        assert int(frames[i].min()) == smin and int(frames[i].max()) == smin + R - 1
        assert R == 1 or int((frames[i] == smin + R - 1).sum()) == 1
    want = {True: _oracle16(frames, True, (0, 1)), False: _oracle16(frames, False, (1,))}
    det = mrgingham_amd.Detector(0)
    dev = _dev(frames)
    for clahe, blur in [(True, 1), (True, 0), (False, 1)]:
        for fused in (1, 0):
            w = want[clahe][blur]
            _check(_run(det, dev, clahe, blur, fused), w, f"{W}x{H} batch clahe {clahe} blur {blur} fused {fused}")
            if clahe:
                for i, (smin, R) in enumerate(cases):
                    _check(_run(det, dev[i:i + 1], clahe, blur, fused), w[i:i + 1],
                           f"{W}x{H} alone smin {smin} R {R} blur {blur} fused {fused}")
    det.close()


@pytest.mark.parametrize("W,H", [
    (2040, 2056),   # tiles of 255 x 257 = 65 535 pixels: one slab of the most pixels a slab may hold
    (2048, 2048),   # 65 536 pixels: two slabs
    (2048, 2056),   # 65 792
])
def test_small_class_slab_edges(W, H):
    """One value in nearly every pixel of a frame of the small range class."""
    import mrgingham_amd
    rng = np.random.RandomState(W * 3 + H)
    frames = []
    for v, spread in [(30000, 2000), (123, 100), (65000, 535)]:   # R <= 4 001
        f = np.full((H, W), v, np.int64)
        f[::97, ::89] = rng.randint(v - min(v, spread), v + spread + 1, f[::97, ::89].shape)
        frames.append(np.clip(f, 0, 65535).astype(np.uint16))
    frames = np.stack(frames)
    assert all(int(f.max()) - int(f.min()) + 1 <= 4096 for f in frames)
    want = _oracle16(frames, True, (0, 1))
    det = mrgingham_amd.Detector(0)
    dev = _dev(frames)
    for blur in (1, 0):
        for fused in (1, 0):
            _check(_run(det, dev, True, blur, fused), want[blur], f"{W}x{H} blur {blur} fused {fused}")
    det.close()


@pytest.mark.parametrize("layout", ["offset", "odd-stride"])
def test_unaligned_frames(layout):
    """A view one element into its rows (base not 16-byte aligned) and rows of W + 1 elements: element loads everywhere."""
    import mrgingham_amd
    W, H = 1024, 768
    cases = [(0, 65536), (37, 4096), (1000, 16385), (65536 - 4097, 4097), (9, 2)]
    rng = np.random.RandomState(5)
    frames = np.stack([_range_frame(H, W, smin, R, rng) for smin, R in cases])
    if layout == "offset":
        buf = np.zeros((len(cases), H, W + 8), np.uint16)
        buf[:, :, 1:W + 1] = frames
        dev = _dev(buf)[:, :, 1:W + 1]
        assert dev.data_ptr() % 16 == 2
    else:
        buf = np.zeros((len(cases), H, W + 1), np.uint16)
        buf[:, :, :W] = frames
        dev = _dev(buf)[:, :, :W]
        assert dev.stride(1) == W + 1
    want = {True: _oracle16(frames, True, (0, 1, 2)), False: _oracle16(frames, False, (1,))}
    det = mrgingham_amd.Detector(0)
    for clahe, blur in [(True, 1), (True, 0), (True, 2), (False, 1)]:
        for fused in (1, 0):
            _check(_run(det, dev, clahe, blur, fused), want[clahe][blur], f"{layout} clahe {clahe} blur {blur} fused {fused}")
    det.close()


# the range of frame i of the seam batch: class (i + i // CHUNK) % 3 -- narrow, middle, wide -- so that the frames on
# either side of a seam differ in class and each scratch slot moves from wide to narrow, narrow to middle, middle to wide
# from one chunk to the next
_SEAM_RANGES = ((1, 2, 100, 4095, 4096), (4097, 16385, 16386, 20000, 32768), (32769, 49153, 60000, 65535, 65536))


def _seam_batch(H, W, n, seed):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        cls = _SEAM_RANGES[(i + i // CHUNK) % 3]
        R = cls[(i // 3) % len(cls)]
        smin = rng.randint(0, 65536 - R + 1)
        out.append(_range_frame(H, W, smin, R, rng))
    return np.stack(out)


@pytest.mark.parametrize("W,H", [(64, 48), (61, 45)])
def test_chunk_seams(W, H):
    """100 frames: two chunk seams today and at least one for any chunk below 100 frames; every frame is different, so a
    chunk that reads or writes another chunk's frames shows."""
    import mrgingham_amd
    frames = _seam_batch(H, W, 100, seed=W * H)
    assert len({f.tobytes() for f in frames}) == len(frames)
    want = {True: _oracle16(frames, True, (0, 1, 2)), False: _oracle16(frames, False, (0, 1, 2))}
    det = mrgingham_amd.Detector(0)
    dev = _dev(frames)
    for clahe in (True, False):
        for blur in (0, 1, 2):
            for fused in (1, 0):
                _check(_run(det, dev, clahe, blur, fused), want[clahe][blur], f"{W}x{H} clahe {clahe} blur {blur} fused {fused}")
    det.close()
