"""Every path of launch_clahe (csrc/preprocess.hip) against the oracle (oracle_preprocess) at full frame sizes: the fused
blend + blur kernel at each of its row counts, the fast blend, the plain blend and the blur alone, on frames padded and
not, aligned and not, through mrgingham_amd_preprocess_batch (Detector.preprocess) with option "preprocess_fused" 1 and 0.
The paths share the histogram and LUT kernels, so comparing them with each other cannot catch a bug in those."""
import concurrent.futures
import functools

import numpy as np
import pytest

PATHS = ("fused32", "fused16", "fused8", "fast", "plain", "blur-only")


def path_of(W, H, aligned, clahe, blur, fused_option):
    """The kernel that blends a W x H frame in Detector.preprocess: the rules of mrgingham_amd_preprocess_batch (api.hip)
    and, in preprocess.hip, clahe_geom, fused_rows (through clahe_blur3_fused) and the `fast` condition of launch_clahe.
    `aligned`: the frames' base address, row stride and frame pitch are multiples of 16 bytes."""
    if not clahe:
        return "blur-only"
    ew, eh = W, H
    if W % 8 or H % 8:                      # OpenCV pads both sides as soon as one of them is ragged
        ew, eh = W + 8 - W % 8, H + 8 - H % 8
    tw, th = ew // 8, eh // 8
    if blur == 1 and fused_option and aligned and W % 16 == 0 and W >= 32 and H >= 2:
        for rows in (32, 16, 8):
            if 4 * rows + 2 <= th:
                return f"fused{rows}"
    if tw >= 256 and th >= 128 and W % 16 == 0 and aligned:
        return "fast"
    return "plain"


# (W, H, how the frames sit in memory): "dense", "strided" (rows of W + 16 bytes) or "offset" (a view 1 byte into such rows)
GEOMETRIES = [
    (4096, 3072, "dense"),      # the bench shape: fused32 (four 1024-column workgroups), fast without it
    (4095, 3071, "dense"),      # both sides ragged and padded, not a multiple of 16: plain
    (4096, 2160, "strided"),
    (2048, 1536, "dense"),
    (2048, 1024, "dense"),      # tile height 128: the lower edge of the fast blend; fused16
    (2064, 1039, "strided"),    # padded: tiles 259 x 130, the lower edge of fused32; fast
    (2064, 272, "dense"),       # tile height 34, the lower edge of fused8; cells 258 px wide: the second workgroup stages ncx_max = 5
    (2064, 271, "dense"),       # padded on both axes: tiles 259 x 34, fused8, the second workgroup again at ncx_max
    (1040, 520, "dense"),       # tile height 65: fused8; a 16-column second workgroup
    (1040, 528, "dense"),       # 66: fused16
    (1040, 527, "strided"),     # padded to 66: fused16
    (1040, 1032, "dense"),      # 129: fused16
    (1040, 1040, "dense"),      # 130: fused32
    (2048, 1536, "offset"),     # the same size 1 byte into an aligned buffer: plain
]
SETTINGS = [(clahe, blur, fused) for clahe in (True, False) for blur in (1, 0, 2, 3) for fused in (1, 0)]
KINDS = ("board", "noise", "tiles", "two", "ramp", "flat")


def _aligned(layout):
    return layout != "offset"


def _padded(W, H):
    return W % 8 != 0 or H % 8 != 0


CASES = [(W, H, layout, clahe, blur, fused) for W, H, layout in GEOMETRIES for clahe, blur, fused in SETTINGS]


def _case_id(c):
    W, H, layout, clahe, blur, fused = c
    return f"{W}x{H}-{layout}-{'clahe' if clahe else 'raw'}-b{blur}-f{fused}-{path_of(W, H, _aligned(layout), clahe, blur, fused)}"


def test_the_case_table_reaches_every_path():
    """Each path is met by a frame that is padded and by one that is not, so a change of the selection rules that
    leaves one of them untested shows up here."""
    seen = {(path_of(W, H, _aligned(lay), c, b, f), _padded(W, H)) for W, H, lay, c, b, f in CASES}
    missing = [(p, pad) for p in PATHS for pad in (False, True) if (p, pad) not in seen]
    assert not missing, missing
    # the edges named in the table
    assert path_of(2048, 1024, True, True, 0, 1) == "fast" and path_of(2048, 1016, True, True, 0, 1) == "plain"
    assert path_of(2064, 272, True, True, 1, 1) == "fused8" and path_of(2064, 264, True, True, 1, 1) == "plain"
    assert path_of(1040, 520, True, True, 1, 1) == "fused8" and path_of(1040, 528, True, True, 1, 1) == "fused16"
    assert path_of(1040, 1032, True, True, 1, 1) == "fused16" and path_of(1040, 1040, True, True, 1, 1) == "fused32"
    assert path_of(2048, 1536, False, True, 1, 1) == "plain" and path_of(2048, 1536, True, True, 1, 0) == "fast"


def _frame(kind, H, W, rng):
    """One uint8 frame; every call draws its own value range."""
    x = np.arange(W)[None, :]
    y = np.arange(H)[:, None]
    if kind == "board":         # a board at reduced range with an offset
        from mrgingham_amd import synth
        f = synth.board_frame(W, H, gridn=10, seed=int(rng.randint(1000)), device="cuda").cpu().numpy().astype(np.float32)
        f = f * rng.uniform(0.3, 0.7) + rng.uniform(5, 60)
    elif kind == "noise":       # noise over a random range
        lo = rng.randint(0, 100)
        f = lo + rng.rand(H, W).astype(np.float32) * rng.uniform(20, 255 - lo)
    elif kind == "tiles":       # whole flat tiles plus sparse outliers: nearly all of a tile clipped off and redistributed
        levels = rng.randint(40, 200, (8, 8)).astype(np.float32)
        f = levels[np.minimum(y * 8 // H, 7), np.minimum(x * 8 // W, 7)]
        f = np.broadcast_to(f, (H, W)).copy()
        m = rng.rand(H, W) < 0.003
        f[m] = rng.randint(0, 256, int(m.sum()))
    elif kind == "two":         # two values
        a, b = sorted(rng.choice(256, 2, replace=False))
        f = np.where(((x // 37) + (y // 23)) % 2 == 0, a, b).astype(np.float32)
    elif kind == "ramp":        # a horizontal ramp: every bin occupied
        f = np.broadcast_to((x * 256 // W).astype(np.float32), (H, W))
    else:                       # constant
        f = np.full((H, W), float(rng.randint(256)), np.float32)
    return np.clip(f, 0, 255).astype(np.uint8)


def _oracle_map(fn, items):
    """fn over items on at most 8 threads (the oracle's ctypes calls release the GIL)."""
    from oracle import oracle
    oracle.lib()
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(fn, items))


def _device_frames(frames, layout):
    import torch
    B, H, W = frames.shape
    if layout == "dense":
        return torch.from_numpy(frames).cuda()
    buf = torch.zeros((B, H, W + 16), dtype=torch.uint8, device="cuda")
    x0 = 1 if layout == "offset" else 0
    view = buf[:, :, x0:x0 + W]
    view.copy_(torch.from_numpy(frames).cuda())
    assert (view.data_ptr() % 16 == 0) == (layout != "offset") and view.stride(1) == W + 16
    return view


@functools.lru_cache(maxsize=1)
def _geometry(W, H, layout):
    """The frames of a geometry, on the host and on the device, and what the oracle makes of them for every setting
    (CLAHE once per frame; the blurs of its result with oracle_box_blur, which oracle_preprocess is built of)."""
    from oracle import oracle
    rng = np.random.RandomState(W * 7 + H)
    frames = np.stack([_frame(k, H, W, rng) for k in KINDS])
    base = _oracle_map(lambda f: oracle.preprocess(f, clahe=True, blur_radius=0), frames)
    want = {}
    for b in (0, 1, 2, 3):
        want[(True, b)] = base if b == 0 else _oracle_map(lambda f: oracle.box_blur(f, b), base)
        want[(False, b)] = _oracle_map(lambda f: oracle.preprocess(f, clahe=False, blur_radius=b), frames)
    assert np.array_equal(want[(True, 1)][0], oracle.preprocess(frames[0], clahe=True, blur_radius=1))
    assert np.array_equal(want[(True, 3)][1], oracle.preprocess(frames[1], clahe=True, blur_radius=3))
    return frames, _device_frames(frames, layout), want


def _check_frames(got, want, what):
    for i in range(len(want)):
        if not np.array_equal(got[i], want[i]):
            d = np.argwhere(got[i] != want[i])
            y, x = d[0]
            pytest.fail(f"{what} frame {i} ({KINDS[i] if len(want) == len(KINDS) else i}): {len(d)} pixels differ, "
                        f"first at (x {x}, y {y}) {got[i][y, x]} != {want[i][y, x]}, max |diff| "
                        f"{int(np.abs(got[i].astype(int) - want[i]).max())}")


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,layout,clahe,blur,fused", CASES, ids=[_case_id(c) for c in CASES])
def test_every_path_matches_the_oracle(W, H, layout, clahe, blur, fused):
    import torch
    import mrgingham_amd
    frames, dev, want = _geometry(W, H, layout)
    det = mrgingham_amd.Detector(0)
    det.set_option("preprocess_fused", fused)
    got = det.preprocess(dev, clahe=clahe, blur_radius=blur)
    torch.cuda.synchronize()
    _check_frames(got.cpu().numpy(), want[(clahe, blur)], _case_id((W, H, layout, clahe, blur, fused)))
    det.close()


@pytest.mark.gpu
def test_a_bench_shape_batch_matches_the_oracle():
    """16 distinct frames of 4096x3072 in rows of 4112 bytes, the tool's default chain (CLAHE, blur 1: fused32), frame by
    frame against the oracle; one of them through the host entry point too."""
    import torch
    import mrgingham_amd
    from oracle import oracle
    W, H = 4096, 3072
    assert path_of(W, H, True, True, 1, 1) == "fused32"
    rng = np.random.RandomState(16)
    frames = np.stack([_frame(KINDS[i % len(KINDS)], H, W, rng) for i in range(16)])
    want = _oracle_map(lambda f: oracle.preprocess(f, clahe=True, blur_radius=1), frames)
    dev = _device_frames(frames, "strided")
    det = mrgingham_amd.Detector(0)
    got = det.preprocess(dev, clahe=True, blur_radius=1)
    torch.cuda.synchronize()
    _check_frames(got.cpu().numpy(), want, "4096x3072 batch of 16")
    det.close()
    assert np.array_equal(mrgingham_amd.preprocess(frames[2], clahe=True, blur_radius=1), want[2])
