"""The command-line tool's 16-bit branch (mrgingham-from-image.cc:85-92, then the box blur of :106-111) for a batch of
frames on the device (mrgingham_amd_preprocess16_batch, Detector.preprocess on uint16): bit-exact against
oracle_preprocess16 frame by frame, against the one-image kernels (option "preprocess_fused" 0) and the host entry point,
and end to end against process_image_ex(bits=16)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ("board12", "eight", "narrow", "full", "flat", "bigbin")


def _frame16(kind, H, W, rng, i):
    """One uint16 [H,W] frame; `i` moves its value range, so that no two frames of a batch share one."""
    from mrgingham_amd import synth
    if kind == "board12":   # a 12-bit sensor: R ~ 4 K, somewhere in the 16-bit range
        b = synth.board_frame(W, H, gridn=10, seed=i).numpy() if min(W, H) >= 64 else rng.randint(0, 256, (H, W))
        return (b.astype(np.int64) * 16 + 977 * i + rng.randint(0, 3000)).astype(np.uint16)
    if kind == "eight":     # 8-bit values on the 16-bit scale
        return (rng.randint(0, 256, (H, W)) * 257 // (1 + i % 3)).astype(np.uint16)
    if kind == "narrow":    # R ~ 100
        base = rng.randint(0, 65000)
        return rng.randint(base, base + 100 + i, (H, W)).astype(np.uint16)
    if kind == "full":      # 0 .. 65535: the global-memory histogram path
        f = rng.randint(0, 65536, (H, W))
        f.flat[0], f.flat[-1] = 0, 65535
        return f.astype(np.uint16)
    if kind == "flat":      # smax == smin
        return np.full((H, W), 1000 + 7 * i, np.uint16)
    # bigbin: one value in nearly every pixel -- a bin of a large tile passes 65 535 -- and a few others
    f = np.full((H, W), 30000 + i, np.int64)
    f[::7, ::5] = rng.randint(20000, 40000, f[::7, ::5].shape)
    return f.astype(np.uint16)


def _batch(kinds, H, W, seed):
    rng = np.random.RandomState(seed)
    return np.stack([_frame16(k, H, W, rng, i) for i, k in enumerate(kinds)])


def _dev(a):
    """numpy uint16 -> device torch.uint16 (through int16: the copy does not depend on uint16 support)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def _want(frames, clahe, blurs):
    """oracle_preprocess16 for every frame and blur radius (the expensive part, CLAHE, once per frame)."""
    from oracle import oracle
    out = {b: [] for b in blurs}
    for f in frames:
        base = oracle.preprocess16(f, clahe=clahe, blur_radius=0)
        for b in blurs:
            out[b].append(base if b == 0 else oracle.box_blur(base, b))
    return out


@pytest.mark.parametrize("W,H,kinds", [
    (8, 8, KINDS),
    (601, 333, KINDS),                 # ragged on both axes: both padded, reflect-101 samples in the histograms
    (1000, 17, KINDS),
    (1920, 1080, ("board12", "full", "bigbin", "narrow")),
    (4096, 3072, ("bigbin", "board12")),   # tiles of 196 608 pixels: one bin holds more than 65 535 of them
])
def test_batch_matches_the_oracle(W, H, kinds):
    import torch
    import mrgingham_amd
    frames = _batch(kinds, H, W, seed=W + H)
    # (the oracle's own blur of its 8-bit image: equal to oracle.preprocess16(.., blur_radius=b), which it is built of)
    f0 = frames[0]
    from oracle import oracle
    assert np.array_equal(oracle.preprocess16(f0, clahe=True, blur_radius=1),
                          oracle.box_blur(oracle.preprocess16(f0, clahe=True, blur_radius=0), 1))
    det = mrgingham_amd.Detector(0)
    d = _dev(frames)
    for clahe, blurs in [(True, (1, 0, 2)), (False, (1, 0))]:
        want = _want(frames, clahe, blurs)
        for blur in blurs:
            got = det.preprocess(d, clahe=clahe, blur_radius=blur)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            assert got.dtype == np.uint8 and got.shape == frames.shape
            for i in range(len(frames)):
                w = want[blur][i]
                assert np.array_equal(got[i], w), (W, H, kinds[i], clahe, blur, int(np.abs(got[i].astype(int) - w).max()),
                                                   int((got[i] != w).sum()))
    det.close()


def test_strided_batch_equals_the_contiguous_one():
    import torch
    import mrgingham_amd
    H, W = 333, 601
    frames = _batch(("board12", "full", "narrow", "bigbin"), H, W, seed=3)
    wide = np.zeros((4, H + 3, W + 40), np.uint16)
    wide[:, :H, :W] = frames
    view = _dev(wide)[:, :H, :W]           # row stride W + 40, frame pitch (H + 3) (W + 40) > H * stride
    assert view.stride(1) == W + 40 and view.stride(0) > H * view.stride(1)
    dense = _dev(frames)
    det = mrgingham_amd.Detector(0)
    for clahe, blur in [(True, 1), (True, 0), (True, 3), (False, 1), (False, 0)]:
        a = det.preprocess(view, clahe=clahe, blur_radius=blur)
        b = det.preprocess(dense, clahe=clahe, blur_radius=blur)
        torch.cuda.synchronize()
        assert torch.equal(a, b), (clahe, blur)
    det.close()


@pytest.mark.parametrize("kind", ["board12", "full"])
def test_three_passes_equal_the_one_image_kernels_and_the_host_call(kind):
    """16 frames of 4096x3072: the new path against option preprocess_fused 0 (normalised copy, 65 536-bin tables,
    separate blur) and against the host entry point per frame."""
    import torch
    import mrgingham_amd
    H, W = 3072, 4096
    frames = _batch((kind,) * 16, H, W, seed=11)
    d = _dev(frames)
    det = mrgingham_amd.Detector(0)
    for clahe, blur in [(True, 1), (True, 0), (False, 1)]:
        one = det.preprocess(d, clahe=clahe, blur_radius=blur)
        det.set_option("preprocess_fused", 0)
        two = det.preprocess(d, clahe=clahe, blur_radius=blur)
        det.set_option("preprocess_fused", 1)
        torch.cuda.synchronize()
        assert torch.equal(one, two), (kind, clahe, blur, int((one != two).sum()))
    host = one.cpu().numpy()
    for i in range(0, 16, 5):
        assert np.array_equal(mrgingham_amd.api.preprocess16(frames[i], clahe=False, blur_radius=1), host[i]), i
    full = det.preprocess(d, clahe=True, blur_radius=1).cpu().numpy()
    for i in range(0, 16, 5):
        assert np.array_equal(mrgingham_amd.api.preprocess16(frames[i], clahe=True, blur_radius=1), full[i]), i
    det.close()


class _CliOptions(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("do_clahe", "blur_radius", "gridn", "image_pyramid_level", "do_refine",
                                            "do_blobs", "debug", "debug_sequence_x", "debug_sequence_y")] + \
               [("filename", ctypes.c_char_p)]


def test_preprocessed_16_bit_frames_give_the_boards_of_the_tool():
    """16-bit board frames -> Detector.preprocess -> Detector.find_boards, against process_image_ex(bits=16) with the
    same options (what the command-line tool does per image)."""
    import torch
    import mrgingham_amd
    from mrgingham_amd import _lib
    from mrgingham_amd import synth
    H, W = 960, 1280
    frames = np.stack([(synth.board_frame(W, H, gridn=10, seed=s).numpy().astype(np.int64) * 12 + 500 * s + 3000)
                       .astype(np.uint16) for s in range(3)])
    det = mrgingham_amd.Detector(0)
    pre = det.preprocess(_dev(frames), clahe=True, blur_radius=1)
    boards, found = det.find_boards(pre, gridn=10)
    L = _lib.lib()
    L.mrgingham_amd_process_image_ex.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(_CliOptions), ctypes.c_void_p, ctypes.c_void_p]
    opt = _CliOptions(1, 1, 10, -1, 1, 0, 0, -1, -1, None)
    for i in range(len(frames)):
        xy = np.zeros((100, 2), np.float64)
        lv = L.mrgingham_amd_process_image_ex(np.ascontiguousarray(frames[i]).ctypes.data, 16, W, H, W, ctypes.byref(opt),
                                              xy.ctypes.data, None)
        assert lv >= 0 and found[i] == lv, (i, lv, found[i])
        assert np.abs(np.asarray(boards[i]) - xy).max() < 1e-6, i
    det.close()


def test_argument_errors_write_nothing():
    import torch
    import mrgingham_amd
    det = mrgingham_amd.Detector(0)
    L, ERR_ARG = det.L, -1
    H, W = 32, 48
    d = _dev(_batch(("board12", "full"), H, W, seed=1))
    out = torch.full((2, H, W), 77, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    f = L.mrgingham_amd_preprocess16_batch
    p, o = d.data_ptr(), out.data_ptr()
    cases = [
        (None, H * W, 2, W, H, W, 1, 1, o),      # NULL frames
        (p, H * W, 2, W, H, W, 1, -1, o),        # bad radius
        (p, H * W, 2, W, H, W, 1, 65, o),
        (p, H * W, 2, W, H, W - 1, 1, 1, o),     # stride < width
        (p, H * W, 2, W, H, W, 1, 1, None),      # NULL output
        (p, H * W, -1, W, H, W, 1, 1, o),        # negative frame count
        (p, H * W, 2, 7, H, W, 1, 1, o),         # CLAHE on a side below 8
        (p, H * W, 2, W, 7, W, 1, 1, o),
    ]
    for c in cases:
        assert f(det.ctx, *c, s) == ERR_ARG, c
    assert f(None, p, H * W, 2, W, H, W, 1, 1, o, s) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    with pytest.raises(AssertionError):
        det.preprocess(d.view(torch.int16))     # other dtypes keep failing as before
    det.close()
