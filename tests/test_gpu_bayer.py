"""Bayer mosaics to grey frames on the device (Detector.bayer_grey, csrc/bayer_grey.hip over csrc/bayer_pixels.h).  The
yardstick is numpy (tests/bayer_cases.py), written from the definition and held against its known answers first.  The
definition is integer: np.array_equal everywhere, no tolerance.

Every call goes through _run: the mosaics sit in a flat device buffer at an offset, a frame pitch and a row stride of the
case's choosing (torch.as_strided views), the output likewise in a buffer filled with 0xA5, and both buffers come back
whole: the frames must equal the yardstick's, every other element of the output must still be 0xA5, and the input must
be unchanged.  The shapes sit where the kernel can go wrong: widths around one and two 16-byte words, odd heights with
more than one frame (a row parity that leaks across frames), offsets that put source and destination rows at every
phase of a 16-byte word, the seams of the schedule (mrgingham_amd.bayer_grey_geometry).  Nothing but the seam cases is
larger than 640 x 480."""
import numpy as np
import pytest

import mrgingham_amd
from mrgingham_amd import synth
from tests import bayer_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    bc.check_known()
    d = mrgingham_amd.Detector()
    yield d
    d.close()


def _dev(a):
    """a numpy array of uint8 or uint16 as a device tensor of the same type"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def _host(t):
    """a contiguous device tensor of uint8 or uint16 as a numpy array of the same type"""
    import torch
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _strided(flat, shape, off, pitch, stride):
    B, h, w = shape
    return np.lib.stride_tricks.as_strided(flat[off:], shape, (pitch * flat.itemsize, stride * flat.itemsize, flat.itemsize))


def _want(frames, pat):
    return np.stack([bc.grey(f, pat) for f in frames])


def _run(det, frames, pat, want=None, src=(0, None, None), dst=(0, None, None)):
    """frames [B,h,w] numpy; src, dst: (offset, frame pitch, row stride) in elements, None: dense.  Both buffers end with
    the last sample of the last frame."""
    import torch
    B, h, w = frames.shape
    dtype = frames.dtype
    fill = dtype.type(0xA5A5 & np.iinfo(dtype).max)
    want = _want(frames, pat) if want is None else want

    def layout(off, pitch, stride):
        stride = w if stride is None else stride
        pitch = h * stride if pitch is None else pitch
        return off, pitch, stride, off + (B - 1) * pitch + (h - 1) * stride + w
    so, sp, ss, sn = layout(*src)
    do, dp, ds, dn = layout(*dst)
    h_in = np.full(sn, fill, dtype)
    _strided(h_in, (B, h, w), so, sp, ss)[...] = frames
    d_in, d_out = _dev(h_in), _dev(np.full(dn, fill, dtype))
    got = det.bayer_grey(d_in.as_strided((B, h, w), (sp, ss, 1), so), pat, out=d_out.as_strided((B, h, w), (dp, ds, 1), do))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, h, w) and got.data_ptr() == d_out.data_ptr() + do * dtype.itemsize
    back = _host(d_out)
    expect = np.full(dn, fill, dtype)
    _strided(expect, (B, h, w), do, dp, ds)[...] = want
    if not np.array_equal(back, expect):
        bad = np.argwhere(_strided(back, (B, h, w), do, dp, ds) != want)
        assert False, (pat, str(dtype), (B, h, w), src, dst, "first wrong (frame, row, column):", bad[:4].tolist(), "of", len(bad),
                       "outside changed:", int((back != expect).sum()) - len(bad))
    assert np.array_equal(_host(d_in), h_in)


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("pat", bc.PATTERNS)
def test_grey_equals_numpy(det, pat, dtype):
    """every shape, three frames (an odd height with more than one frame: the row parity belongs to the frame), dense"""
    import torch
    assert any(h % 2 for h, w in bc.SHAPES)
    for k, (h, w) in enumerate(bc.SHAPES):
        frames = bc.random_frames(3, h, w, dtype, seed=1000 + k)
        _run(det, frames, pat)
    # and the call without `out`
    frames = bc.random_frames(3, 9, 17, dtype, seed=5)
    got = det.bayer_grey(_dev(frames), pat)
    torch.cuda.synchronize()
    assert got.is_contiguous() and np.array_equal(_host(got), _want(frames, pat))


@pytest.mark.parametrize("dtype", bc.DTYPES)
def test_seams_of_the_schedule(det, dtype):
    """a slab's last row, the first row of the next one, a third slab of one row; a row one word wider than a workgroup's
    span, whole and with a tail; more frames than the grid has planes"""
    lanes, rows, per_cu = mrgingham_amd.bayer_grey_geometry()
    assert per_cu == 0                                                # the grid is not capped: no second trip over the rows to test
    npx = 16 // np.dtype(dtype).itemsize                               # samples of a 16-byte word
    for i, h in enumerate((rows - 1, rows + 1, 2 * rows + 1)):
        _run(det, bc.random_frames(2, h, 19, dtype, seed=i), bc.PATTERNS[i])
        _run(det, bc.random_frames(2, h, 19, dtype, seed=i), bc.PATTERNS[i + 1], src=(1, None, 23), dst=(3, None, 32))
    for i, w in enumerate(((lanes + 1) * npx, (lanes + 1) * npx + 5)):
        _run(det, bc.random_frames(2, 3, w, dtype, seed=10 + i), bc.PATTERNS[2 + i])
        _run(det, bc.random_frames(2, 3, w, dtype, seed=10 + i), bc.PATTERNS[i], src=(3, None, w + 3), dst=(5, None, w + 16))
    # the frame loop: 65535 planes at the most, so 65537 frames (seven different ones, over and over) of 3 x 5
    few = bc.random_frames(7, 3, 5, dtype, seed=20)
    idx = np.arange(65537) % 7
    _run(det, few[idx], "grbg", want=_want(few, "grbg")[idx])


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("pat", bc.PATTERNS)
def test_views(det, pat, dtype):
    """input frames big[:, 1:1+h, 3:3+w] of a tensor with rows of odd length: an odd element offset, source rows at every
    phase of a 16-byte word; output a view inside a larger tensor, destination rows at every phase; both ending exactly
    where their tensors end.  Then rows 64 elements apart and every offset: the words of all rows aligned alike, the
    first whole word beginning at even and odd pixels."""
    for k, (h, w) in enumerate(((5, 3), (9, 17), (4, 33), (70, 33), (33, 130), (2, 300))):
        frames = bc.random_frames(3, h, w, dtype, seed=2000 + k)
        want = _want(frames, pat)
        stride = w + 7
        pitch = (h + 2) * stride
        _run(det, frames, pat, want, src=(stride + 3, pitch, stride), dst=(2 * (w + 5) + 1, (h + 3) * (w + 5), w + 5))
        _run(det, frames, pat, want, src=(stride + 3, pitch, stride))
        _run(det, frames, pat, want, dst=(1, h * (w + 2) + 1, w + 2))
    frames = bc.random_frames(2, 9, 37, dtype, seed=3000)
    want = _want(frames, pat)
    for off in range(16 // np.dtype(dtype).itemsize):
        _run(det, frames, pat, want, src=(off, 640, 64), dst=((5 * off + 3) % 16, 704, 64))
    _run(det, frames, pat, want, src=(0, 640, 64), dst=(0, 640, 64))


@pytest.mark.parametrize("dtype", bc.DTYPES)
def test_impulses_and_all_top(det, dtype):
    """the top value at every pixel of a 6 x 7 frame in turn and the complement, one batch per pattern; all samples at the
    top value give the top value"""
    frames = bc.impulse_frames(6, 7, dtype)
    top = np.iinfo(dtype).max
    for pat in bc.PATTERNS:
        _run(det, frames, pat)
        _run(det, frames, pat, src=(1, None, 9), dst=(3, None, 11))
        for h, w in ((2, 2), (5, 3), (9, 17), (4, 33)):
            full = np.full((2, h, w), top, dtype)
            _run(det, full, pat, want=full)


@pytest.mark.parametrize("dtype", bc.DTYPES)
def test_input_frames_may_repeat(det, dtype):
    """a frame pitch of 0 on the input (an expanded view): every output frame is the grey of the one mosaic"""
    import torch
    frame = bc.random_frames(1, 9, 17, dtype, seed=9)
    got = det.bayer_grey(_dev(frame).expand(3, 9, 17), "bggr")
    torch.cuda.synchronize()
    assert np.array_equal(_host(got), np.repeat(_want(frame, "bggr"), 3, axis=0))


@pytest.mark.parametrize("dtype", bc.DTYPES)
def test_bad_arguments_are_refused_and_write_nothing(det, dtype):
    import torch
    es = np.dtype(dtype).itemsize
    bits = 8 * es
    fill = dtype(0x5A5A & np.iinfo(dtype).max)
    B, h, w = 2, 5, 9
    frames = bc.random_frames(B, h, w + 3, dtype, seed=3)
    d_in = _dev(frames)
    n_out = (B * h) * (w + 2) + 16
    d_out = _dev(np.full(n_out, fill, dtype))
    in_pitch, in_stride, out_pitch, out_stride = h * (w + 3), w + 3, h * (w + 2), w + 2
    in_bytes = es * ((B - 1) * in_pitch + (h - 1) * in_stride + w)

    def call(ctx=-1, d_i=None, bits_=bits, n=B, width=w, height=h, ip=in_pitch, is_=in_stride, pattern=0, d_o=None, op=out_pitch, os_=out_stride):
        return det.L.mrgingham_amd_bayer_grey_batch(det.ctx if ctx == -1 else ctx, d_in.data_ptr() if d_i is None else d_i, bits_, n, width,
                                                    height, ip, is_, pattern, d_out.data_ptr() if d_o is None else d_o, op, os_, None)
    bad = [dict(pattern=4), dict(pattern=-1), dict(bits_=12), dict(bits_=0), dict(bits_=32), dict(width=1), dict(height=1),
           dict(width=32768, is_=32768, os_=32768), dict(height=32768), dict(width=0), dict(height=-1), dict(is_=w - 1), dict(os_=w - 1),
           dict(is_=0), dict(os_=-out_stride), dict(d_i=0), dict(d_o=0), dict(n=-1), dict(ip=-1), dict(op=-1), dict(ctx=None),
           dict(op=(h - 1) * out_stride + w - 1),                                                  # output frames that overlap each other
           dict(d_o=d_in.data_ptr()), dict(d_o=d_in.data_ptr() + in_bytes - es),                   # output begins inside the input
           dict(d_i=d_out.data_ptr() + es * 8), dict(d_o=d_in.data_ptr() - es * ((B - 1) * out_pitch + (h - 1) * out_stride + w) + es)]
    if es == 2:
        bad += [dict(d_i=d_in.data_ptr() + 1), dict(d_o=d_out.data_ptr() + 1)]                      # an odd uint16 address
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(d_o=d_in.data_ptr() + es) == -1 and b"overlap" in det.L.mrgingham_amd_last_error(det.ctx)
    assert call(n=0) == 0                                                 # nothing to do is not an error
    assert call(n=0, d_i=0, d_o=0) == 0
    torch.cuda.synchronize()
    assert (_host(d_out) == fill).all() and np.array_equal(_host(d_in), frames)
    assert call() == 0
    torch.cuda.synchronize()
    back = _host(d_out)
    want = _want(frames[:, :, :w], "rggb")
    assert np.array_equal(back[:B * h * (w + 2)].reshape(B, h, w + 2)[:, :, :w], want)
    assert (back[:B * h * (w + 2)].reshape(B, h, w + 2)[:, :, w:] == fill).all() and (back[B * h * (w + 2):] == fill).all()

    # the same through the Python method: each raises, and neither the frames nor `out` change
    keep = _dev(np.full((B, h, w), fill, dtype))
    view = d_in[:, :, :w]
    for kw in (dict(pattern="rgbg"), dict(pattern=0), dict(pattern=None), dict(out=keep[:1]), dict(out=keep[:, :, :w - 1]),
               dict(out=keep.view(torch.int16 if es == 2 else torch.int8)), dict(out=keep.cpu()), dict(out=_dev(np.zeros((B, h, 2 * w), dtype))[:, :, ::2]),
               dict(out=keep[:1].expand(B, h, w))):
        args = dict(pattern="rggb", out=keep)
        args.update(kw)
        with pytest.raises(ValueError):
            det.bayer_grey(view, **args)
    for frames_bad in (view.cpu(), view[0], view[:, :1], view[:, :, :1], d_in[:, :, ::2], view.view(torch.int16 if es == 2 else torch.int8),
                       frames.astype(np.float32)):
        with pytest.raises(ValueError):
            det.bayer_grey(frames_bad, "rggb")
    with pytest.raises(RuntimeError, match="overlap"):                    # `out` inside the tensor of the frames, either order
        det.bayer_grey(d_in[:, :h - 1, :w], "rggb", out=d_in[:, 1:, :w])
    with pytest.raises(RuntimeError, match="overlap"):
        det.bayer_grey(d_in[:, 1:, :w], "rggb", out=d_in[:, :h - 1, :w])
    torch.cuda.synchronize()
    assert (_host(keep) == fill).all() and np.array_equal(_host(d_in), frames)
    assert tuple(det.bayer_grey(view[:0], "rggb").shape) == (0, h, w)


def _check_boards(boards, lattices, what):
    worst = 0.0
    for f, lattice in enumerate(lattices):
        lat = lattice.reshape(-1, 2)
        d = np.hypot(boards[f][:, None, 0] - lat[None, :, 0], boards[f][:, None, 1] - lat[None, :, 1]).min(axis=1)
        worst = max(worst, float(d.max()))
    print(f"{what}: worst corner {worst:.3f} px from its lattice point")
    assert worst <= 0.4, (what, worst)


def test_tinted_boards_to_boards(det):
    """boards tinted R : G : B = 1 : 3/4 : 1/2 behind each of the four filters, four frames: find_boards(bayer_grey(..)) at
    level 0 finds all four, equal double for double to the boards from the yardstick's grey uploaded, every corner within
    0.4 px of its lattice point.  Once at 16 bit through preprocess (the yardstick's route gives 0.242 px)."""
    W, H = 640, 480
    lattices = [synth.board_lattice(W, H, 10, seed) for seed in range(4)]
    for pat in bc.PATTERNS:
        m = np.stack([bc.tinted_board(seed, pat) for seed in range(4)])
        want_boards, want_found = det.find_boards(_dev(_want(m, pat)), gridn=10, image_pyramid_level=0)
        boards, found = det.find_boards(det.bayer_grey(_dev(m), pat), gridn=10, image_pyramid_level=0)
        assert (np.asarray(found) >= 0).all() and np.array_equal(found, want_found), pat
        assert np.array_equal(boards, want_boards), pat
        _check_boards(boards, lattices, pat)
    m = np.stack([bc.tinted_board(seed, "rggb", bits=16) for seed in range(4)])
    assert m.dtype == np.uint16 and m.max() > 2048
    want_boards, want_found = det.find_boards(det.preprocess(_dev(_want(m, "rggb"))), gridn=10, image_pyramid_level=0)
    boards, found = det.find_boards(det.preprocess(det.bayer_grey(_dev(m), "rggb")), gridn=10, image_pyramid_level=0)
    assert (np.asarray(found) >= 0).all() and np.array_equal(found, want_found)
    assert np.array_equal(boards, want_boards)
    _check_boards(boards, lattices, "rggb, 16 bit")
