"""Colour frames to grey frames on the device (Detector.colour_grey, csrc/colour_grey.hip over csrc/colour_pixels.h).  The
yardstick is numpy (tests/colour_cases.py), written from the definition and held against its known answers first.  The
definition is integer: np.array_equal everywhere, no tolerance.

Every call goes through _run: the frames sit in a flat device buffer at an offset, a frame pitch, a row stride and (planar)
a plane pitch of the case's choosing (torch.as_strided views), the output likewise in a buffer filled with 0xA5; both
buffers END with the last sample, and both come back whole: the frames must equal the yardstick's, every other element of
the output must still be 0xA5, and the input must be unchanged.  The shapes sit where the kernel can go wrong: widths
around one and two 16-byte destination words, heights 1 and odd, offsets that put source and destination rows at every
phase of a 16-byte word, the seams of the row schedule (mrgingham_amd.colour_grey_geometry).  Nothing but the seam and
far-view cases is larger than 640 x 480."""
import numpy as np
import pytest

import mrgingham_amd
from tests import colour_cases as cc
from tests import far_views as fv

pytestmark = pytest.mark.gpu

CASES = cc.cases()
CASE_IDS = [f"{fmt}-{np.dtype(dtype).name}" for fmt, dtype in CASES]


@pytest.fixture(scope="module")
def det():
    cc.check_known()
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
    """a device tensor of uint8 or uint16 as a numpy array of the same type"""
    import torch
    t = t.contiguous()
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _strided(flat, shape, off, strides):
    return np.lib.stride_tricks.as_strided(flat[off:], shape, tuple(s * flat.itemsize for s in strides))


def _src_layout(fmt, B, h, w, off=0, pitch=None, stride=None, plane=None):
    """-> (view shape, element strides, offset, elements of the buffer: it ends with the last sample)"""
    C = cc.CHANNELS[fmt]
    if cc.planar(fmt):
        stride = w if stride is None else stride
        plane = h * stride if plane is None else plane
        pitch = 3 * plane if pitch is None else pitch
        return (B, 3, h, w), (pitch, plane, stride, 1), off, off + (B - 1) * pitch + 2 * plane + (h - 1) * stride + w
    stride = C * w if stride is None else stride
    pitch = h * stride if pitch is None else pitch
    return (B, h, w, C), (pitch, stride, C, 1), off, off + (B - 1) * pitch + (h - 1) * stride + C * w


def _dst_layout(B, h, w, off=0, pitch=None, stride=None):
    stride = w if stride is None else stride
    pitch = h * stride if pitch is None else pitch
    return (B, h, w), (pitch, stride, 1), off, off + (B - 1) * pitch + (h - 1) * stride + w


def _run(det, frames, fmt, want=None, src={}, dst={}):
    """frames [B, *frame shape] numpy; src: off, pitch, stride, plane; dst: off, pitch, stride -- in elements, default dense"""
    import torch
    dtype = frames.dtype
    B = frames.shape[0]
    h, w = cc.hw(fmt, frames.shape)
    fill = dtype.type(0xA5A5 & np.iinfo(dtype).max)
    want = cc.grey(frames, fmt) if want is None else want
    sshape, sstr, so, sn = _src_layout(fmt, B, h, w, **src)
    dshape, dstr, do, dn = _dst_layout(B, h, w, **dst)
    h_in = np.full(sn, fill, dtype)
    _strided(h_in, sshape, so, sstr)[...] = frames
    d_in, d_out = _dev(h_in), _dev(np.full(dn, fill, dtype))
    got = det.colour_grey(d_in.as_strided(sshape, sstr, so), fmt, out=d_out.as_strided(dshape, dstr, do))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, h, w) and got.data_ptr() == d_out.data_ptr() + do * dtype.itemsize
    back = _host(d_out)
    expect = np.full(dn, fill, dtype)
    _strided(expect, dshape, do, dstr)[...] = want
    if not np.array_equal(back, expect):
        bad = np.argwhere(_strided(back, dshape, do, dstr) != want)
        assert False, (fmt, str(dtype), (B, h, w), src, dst, "first wrong (frame, row, column):", bad[:4].tolist(), "of", len(bad),
                       "outside changed:", int((back != expect).sum()) - len(bad))
    assert np.array_equal(_host(d_in), h_in)


def _up16(v):
    return (v + 15) // 16 * 16


@pytest.mark.parametrize("fmt,dtype", CASES, ids=CASE_IDS)
def test_grey_equals_numpy(det, fmt, dtype):
    """every shape, three frames, dense; and the call without `out`"""
    import torch
    for k, (h, w) in enumerate(cc.SHAPES):
        _run(det, cc.random_frames(3, h, w, fmt, dtype, seed=1000 + k), fmt)
    frames = cc.random_frames(3, 9, 17, fmt, dtype, seed=5)
    got = det.colour_grey(_dev(frames), fmt)
    torch.cuda.synchronize()
    assert got.is_contiguous() and got.dtype == _dev(frames).dtype and np.array_equal(_host(got), cc.grey(frames, fmt))


@pytest.mark.parametrize("fmt,dtype", CASES, ids=CASE_IDS)
def test_views(det, fmt, dtype):
    """row strides that are no multiple of the pixel size, with an odd offset: source rows wander through the phases of a
    16-byte word; destination rows likewise.  Then rows a multiple of 16 bytes apart at every element offset: all rows of
    a call at one phase, every phase in turn, source and destination.  Planar: a plane pitch that puts the three planes
    at three different phases, and planes further apart than frames (a [3,B,H,W] tensor seen as [B,3,H,W])."""
    C = cc.CHANNELS[fmt] or 1
    es = np.dtype(dtype).itemsize
    for k, (h, w) in enumerate(((3, 5), (9, 17), (4, 33), (70, 33), (2, 300))):
        frames = cc.random_frames(3, h, w, fmt, dtype, seed=2000 + k)
        want = cc.grey(frames, fmt)
        stride = C * w + 7
        assert stride % C or C == 1
        plane = (h + 1) * stride + 5
        src = dict(off=stride + 3, stride=stride, pitch=(3 * plane + stride) if cc.planar(fmt) else (h + 2) * stride)
        if cc.planar(fmt):
            src["plane"] = plane
        _run(det, frames, fmt, want, src=src, dst=dict(off=2 * (w + 5) + 1, pitch=(h + 3) * (w + 5), stride=w + 5))
        _run(det, frames, fmt, want, src=src)
        _run(det, frames, fmt, want, dst=dict(off=1, pitch=h * (w + 2) + 1, stride=w + 2))
    B, h, w = 2, 9, 37
    frames = cc.random_frames(B, h, w, fmt, dtype, seed=3000)
    want = cc.grey(frames, fmt)
    stride = _up16(C * w) + 16
    for off in range(16 // es):
        src = dict(off=off, stride=stride, pitch=(3 * h + 1) * stride)
        if cc.planar(fmt):
            src["plane"] = h * stride + 5                                 # bytes 5, 10 (16 bit: 10, 20) behind a boundary
            assert len({(k * src["plane"] * es) % 16 for k in range(3)}) == 3
        _run(det, frames, fmt, want, src=src, dst=dict(off=(5 * off + 3) % (16 // es), pitch=704, stride=64))
    _run(det, frames, fmt, want, src=dict(stride=stride, pitch=(3 * h + 1) * stride), dst=dict(pitch=640, stride=64))
    if cc.planar(fmt):
        _run(det, frames, fmt, want, src=dict(pitch=h * w, plane=B * h * w))
        _run(det, frames, fmt, want, src=dict(off=3, stride=w + 3, pitch=h * (w + 3) + 1, plane=B * (h * (w + 3) + 1) + 7),
             dst=dict(off=5, stride=w + 1, pitch=h * (w + 1)))


@pytest.mark.parametrize("fmt,dtype", CASES, ids=CASE_IDS)
def test_seams_of_the_schedule(det, fmt, dtype):
    """a row one word wider than the lanes of a workgroup, whole and with a tail; more rows of one-word frames than one
    trip of the capped grid covers; 65537 frames of 1 x 2"""
    import torch
    lanes, per_cu = mrgingham_amd.colour_grey_geometry()
    npx = 16 // np.dtype(dtype).itemsize
    for i, w in enumerate(((lanes + 1) * npx, (lanes + 1) * npx + 5)):
        frames = cc.random_frames(2, 2, w, fmt, dtype, seed=10 + i)
        want = cc.grey(frames, fmt)
        _run(det, frames, fmt, want)
        _run(det, frames, fmt, want, src=dict(off=3), dst=dict(off=5, stride=w + 16))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = cus * per_cu * lanes + 1000                                    # (a workgroup takes at most `lanes` rows per trip)
    H = 32767
    B = -(-rows // H)
    few = cc.random_frames(1, 611, 3, fmt, dtype, seed=20)[0]           # 611 different rows, over and over
    idx = np.arange(B * H).reshape(B, H) % 611
    frames = np.moveaxis(few[:, idx], 0, 1) if cc.planar(fmt) else few[idx]
    _run(det, np.ascontiguousarray(frames), fmt, want=cc.grey(few, fmt)[idx])
    few = cc.random_frames(7, 1, 2, fmt, dtype, seed=21)
    idx = np.arange(65537) % 7
    _run(det, few[idx], fmt, want=cc.grey(few, fmt)[idx])


@pytest.mark.parametrize("fmt,dtype", CASES, ids=CASE_IDS)
def test_input_frames_may_repeat(det, fmt, dtype):
    """a frame pitch of 0 on the input (an expanded view): every output frame is the grey of the one frame"""
    import torch
    frame = cc.random_frames(1, 9, 17, fmt, dtype, seed=9)
    got = det.colour_grey(_dev(frame).expand(3, *frame.shape[1:]), fmt)
    torch.cuda.synchronize()
    assert np.array_equal(_host(got), np.repeat(cc.grey(frame, fmt), 3, axis=0))


@pytest.mark.parametrize("fmt,dtype", CASES, ids=CASE_IDS)
def test_impulses_and_all_top(det, fmt, dtype):
    """the top value in one sample of one pixel of a 3 x 5 frame in turn, every channel, as one batch: an alpha or chroma
    impulse changes nothing; all samples at the top value give the top value"""
    frames = cc.impulse_frames(fmt, dtype)
    want = cc.grey(frames, fmt)
    assert np.array_equal(~want.reshape(len(frames), -1).any(axis=1), cc.ignored(fmt))
    _run(det, frames, fmt, want)
    C = cc.CHANNELS[fmt] or 1
    _run(det, frames, fmt, want, src=dict(off=1, stride=5 * C + 4), dst=dict(off=3, stride=11))
    top = np.iinfo(dtype).max
    for h, w in ((1, 1), (3, 5), (9, 17), (4, 33)):
        _run(det, np.full((2,) + cc.frame_shape(fmt, h, w), top, dtype), fmt, want=np.full((2, h, w), top, dtype))


@pytest.mark.parametrize("fmt,dtype", CASES, ids=CASE_IDS)
def test_bad_arguments_are_refused_and_write_nothing(det, fmt, dtype):
    import torch
    es = np.dtype(dtype).itemsize
    bits = 8 * es
    f = mrgingham_amd.COLOUR_FORMATS[fmt]
    C = cc.CHANNELS[fmt] or 1
    fill = dtype(0x5A5A & np.iinfo(dtype).max)
    B, h, w = 2, 5, 9
    wide = cc.random_frames(B, h, w + 3, fmt, dtype, seed=3)             # the frames are its first w columns
    d_in = _dev(wide)
    n_out = (B * h) * (w + 2) + 16
    d_out = _dev(np.full(n_out, fill, dtype))
    in_stride, out_pitch, out_stride = C * (w + 3), h * (w + 2), w + 2
    plane = h * in_stride if cc.planar(fmt) else 0
    in_pitch = 3 * plane if cc.planar(fmt) else h * in_stride
    in_bytes = es * ((B - 1) * in_pitch + 2 * plane + (h - 1) * in_stride + C * w)

    def call(ctx=-1, d_i=None, bits_=bits, fmt_=f, n=B, width=w, height=h, ip=in_pitch, pp=plane, is_=in_stride, d_o=None, op=out_pitch,
             os_=out_stride):
        return det.L.mrgingham_amd_colour_grey_batch(det.ctx if ctx == -1 else ctx, d_in.data_ptr() if d_i is None else d_i, bits_, fmt_, n, width,
                                                     height, ip, pp, is_, d_out.data_ptr() if d_o is None else d_o, op, os_, None)
    bad = [dict(fmt_=8), dict(fmt_=-1), dict(bits_=12), dict(bits_=0), dict(bits_=32), dict(bits_=16, fmt_=6), dict(bits_=16, fmt_=7),
           dict(width=0), dict(height=0), dict(width=-1), dict(height=-1), dict(width=32768, is_=32768 * C, os_=32768), dict(height=32768),
           dict(is_=C * w - 1), dict(os_=w - 1), dict(is_=0), dict(os_=-out_stride), dict(d_i=0), dict(d_o=0), dict(n=-1), dict(ip=-1),
           dict(op=-1), dict(ctx=None),
           dict(op=(h - 1) * out_stride + w - 1),                                                  # output frames that overlap each other
           dict(d_o=d_in.data_ptr()), dict(d_o=d_in.data_ptr() + in_bytes - es),                   # output begins inside the input
           dict(d_i=d_out.data_ptr() + es * 8), dict(d_o=d_in.data_ptr() - es * ((B - 1) * out_pitch + (h - 1) * out_stride + w) + es)]
    if cc.planar(fmt):
        bad += [dict(pp=-1), dict(pp=-plane)]
    if es == 2:
        bad += [dict(d_i=d_in.data_ptr() + 1), dict(d_o=d_out.data_ptr() + 1)]                      # an odd uint16 address
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(d_o=d_in.data_ptr() + es) == -1 and b"overlap" in det.L.mrgingham_amd_last_error(det.ctx)
    assert call(n=0) == 0                                                 # nothing to do is not an error
    assert call(n=0, d_i=0, d_o=0) == 0
    torch.cuda.synchronize()
    assert (_host(d_out) == fill).all() and np.array_equal(_host(d_in), wide)
    assert call() == 0
    torch.cuda.synchronize()
    back = _host(d_out)
    view = d_in[..., :w] if cc.planar(fmt) else d_in[:, :, :w]
    frames = wide[..., :w] if cc.planar(fmt) else wide[:, :, :w]
    want = cc.grey(frames, fmt)
    assert np.array_equal(back[:B * h * (w + 2)].reshape(B, h, w + 2)[:, :, :w], want)
    assert (back[:B * h * (w + 2)].reshape(B, h, w + 2)[:, :, w:] == fill).all() and (back[B * h * (w + 2):] == fill).all()

    # the same through the Python method: each raises, and neither the frames nor `out` change
    keep = _dev(np.full((B, h, w), fill, dtype))
    other = torch.int16 if es == 2 else torch.int8
    for kw in (dict(format="rgbx"), dict(format=0), dict(format=None), dict(out=keep[:1]), dict(out=keep[:, :, :w - 1]),
               dict(out=keep.view(other)), dict(out=keep.cpu()), dict(out=_dev(np.zeros((B, h, 2 * w), dtype))[:, :, ::2]),
               dict(out=keep[:1].expand(B, h, w))):
        args = dict(format=fmt, out=keep)
        args.update(kw)
        with pytest.raises(ValueError):
            det.colour_grey(view, **args)
    wrong = "rgba" if C == 3 else "rgb"                                   # a format of another shape
    for frames_bad, fmt_bad in ((view.cpu(), fmt), (view[0], fmt), (view.view(other), fmt), (frames.astype(np.float32), fmt), (view, wrong),
                                (view[..., ::2] if cc.planar(fmt) else view[:, :, ::2], fmt), (view[:, :, :0], fmt)):
        with pytest.raises(ValueError):
            det.colour_grey(frames_bad, fmt_bad)
    if es == 2:
        with pytest.raises(ValueError):
            det.colour_grey(_dev(np.zeros((B, h, w, 2), dtype)), "yuyv")
    # `out` inside the tensor of the frames, either order
    inside = d_in.view(-1)
    lo = inside[:B * h * w].view(B, h, w)
    hi = inside[inside.numel() - B * h * w:].view(B, h, w)
    for o in (lo, hi):
        with pytest.raises(RuntimeError, match="overlap"):
            det.colour_grey(view, fmt, out=o)
    torch.cuda.synchronize()
    assert (_host(keep) == fill).all() and np.array_equal(_host(d_in), wide)
    assert tuple(det.colour_grey(view[:0], fmt).shape) == (0, h, w)


@pytest.mark.parametrize("channels,fmt", ((3, "rgb"), (4, "rgba")))
def test_contiguous_8_bit_frames_equal_pnm_unpack(det, channels, fmt):
    """the route a caller had before: the same bytes as a Netpbm payload of depth 3 / 4"""
    import torch
    for k, (h, w) in enumerate(((9, 17), (33, 130), (16, 64))):
        frames = cc.random_frames(3, h, w, fmt, np.uint8, seed=60 + k)
        nbytes = h * w * channels
        payload = np.zeros((3, _up16(nbytes)), np.uint8)
        payload[:, :nbytes] = frames.reshape(3, -1)
        old = det.pnm_unpack(_dev(payload), h, w, 8, channels)
        new = det.colour_grey(_dev(frames), fmt)
        torch.cuda.synchronize()
        assert torch.equal(old, new) and np.array_equal(_host(new), cc.grey(frames, fmt)), (h, w)


def test_tinted_boards_to_boards(det):
    """boards tinted R : G : B = 1 : 3/4 : 1/2, 640 x 480, four frames, every format at 8 bit: find_boards(colour_grey(..))
    at level 0 finds all four, equal double for double to the boards from the yardstick's grey uploaded.  Once at 16 bit
    (rgb_planar) through preprocess.  No pixel tolerance: equality with the yardstick's route is the whole claim."""
    for fmt in cc.FORMATS:
        m = np.stack([cc.tinted_board(seed, fmt) for seed in range(4)])
        want_boards, want_found = det.find_boards(_dev(cc.grey(m, fmt)), gridn=10, image_pyramid_level=0)
        boards, found = det.find_boards(det.colour_grey(_dev(m), fmt), gridn=10, image_pyramid_level=0)
        assert (np.asarray(found) >= 0).all() and np.array_equal(found, want_found), fmt
        assert np.array_equal(boards, want_boards), fmt
    m = np.stack([cc.tinted_board(seed, "rgb_planar", bits=16) for seed in range(4)])
    assert m.dtype == np.uint16 and m.max() > 2048
    want_boards, want_found = det.find_boards(det.preprocess(_dev(cc.grey(m, "rgb_planar"))), gridn=10, image_pyramid_level=0)
    boards, found = det.find_boards(det.preprocess(det.colour_grey(_dev(m), "rgb_planar")), gridn=10, image_pyramid_level=0)
    assert (np.asarray(found) >= 0).all() and np.array_equal(found, want_found)
    assert np.array_equal(boards, want_boards)


# ---------------------------------------------------------------------------------------------------- far views

@pytest.fixture(scope="module")
def far_buffers():
    """two buffers of far_views.BUFFER_BYTES (the frames, the output), freed at module teardown; skipped where the device
    has not the memory"""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * fv.BUFFER_BYTES + 2**30:
        pytest.skip("the device has not the memory for two far buffers")
    bufs = [torch.empty(fv.BUFFER_BYTES, dtype=torch.uint8, device="cuda") for _ in range(2)]
    yield bufs
    bufs.clear()
    torch.cuda.empty_cache()


def _writer(buf):
    import torch

    def write(at, data):
        buf[at:at + len(data)].copy_(torch.from_numpy(np.ascontiguousarray(data)))
    return write


def _reader(buf):
    return lambda at, n: buf[at:at + n].cpu().numpy()


@pytest.mark.parametrize("fmt,es", (("bgr", 1), ("rgba", 2), ("rgb_planar", 2), ("uyvy", 1)))
def test_far_views(det, far_buffers, fmt, es):
    """one case per layout, on two geometries of tests/far_views.py: three frames 2^31 + 2^22 bytes apart, input AND output
    (frame 2 begins beyond 4 GiB); and two frames whose rows lie 2^32 / 55 bytes apart, so that y * in_stride passes 2^32
    inside one frame.  Every far source row has its complement as a decoy at each address a 32-bit cut of the frame
    offset, the row offset or their sum would reach; the output's alias windows and guard bands must keep the sentinel.
    A source row is the w x C samples of its pixels (planar: a frame of 3h rows, the planes h rows apart)."""
    import torch
    frames_buf, out_buf = far_buffers
    dtype, tdtype = (np.uint8, torch.uint8) if es == 1 else (np.uint16, torch.uint16)
    C = cc.CHANNELS[fmt] or 1
    for name in ("far frames", "far rows"):
        if name == "far frames":
            h, w = 56, 130
            hs = 3 * h if cc.planar(fmt) else h                           # source rows of a frame
            g_in, g_out = fv.far_frames(hs, w * C, es, fv.PHASES[es][1]), fv.far_frames(h, w, es, fv.PHASES[es][1])
        else:
            # (the last row lies 304 bytes beyond 2^32: a row with its guard bands must fit in front of that alias)
            h, w = (18, 20) if cc.planar(fmt) else (56, 20)                # 18 rows a plane: three planes in the 56-row geometry
            g_in, g_out = fv.far_rows(56, w * C, "past2^32", es), fv.far_rows(56, w, "past2^32", es)
            if cc.planar(fmt):
                g_out = fv.Geometry("far-rows/out", 2, h, w, es, g_out.origin, g_out.pitch, g_out.stride)
                g_out.check(far=g_out.offset(1, h - 1) >= 2**31)
            assert (g_in.h - 1) * g_in.stride >= 2**32
        B = g_in.B
        frames = cc.random_frames(B, h, w, fmt, dtype, seed=es + len(name))
        want = cc.grey(frames, fmt)
        rows = np.zeros((B, g_in.h, w * C), dtype)                        # (far rows, planar: the last two source rows are nobody's)
        rows[:, :(3 * h if cc.planar(fmt) else h)] = frames.reshape(B, -1, w * C)
        plan = fv.coalesce(fv.input_plan(g_in, rows))
        fv.apply_plan(_writer(frames_buf), plan)
        fv.apply_plan(_writer(out_buf), fv.output_plan(g_out))
        view = g_in.torch_view(frames_buf, tdtype)
        view = view[:, :3 * h].unflatten(1, (3, h)) if cc.planar(fmt) else view.unflatten(2, (w, C))
        if name == "far frames":
            det.colour_grey(view, fmt, out=g_out.torch_view(out_buf, tdtype))
        else:                                                             # (the frames of the far rows interleave, which an output must not: one by one)
            for f in range(B):
                det.colour_grey(view[f:f + 1], fmt, out=g_out.torch_view(out_buf, tdtype)[f:f + 1])
        torch.cuda.synchronize()
        assert np.array_equal(_host(det.colour_grey(_dev(frames), fmt)), want), "the contiguous copy against the numpy statement"
        assert fv.plan_mismatches(_reader(out_buf), fv.output_plan(g_out, want)) == [], name
        assert fv.plan_mismatches(_reader(frames_buf), plan) == [], name
    with pytest.raises(RuntimeError, match="overlap"):                     # one frame, both in one buffer, 1 MiB apart: their rows interleave
        det.colour_grey(view[:1], fmt, out=fv.Geometry("beside", g_out.B, g_out.h, w, es, g_out.origin + 2**20, g_out.pitch,
                                                       g_out.stride).torch_view(frames_buf, tdtype)[:1])
