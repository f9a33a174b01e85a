"""Packed 10 / 12 / 14-bit camera frames to uint16 frames on the device (Detector.raw_unpack, csrc/raw_unpack.hip over
csrc/raw_pixels.h).  The yardstick is numpy (tests/raw_cases.py: np.unpackbits for the bit streams, the three byte
formulas for the pixel pairs), held against the known answers of the format definitions first.  np.array_equal
everywhere, no tolerance.

The shapes sit where the kernel can go wrong: dense frames of odd size put the destination rows at every 2-byte phase of
a 16-byte word, so a lane's word begins at odd pixels and at every bit phase of the stream; odd row_bytes put the source
rows at all four byte phases of a dword.  Nothing but the row-loop cases is larger than 640 x 480."""
import numpy as np
import pytest

import mrgingham_amd
from mrgingham_amd import synth
from tests import raw_cases as rc

pytestmark = pytest.mark.gpu

SHAPES = rc.SHAPES + ((2, 4200),)                                 # (a row of more words than a workgroup has lanes)


@pytest.fixture(scope="module")
def det():
    rc.check_known()
    d = mrgingham_amd.Detector()
    yield d
    d.close()


def _up16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def _unpack(det, pay, h, w, fmt, row_bytes=None, out=None):
    import torch
    got = det.raw_unpack(torch.from_numpy(pay).cuda(), h, w, fmt, row_bytes=row_bytes, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _row_bytes_of(h, w, fmt):
    """the row_bytes a shape runs at: the minimum, three more, and for two shapes the next multiple of 16"""
    rmin = rc.min_row_bytes(w, fmt)
    rowbs = [rmin, rmin + 3]
    if (h, w) in ((9, 17), (70, 33)):
        rowbs.append((rmin + 15) // 16 * 16)
    return rowbs


@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_unpack_equals_numpy(det, fmt):
    """nine dense frames per shape and row_bytes; the bytes behind each payload are 0xEE"""
    cases = [(h, w, rowb) for h, w in SHAPES for rowb in _row_bytes_of(h, w, fmt)]
    assert any(rowb % 2 == 1 and h >= 4 for h, w, rowb in cases)      # source rows at all four byte phases of a dword
    assert any(rowb % 16 == 0 for h, w, rowb in cases)
    assert any((h * w) % 2 == 1 for h, w, rowb in cases)              # destination rows at every 2-byte phase of a word
    for k, (h, w, rowb) in enumerate(cases):
        frames = rc.random_frames(9, h, w, fmt, seed=1000 * rc.BITS[fmt] + k)
        pay = rc.payload(frames, fmt, rowb, pitch=(h * rowb + 15) // 16 * 16 + 16)
        assert (pay[:, h * rowb:] == 0xEE).all()
        want = np.stack([rc.unpack(pay[f, :h * rowb].reshape(h, rowb), w, fmt) for f in range(9)])
        assert np.array_equal(want, frames)
        got = _unpack(det, pay, h, w, fmt, row_bytes=rowb)
        assert got.dtype == np.uint16 and got.shape == (9, h, w)
        assert np.array_equal(got, want), (h, w, rowb)
        if rowb == rc.min_row_bytes(w, fmt):
            assert np.array_equal(_unpack(det, pay, h, w, fmt), want), (h, w)              # the default row


@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_every_value_once(det, fmt):
    """(a wrong mask or shift cannot hide)"""
    a = rc.every_value(fmt)
    h, w = a.shape
    got = _unpack(det, rc.payload(a[None], fmt), h, w, fmt)
    assert np.array_equal(got[0], a)
    # and nothing leaks between neighbours: 2^N - 1 at one of the pixels 0 .. 15, and the complement
    frames = rc.single_pixel_frames(fmt)
    assert np.array_equal(_unpack(det, rc.payload(frames, fmt), 1, 16, fmt), frames)


@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_strided_out_keeps_what_lies_outside(det, fmt):
    import torch
    for h, w in ((5, 3), (9, 17), (3, 16), (70, 33)):
        frames = rc.random_frames(3, h, w, fmt, seed=h * w)
        pay = rc.payload(frames, fmt)
        big = torch.full((3, h + 2, (w + 5) * 2), 0xA5, dtype=torch.uint8, device="cuda").view(torch.uint16)
        assert tuple(big.shape) == (3, h + 2, w + 5)
        got = _unpack(det, pay, h, w, fmt, out=big[:, :h, :])
        assert got.shape == (3, h, w) and np.array_equal(got, frames), (h, w)
        back = big.cpu().numpy()
        assert np.array_equal(back[:, :h, :w], frames), (h, w)
        assert (back[:, :h, w:] == 0xA5A5).all() and (back[:, h:, :] == 0xA5A5).all(), (h, w)


@pytest.mark.parametrize("rows_per_workgroup", [1, 256])
def test_unpack_takes_a_second_trip_over_the_rows(det, rows_per_workgroup):
    """The grid is capped at max_workgroups_per_cu workgroups per CU and the kernel loops over the rows beyond.  A row is
    taken by the power of two of lanes that covers its 16-byte words: a workgroup holds one dense row of 1025 samples (129
    words and one more, the rows beginning inside a word) or 256 aligned rows of 8.  The smallest row count above one
    trip, the last trip ragged.  P12."""
    import torch
    lanes, per_cu = mrgingham_amd.raw_unpack_geometry()
    assert lanes == 256
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows_per_trip = per_cu * cus * rows_per_workgroup
    if rows_per_workgroup == 1:
        B, h, w = 1, rows_per_trip + 37, 1025
        assert (2 * w + 15) // 16 + 1 > lanes // 2 and (2 * w) % 16 != 0
    else:
        w = 8
        h = next(h for h in range(4099, 4200) if ((rows_per_trip // h + 1) * h - rows_per_trip) % 256)
        B = rows_per_trip // h + 1
    nrows = B * h
    assert rows_per_trip < nrows < 2 * rows_per_trip
    assert (nrows - rows_per_trip) % rows_per_workgroup or rows_per_workgroup == 1
    rowb = rc.min_row_bytes(w, "p12")
    raw = np.random.default_rng(rows_per_workgroup).integers(0, 256, (B, (h * rowb + 15) // 16 * 16), dtype=np.uint8)
    want = rc.unpack(raw[:, :h * rowb].reshape(B * h, rowb), w, "p12").reshape(B, h, w)
    got = _unpack(det, raw, h, w, "p12")
    assert got.shape == (B, h, w) and np.array_equal(got, want)


@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_last_frame_without_padding_behind_its_last_sample(det, fmt):
    """a payload tensor of exactly B*P bytes, P the frame's own size: the tail of the last row of the last frame ends
    where the tensor ends, and its values are right"""
    for h, w in ((4, 32), (16, 16), (8, 40)):
        rowb = rc.min_row_bytes(w, fmt)
        assert (h * rowb) % 16 == 0, (h, w, fmt)
        frames = rc.random_frames(3, h, w, fmt, seed=7 * h + w)
        pay = rc.payload(frames, fmt)
        assert pay.shape == (3, h * rowb)
        assert np.array_equal(_unpack(det, pay, h, w, fmt), frames), (h, w)
    # ... and with the last row's samples ending inside the last dword of the tensor
    w = 9
    rmin = rc.min_row_bytes(w, fmt)
    h, rowb = next((h, r) for h in (5, 6, 7, 8) for r in range(rmin, rmin + 64) if -((h - 1) * r + rmin) % 16 in (1, 2, 3))
    frames = rc.random_frames(2, h, w, fmt, seed=3)
    pitch = ((h - 1) * rowb + rmin + 15) // 16 * 16
    pay = rc.payload(frames, fmt, rowb, pitch=pitch)
    assert pay.shape == (2, pitch) and 1 <= pitch - ((h - 1) * rowb + rmin) <= 3
    assert np.array_equal(_unpack(det, pay, h, w, fmt, row_bytes=rowb), frames)


def test_bad_arguments_raise_and_write_nothing(det):
    import torch
    h, w, fmt = 5, 9, "p12"
    rmin = rc.min_row_bytes(w, fmt)
    rowb = rmin + 2
    frames = rc.random_frames(1, h, w, fmt, seed=3)
    pay = rc.payload(frames, fmt, rowb, pitch=(h * rowb + 15) // 16 * 16 + 16)
    pitch = pay.shape[1]
    d_pay = torch.from_numpy(pay).cuda()
    out = torch.full((2 * (h * w + 8),), 0x5A, dtype=torch.uint8, device="cuda").view(torch.uint16)
    need = (h - 1) * rowb + rmin

    def call(d_payload=None, payload_pitch=pitch, n=1, width=w, height=h, row_bytes=rowb, f=1, d_out=None, frame_pitch=w * h, stride=w, ctx=-1):
        return det.L.mrgingham_amd_raw_unpack_batch(det.ctx if ctx == -1 else ctx, d_pay.data_ptr() if d_payload is None else d_payload,
                                                    payload_pitch, n, width, height, row_bytes, f,
                                                    out.data_ptr() if d_out is None else d_out, frame_pitch, stride, None)
    bad = [dict(f=5), dict(f=-1), dict(row_bytes=rmin - 1), dict(row_bytes=0), dict(row_bytes=-rowb), dict(payload_pitch=pitch + 8),
           dict(payload_pitch=need // 16 * 16), dict(payload_pitch=-16), dict(row_bytes=rowb + 16), dict(d_payload=d_pay.data_ptr() + 4),
           dict(d_payload=d_pay.data_ptr() + 8), dict(d_payload=0), dict(d_out=0), dict(d_out=out.data_ptr() + 1), dict(n=-1),
           dict(width=0, stride=0), dict(width=-1), dict(height=0), dict(height=-1), dict(stride=w - 1), dict(frame_pitch=-1),
           dict(width=32768, stride=32768, payload_pitch=1 << 40), dict(height=32768, payload_pitch=1 << 40), dict(ctx=None),
           dict(d_out=d_pay.data_ptr()), dict(d_out=d_pay.data_ptr() + pitch - 2), dict(d_payload=out.data_ptr() // 16 * 16)]
    assert need // 16 * 16 < need <= pitch - 16 and (h - 1) * (rowb + 16) + rmin > pitch and out.data_ptr() % 16 == 0
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(n=0) == 0                                                 # nothing to do is not an error
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A).all() and np.array_equal(d_pay.cpu().numpy(), pay)
    assert call() == 0
    torch.cuda.synchronize()
    back = out.cpu().numpy()
    assert np.array_equal(back[:h * w].reshape(h, w), frames[0]) and (back[h * w:] == 0x5A5A).all()

    # the same through the Python method: each raises, and neither the payload nor `out` changes
    keep = torch.full((1, h, 2 * w), 0x5A, dtype=torch.uint8, device="cuda").view(torch.uint16)
    for kw in (dict(fmt="p16"), dict(fmt=1), dict(row_bytes=rmin - 1), dict(row_bytes=rowb + 16)):
        args = dict(fmt=fmt, row_bytes=rowb, out=keep)
        args.update(kw)
        with pytest.raises(ValueError):
            det.raw_unpack(d_pay, h, w, **args)
    with pytest.raises(ValueError):                                       # a pitch that is no multiple of 16
        det.raw_unpack(d_pay[:, :pitch - 8].contiguous(), h, w, fmt, row_bytes=rowb, out=keep)
    with pytest.raises(ValueError):                                       # ... or too small
        det.raw_unpack(d_pay[:, :need // 16 * 16].contiguous(), h, w, fmt, row_bytes=rowb, out=keep)
    with pytest.raises(ValueError):                                       # a misaligned payload
        det.raw_unpack(torch.from_numpy(np.concatenate([pay[0], pay[0]])).cuda()[8:8 + pitch].view(1, pitch), h, w, fmt, row_bytes=rowb, out=keep)
    inside = d_pay.view(-1)[:2 * h * w].view(torch.uint16).view(1, h, w)  # `out` inside the payload
    assert 2 * h * w <= pitch
    with pytest.raises(RuntimeError, match="overlap"):
        det.raw_unpack(d_pay, h, w, fmt, row_bytes=rowb, out=inside)
    torch.cuda.synchronize()
    assert (keep.cpu().numpy() == 0x5A5A).all() and np.array_equal(d_pay.cpu().numpy(), pay)
    assert tuple(det.raw_unpack(d_pay[:0], h, w, fmt, row_bytes=rowb).shape) == (0, h, w)


def test_packed_frames_to_boards(det):
    """find_boards(preprocess(raw_unpack(..))) on 12-bit frames packed as P12 and as GEV12 against the same two calls on the
    uint16 frames uploaded directly: the same boards and corner levels, double for double; all four boards found"""
    W, H = 640, 480
    f8 = synth.board_batch(4, W, H).numpy()
    f12 = f8.astype(np.uint16) * 16 + (f8 >> 4)                           # 0 .. 4095
    assert f12.max() <= 4095 and f12.max() > 2048
    want_boards, want_found, want_levels = det.find_boards(det.preprocess(_up16(f12)), gridn=10, levels=True)
    assert (np.asarray(want_found) >= 0).all()
    import torch
    for fmt in ("p12", "gev12"):
        frames = det.raw_unpack(torch.from_numpy(rc.payload(f12, fmt)).cuda(), H, W, fmt)
        assert np.array_equal(frames.cpu().numpy(), f12)
        boards, found, levels = det.find_boards(det.preprocess(frames), gridn=10, levels=True)
        assert np.array_equal(found, want_found) and (np.asarray(found) >= 0).all(), fmt
        assert np.array_equal(boards, want_boards) and np.array_equal(levels, want_levels), fmt
