"""The numpy yardstick of the colour-to-grey definition (include/mrgingham_amd.h at MRGINGHAM_AMD_COLOUR_RGB), written from
the definition alone, the known answers it is held against (check_known), and the frames the host and the device tests
share.

A frame is kept in the shape the entry points take: [h, w, C] with C = 3 (rgb, bgr), 4 (rgba, bgra) or 2 (yuyv, uyvy), or
[3, h, w] for the planar formats."""
import numpy as np

FORMATS = ("rgb", "bgr", "rgba", "bgra", "rgb_planar", "bgr_planar", "yuyv", "uyvy")
DTYPES = (np.uint8, np.uint16)
# samples of a pixel along the last axis; 0: planar
CHANNELS = {"rgb": 3, "bgr": 3, "rgba": 4, "bgra": 4, "rgb_planar": 0, "bgr_planar": 0, "yuyv": 2, "uyvy": 2}
# around one and two 16-byte destination words at both sample widths (8 and 16 pixels), heights 1 and odd
SHAPES = ((1, 1), (1, 2), (2, 3), (3, 5), (5, 15), (4, 16), (9, 17), (3, 31), (4, 33), (70, 33), (33, 130), (2, 300))
CR, CG, CB = 4899, 9617, 1868


def allowed(fmt, dtype):
    """the 4:2:2 forms are 8 bit"""
    return CHANNELS[fmt] != 2 or np.dtype(dtype) == np.uint8


def cases():
    return [(fmt, dtype) for fmt in FORMATS for dtype in DTYPES if allowed(fmt, dtype)]


def planar(fmt):
    return CHANNELS[fmt] == 0


def frame_shape(fmt, h, w):
    return (3, h, w) if planar(fmt) else (h, w, CHANNELS[fmt])


def hw(fmt, shape):
    """(h, w) of a frame's shape (the last three axes)"""
    return tuple(shape[-2:]) if planar(fmt) else tuple(shape[-3:-1])


def rgb_of(frame, fmt):
    """(R, G, B) as uint64 arrays [.., h, w] of a frame or a batch of frames in format `fmt` (not the 4:2:2 forms)"""
    a = np.asarray(frame).astype(np.uint64)
    s = (a[..., 0, :, :], a[..., 1, :, :], a[..., 2, :, :]) if planar(fmt) else (a[..., 0], a[..., 1], a[..., 2])
    return s[::-1] if fmt.startswith("bgr") else s


def grey(frame, fmt):
    """the definition, in uint64 arithmetic, on a frame or a batch of frames"""
    a = np.asarray(frame)
    assert a.dtype in (np.uint8, np.uint16) and allowed(fmt, a.dtype)
    if CHANNELS[fmt] == 2:
        return a[..., 1 if fmt == "uyvy" else 0].copy()
    r, g, b = rgb_of(a, fmt)
    s = CR * r + CG * g + CB * b + 8192
    assert int(s.max(initial=0)) < 1 << 32
    return (s >> 14).astype(a.dtype)


def from_rgb(rgb, fmt, extra):
    """an [.., h, w, 3] R, G, B image in format `fmt` (not the 4:2:2 forms); extra [.., h, w]: the fourth sample"""
    c = rgb[..., ::-1] if fmt.startswith("bgr") else rgb
    if planar(fmt):
        return np.ascontiguousarray(np.moveaxis(c, -1, -3))
    if CHANNELS[fmt] == 4:
        return np.ascontiguousarray(np.concatenate([c, extra[..., None]], axis=-1))
    return np.ascontiguousarray(c)


KNOWN = ((np.uint8, 255, (76, 150, 29)), (np.uint16, 65535, (19596, 38467, 7472)))


def check_known(fn=grey):
    for dtype, top, answers in KNOWN:
        for fmt in FORMATS[:6]:
            for ch, want in enumerate(answers):                      # pure R, G, B at the top value
                rgb = np.zeros((3, 5, 3), dtype)
                rgb[..., ch] = top
                got = fn(from_rgb(rgb, fmt, np.full((3, 5), 0x5A, dtype)), fmt)
                assert got.dtype == dtype and got.shape == (3, 5) and (got == want).all(), (fmt, dtype, ch, got.tolist())
            for v in (0, 1, 77, top):                                # equal samples v give v
                rgb = np.full((2, 17, 3), v, dtype)
                assert (fn(from_rgb(rgb, fmt, np.zeros((2, 17), dtype)), fmt) == v).all(), (fmt, dtype, v)
    y = np.arange(15, dtype=np.uint8).reshape(3, 5) * 17              # 4:2:2: the Y byte as it is
    for fmt in ("yuyv", "uyvy"):
        f = np.full((3, 5, 2), 0x80, np.uint8)
        f[..., 1 if fmt == "uyvy" else 0] = y
        assert np.array_equal(fn(f, fmt), y), fmt


def random_frames(n, h, w, fmt, dtype, seed):
    """[n, *frame_shape]: the full sample range in every sample, the ignored ones included"""
    return np.random.default_rng(seed).integers(0, int(np.iinfo(dtype).max) + 1, (n,) + frame_shape(fmt, h, w), dtype=dtype)


def impulse_frames(fmt, dtype, h=3, w=5):
    """the top value in one sample of one pixel of an h x w frame and 0 elsewhere, in turn for every sample of every pixel
    (the ignored ones included): [h*w*C, *frame_shape]"""
    shape = frame_shape(fmt, h, w)
    n = int(np.prod(shape))
    a = np.zeros((n, n), dtype)
    a[np.arange(n), np.arange(n)] = np.iinfo(dtype).max
    return a.reshape((n,) + shape)


def ignored(fmt, h=3, w=5):
    """bool [h*w*C]: the impulses of impulse_frames that hit a sample the definition never looks at"""
    idx = np.arange(int(np.prod(frame_shape(fmt, h, w)))).reshape(frame_shape(fmt, h, w))
    if CHANNELS[fmt] == 4:
        keep = idx[..., 3]
    elif CHANNELS[fmt] == 2:
        keep = idx[..., 0 if fmt == "uyvy" else 1]
    else:
        keep = idx[:0]
    out = np.zeros(idx.size, bool)
    out[keep.reshape(-1)] = True
    return out


def tinted_board(seed, fmt, W=640, H=480, gridn=10, bits=8):
    """synth.board_frame times 1 : 3/4 : 1/2 per channel in format `fmt`; bits 16: f*16 + (f >> 4) first.  The fourth sample
    is the complement of the board; 4:2:2: Y is the frame tinted and greyed by the definition, chroma a ramp."""
    from mrgingham_amd import synth
    f = synth.board_frame(W, H, gridn, seed).numpy().astype(np.uint32)
    dtype = np.uint8
    if bits == 16:
        f, dtype = f * 16 + (f >> 4), np.uint16
    rgb = np.stack([f, f * 3 // 4, f // 2], axis=-1).astype(dtype)
    if CHANNELS[fmt] == 2:
        out = np.empty((H, W, 2), np.uint8)
        out[..., 1 if fmt == "uyvy" else 0] = grey(rgb, "rgb")
        out[..., 0 if fmt == "uyvy" else 1] = (np.arange(W) * 7 + np.arange(H)[:, None] * 3) & 255
        return out
    return from_rgb(rgb, fmt, (np.iinfo(dtype).max - f).astype(dtype))
