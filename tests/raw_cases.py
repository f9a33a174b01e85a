"""Packed 10 / 12 / 14-bit camera frames for the tests, written in numpy from the definitions of include/mrgingham_amd.h
alone: the yardstick of tests/test_raw_unpack.py and tests/test_gpu_raw.py.

Stream formats (p10, p12, p14): np.unpackbits / np.packbits with bitorder="little".  Pair formats (gev10, gev12): the
three byte formulas.  pack() sets what no sample owns -- the padding bits behind a row's last sample, the padding bytes
up to row_bytes, the ignored bits 2, 3, 6, 7 of a GEV10 middle byte -- to `fill` ones, so a decoder that looks at them
shows."""
import numpy as np

FORMATS = ("p10", "p12", "p14", "gev10", "gev12")
BITS = {"p10": 10, "p12": 12, "p14": 14, "gev10": 10, "gev12": 12}
PAIRS = ("gev10", "gev12")
# the shapes (h, w) every format is checked on: one pixel, odd widths, every width around one and two 16-byte words,
# more rows than a workgroup has row slots at that width, a row of several words
SHAPES = ((1, 1), (5, 3), (9, 17), (3, 7), (3, 8), (3, 9), (3, 15), (3, 16), (3, 17), (70, 33), (2, 300))


def min_row_bytes(w, fmt):
    return 3 * ((w + 1) // 2) if fmt in PAIRS else (w * BITS[fmt] + 7) // 8


def pack(a, fmt, row_bytes=None, fill=True):
    """uint16 [H, W] (values below 2**N) -> uint8 [H, row_bytes]"""
    a = np.asarray(a, dtype=np.uint16)
    h, w = a.shape
    n = BITS[fmt]
    assert int(a.max(initial=0)) < (1 << n)
    rmin = min_row_bytes(w, fmt)
    rowb = rmin if row_bytes is None else row_bytes
    assert rowb >= rmin
    out = np.full((h, rowb), 0xFF if fill else 0, dtype=np.uint8)
    if fmt in PAIRS:
        L = n - 8
        lm = (1 << L) - 1
        e = np.zeros((h, 2 * ((w + 1) // 2)), dtype=np.uint16)
        e[:, :w] = a
        if fill and w % 2:
            e[:, w] = (1 << n) - 1
        p0, p1 = e[:, 0::2], e[:, 1::2]
        mid = (p0 & lm) | ((p1 & lm) << 4)
        if fill:
            mid = mid | (0xFF & ~(lm | (lm << 4)))
        out[:, 0:rmin:3] = p0 >> L
        out[:, 1:rmin:3] = mid
        out[:, 2:rmin:3] = p1 >> L
    else:
        bits = np.full((h, rmin * 8), 1 if fill else 0, dtype=np.uint8)
        sample_bits = (a[:, :, None] >> np.arange(n, dtype=np.uint16)[None, None, :]) & 1
        bits[:, :w * n] = sample_bits.reshape(h, w * n)
        out[:, :rmin] = np.packbits(bits, axis=1, bitorder="little")
    return out


def unpack(rows, w, fmt):
    """uint8 [H, >= min_row_bytes] -> uint16 [H, W]: the yardstick"""
    rows = np.asarray(rows, dtype=np.uint8)
    h = rows.shape[0]
    n = BITS[fmt]
    rmin = min_row_bytes(w, fmt)
    if fmt in PAIRS:
        L = n - 8
        lm = (1 << L) - 1
        b0 = rows[:, 0:rmin:3].astype(np.uint16)
        b1 = rows[:, 1:rmin:3].astype(np.uint16)
        b2 = rows[:, 2:rmin:3].astype(np.uint16)
        e = np.empty((h, 2 * b0.shape[1]), dtype=np.uint16)
        e[:, 0::2] = (b0 << L) | (b1 & lm)
        e[:, 1::2] = (b2 << L) | ((b1 >> 4) & lm)
        return np.ascontiguousarray(e[:, :w])
    bits = np.unpackbits(rows[:, :rmin], axis=1, bitorder="little")[:, :w * n].reshape(h, w, n)
    out = np.zeros((h, w), dtype=np.uint16)
    for i in range(n):                                        # (bit by bit: no [H, W, N] array of wide integers)
        out |= bits[:, :, i].astype(np.uint16) << np.uint16(i)
    return out


# known answers: (format, samples, the bytes of the row)
KNOWN = (
    ("p12", (0xABC, 0x123), bytes.fromhex("BC3A12")),
    ("gev12", (0xABC, 0x123), bytes.fromhex("AB3C12")),
    ("p10", (0x3FF, 0, 0x2AA, 0x155), bytes.fromhex("FF03A06A55")),
    ("gev10", (0x2A7, 0x159), bytes.fromhex("A91356")),
)


def check_known():
    """the packer and the yardstick against the known answers, before either is trusted"""
    for fmt, samples, data in KNOWN:
        a = np.array([samples], dtype=np.uint16)
        assert pack(a, fmt, fill=False).tobytes() == data, fmt
        assert np.array_equal(unpack(np.frombuffer(data, np.uint8)[None, :], len(samples), fmt), a), fmt
        # the ones the packer puts where no sample lives change only those bits
        filled = pack(a, fmt)
        assert np.array_equal(unpack(filled, len(samples), fmt), a), fmt
        if fmt == "gev10":
            assert filled.tobytes() == bytes([data[0], data[1] | 0xCC, data[2]])


def random_frames(b, h, w, fmt, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << BITS[fmt], size=(b, h, w), dtype=np.uint16)


def every_value(fmt):
    """one frame that holds every value 0 .. 2^N - 1 once, in a shuffled order, at an odd width"""
    n = 1 << BITS[fmt]
    w = 257 if BITS[fmt] == 14 else 129
    h = (n + w - 1) // w
    v = np.random.default_rng(BITS[fmt]).permutation(n).astype(np.uint16)
    a = np.zeros(h * w, dtype=np.uint16)
    a[:n] = v
    return a.reshape(h, w)


def single_pixel_frames(fmt):
    """[32, 1, 16]: frame k < 16 holds 2^N - 1 at pixel k and 0 elsewhere, frame 16 + k the complement"""
    top = (1 << BITS[fmt]) - 1
    a = np.zeros((32, 1, 16), dtype=np.uint16)
    for k in range(16):
        a[k, 0, k] = top
        a[16 + k, 0, :] = top
        a[16 + k, 0, k] = 0
    return a


def payload(frames, fmt, row_bytes=None, pitch=None, tail=0xEE):
    """uint16 [B, H, W] -> uint8 [B, P]: every frame packed, P the frame's bytes rounded up to 16 (or `pitch`, which may
    cut the padding bytes of the last row), the bytes behind each frame `tail`"""
    b, h, w = frames.shape
    rows = [pack(f, fmt, row_bytes) for f in frames]
    nb = rows[0].size if b else 0
    p = (nb + 15) // 16 * 16 if pitch is None else pitch
    assert b == 0 or p >= nb - rows[0].shape[1] + min_row_bytes(w, fmt)
    out = np.full((b, p), tail, dtype=np.uint8)
    for i, r in enumerate(rows):
        out[i, :min(nb, p)] = r.reshape(-1)[:p]
    return out
