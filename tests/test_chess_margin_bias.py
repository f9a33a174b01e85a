"""The arithmetic behind the row mask of the clamped ChESS kernels (chess.hip, response_pair_biased), on the host.

A row of the zeroed 7-pixel frame takes the bias kYBiasFrameRow on Y instead of kYBias; the claim is that the same packed
32-bit expressions then give exactly 0 in both 16-bit halves after the saturating subtraction of the column-mask constant,
and that a row inside the frame gives what the kernel gave before (the clamped response inside the frame columns, 0
outside), with no borrow or carry between the halves.  Checked on the corners of the value ranges the derivation uses:
Y - X in {-1020, 0, 1020} x |M - LM| in {0, 4080} x both column-mask constants, independently in each half.
"""
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xffffffff


def _constants():
    src = open(os.path.join(ROOT, "mrgingham_amd", "csrc", "chess.hip")).read()
    m = re.search(r"constexpr uint32_t kYBias = (0x[0-9A-Fa-f]+)u, kYBiasFrameRow = (0x[0-9A-Fa-f]+)u;", src)
    assert m, "the bias constants of response_pair_biased"
    # the column-mask constants of the CLAMP kernels: inside / outside the frame columns, low half
    c = re.search(r"xmask\[k\] = \(ina \? (0x[0-9a-f]+)u : (0x[0-9a-f]+)u\) \| \(inb \? (0x[0-9a-f]+)u : (0x[0-9a-f]+)u\);", src)
    assert c, "the column-mask constants of chess_v1_body"
    lo_in, lo_out, hi_in, hi_out = (int(c.group(i), 16) for i in range(1, 5))
    assert (hi_in, hi_out) == (lo_in << 16, lo_out << 16)
    return int(m.group(1), 16), int(m.group(2), 16), lo_in, lo_out


def _pack(lo, hi):
    assert 0 <= lo <= 0xffff and 0 <= hi <= 0xffff
    return lo | (hi << 16)


def _pk_sub_sat_u16(a, b):   # v_pk_sub_u16 ... clamp
    return _pack(max((a & 0xffff) - (b & 0xffff), 0), max((a >> 16) - (b >> 16), 0))


def _biased(Y, X, dev, ybias):
    """The tail of response_pair_biased: plain 32-bit adds and subtracts on registers that hold two 16-bit values."""
    Yb = (Y + ybias) & M32
    d1x = (Yb - X) & M32
    return ((d1x + d1x) - dev) & M32


def test_frame_rows_saturate_to_zero_and_other_rows_are_unchanged():
    kYBias, kYBiasFrameRow, col_in, col_out = _constants()
    assert (kYBias, kYBiasFrameRow) == (0x10001000, 0x0C000C00)
    # (Y, X) with Y - X at the ends of its range and in the middle: Y <= 4 * 510, X <= 8 * 255 = 2040 and
    # 2 * (Y - X) = sum response - difference response, in [-2040, 2040]
    yx = [(1020, 2040), (0, 1020), (0, 0), (1020, 1020), (2040, 2040), (2040, 1020), (1020, 0)]
    assert sorted({y - x for y, x in yx}) == [-1020, 0, 1020]
    devs = [0, 4080]
    cols = [col_in, col_out]
    half = list(itertools.product(yx, devs, cols))
    n = 0
    for ((yl, xl), dl, cl), ((yh, xh), dh, ch) in itertools.product(half, half):
        Y, X, dev, col = _pack(yl, yh), _pack(xl, xh), _pack(dl, dh), _pack(cl, ch)
        resp = [2 * (yl - xl) - dl, 2 * (yh - xh) - dh]   # what ChESS.c:104 computes
        # a row inside the frame: the bias comes off again, negative responses clamp, frame columns are 0
        P = _biased(Y, X, dev, kYBias)
        assert [P & 0xffff, P >> 16] == [r + 8192 for r in resp]          # no borrow between the halves
        want = [max(r, 0) if c == col_in else 0 for r, c in zip(resp, (cl, ch))]
        assert _pk_sub_sat_u16(P, col) == _pack(*want)
        # a frame row: the same expressions with the smaller bias
        Pf = _biased(Y, X, dev, kYBiasFrameRow)
        assert [Pf & 0xffff, Pf >> 16] == [r + 6144 for r in resp]
        assert all(24 <= v <= 8184 for v in (Pf & 0xffff, Pf >> 16))
        assert _pk_sub_sat_u16(Pf, col) == 0
        # every intermediate stays inside its half
        for bias in (kYBias, kYBiasFrameRow):
            Yb = (Y + bias) & M32
            d = (Yb - X) & M32
            for v, b in ((Yb, bias), (d, bias)):
                assert 0 < (v & 0xffff) < 0x8000 and 0 < (v >> 16) < 0x8000
            assert [d & 0xffff, d >> 16] == [yl - xl + (bias & 0xffff), yh - xh + (bias >> 16)]
        n += 1
    assert n == (7 * 2 * 2) ** 2


def test_the_saturation_needs_the_smaller_bias():
    """The column constant inside the frame is 8192: with the normal bias a positive response survives it, so the frame
    row really is zeroed by the bias and by nothing else."""
    kYBias, kYBiasFrameRow, col_in, _ = _constants()
    Y, X, dev = _pack(2040, 2040), _pack(1020, 1020), 0
    assert _pk_sub_sat_u16(_biased(Y, X, dev, kYBias), _pack(col_in, col_in)) == _pack(2040, 2040)
    assert _pk_sub_sat_u16(_biased(Y, X, dev, kYBiasFrameRow), _pack(col_in, col_in)) == 0
    assert 2 * (kYBiasFrameRow & 0xffff) + 2040 < col_in <= 2 * (kYBias & 0xffff)
