"""Files whose raster begins at a chosen byte, around the 4096 bytes every reader reads of a file first (probe_image and
the batch loaders): 17 x 5 binary PGM and PAM files whose header a '#' comment pads, and a 40 x 35 24-bit BMP whose pixel
array begins inside the first 4096 bytes and ends behind them.  For tests/test_file_heads.py and the GPU loader tests."""
from tests import bmp_cases, pnm_cases

W, H = 17, 5
STARTS = (4095, 4096, 4097, 8193)     # where the samples of a padded file begin: around one head, behind two
PAM = {8: (1, "GRAYSCALE"), 16: (3, "RGB")}    # the PAM of a depth: channels, TUPLTYPE


def samples(bits, channels):
    return pnm_cases.random_samples(W, H, bits, channels, seed=bits + channels)


def grey(bits, channels):
    """the grey [H, W] the files of these samples read to: uint8, or uint16 (read_image gives its high bytes)"""
    return pnm_cases.expected(samples(bits, channels), bits, channels)


def _padded(front, rest, start):
    """front + a comment line + rest, `start` bytes long (None: no comment)"""
    if start is None:
        return front + rest
    pad = start - len(front) - len(rest) - 2
    assert pad >= 0
    return front + b"#" + b"c" * pad + b"\n" + rest


def pgm(bits, start=None):
    """-> (file bytes, where its samples begin)"""
    head = _padded(b"P5\n", b"%d %d\n%d\n" % (W, H, pnm_cases.default_maxval(bits)), start)
    return head + pnm_cases.raster(samples(bits, 1), bits), len(head)


def pam(bits, start=None):
    channels, tupltype = PAM[bits]
    plain = pnm_cases.pam_head(W, H, channels, pnm_cases.default_maxval(bits), tupltype)
    head = _padded(plain[:3], plain[3:], start)
    return head + pnm_cases.raster(samples(bits, channels), bits), len(head)


def bmp24():
    """-> (file bytes, where its pixel array begins, the grey it reads to): 40 x 35, so that the array crosses byte 4096"""
    pixels = bmp_cases.random_pixels(40, 35, 24, seed=3)
    data = bmp_cases.write(pixels, 24)
    off = int.from_bytes(data[10:14], "little")
    assert off < 4096 < off + bmp_cases.row_bytes(40, 24) * 35 == len(data)
    return data, off, bmp_cases.expected(pixels, 24)
