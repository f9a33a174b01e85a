"""Windows Bitmap files for the tests of the BMP reader (tests/test_bmp_io.py, tests/test_gpu_bmp.py): a writer that shares
nothing with the library or with Pillow, the grey a file must read to, RLE8 streams built by hand, and a corpus of files
that each break one rule of the subset (include/mrgingham_amd.h: mrgingham_amd_bmp_layout)."""
import struct

import numpy as np

HEADERS = (40, 52, 56, 108, 124)
MASKS = (0x00FF0000, 0x0000FF00, 0x000000FF)


def grey(r, g, b):
    """the library's one set of grey weights (csrc/png_filter.h: png_grey), on integers or integer arrays"""
    return (np.asarray(r, np.int64) * 4899 + np.asarray(g, np.int64) * 9617 + np.asarray(b, np.int64) * 1868 + 8192) >> 14


def row_bytes(width, bits):
    return (width * bits + 31) // 32 * 4


def grey_ramp(n=256):
    """the palette of a grey camera file: entry i is (i, i, i)"""
    return np.stack([np.arange(n, dtype=np.uint8)] * 3, axis=1)


def random_palette(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


def random_pixels(width, height, bits, seed=0, top=None):
    """indices [h, w] below `top` (default 2^bits) for palette depths, samples [h, w, 3] for 24 and [h, w, 4] for 32 bits"""
    rng = np.random.default_rng(seed)
    if bits <= 8:
        return rng.integers(0, top or (1 << bits), (height, width)).astype(np.uint8)
    return rng.integers(0, 256, (height, width, 3 if bits == 24 else 4)).astype(np.uint8)


def expected(pixels, bits, palette=None):
    """the grey [h, w] uint8 the file reads to: palette entries (R, G, B rows) through the weights, an index beyond the
    palette 0; colour samples (R, G, B[, X]) through the weights, X ignored"""
    pixels = np.asarray(pixels)
    if bits <= 8:
        lut = np.zeros(256, np.uint8)
        pal = np.asarray(palette)
        lut[:len(pal)] = grey(pal[:, 0], pal[:, 1], pal[:, 2])
        return lut[pixels]
    return grey(pixels[..., 0], pixels[..., 1], pixels[..., 2]).astype(np.uint8)


def pack_rows(pixels, bits):
    """[h, w(, c)] -> the rows as they lie in a file, top row first: uint8 [h, row_bytes]; the padding is 0xEE, not zero
    (what lies behind a row's pixels is never a sample)"""
    pixels = np.asarray(pixels)
    h, w = pixels.shape[:2]
    out = np.full((h, row_bytes(w, bits)), 0xEE, np.uint8)
    if bits == 8:
        out[:, :w] = pixels
    elif bits in (1, 4):
        per = 8 // bits
        padded = np.zeros((h, (w + per - 1) // per * per), np.uint8)
        padded[:, :w] = pixels
        # (the unused low bits of a row's last byte are set as well)
        padded[:, w:] = (1 << bits) - 1
        acc = np.zeros((h, padded.shape[1] // per), np.uint8)
        for k in range(per):
            acc |= (padded[:, k::per] << (8 - bits * (k + 1))).astype(np.uint8)
        out[:, :acc.shape[1]] = acc
    elif bits == 24:
        out[:, :3 * w] = pixels[..., ::-1].reshape(h, 3 * w)                      # B G R
    else:
        out[:, :4 * w] = pixels[..., [2, 1, 0, 3]].reshape(h, 4 * w)              # B G R X
    return out


def info_header(size, width, height, bits, compression, clr_used, planes=1, masks=MASKS):
    """BITMAPINFOHEADER, or one of its longer forms: the masks at bytes 40 .. 52 (56 with alpha), zeros behind them"""
    head = struct.pack("<IiiHHIIiiII", size, width, height, planes, bits, compression, 0, 2835, 2835, clr_used, 0)
    if size > 40:
        head += struct.pack("<III", *masks)
    if size > 52:
        head += struct.pack("<I", 0xFF000000 if bits == 32 else 0)
    if size > 56:
        head += b"sRGB"[::-1] + bytes(size - 60)
    assert len(head) == size
    return head


def assemble(info, palette_bytes, payload, gap=0, off_bits=None):
    """file header + info header (+ masks) + palette + gap + pixel array; bfSize is left 0 (it is not trusted)"""
    front = 14 + len(info) + len(palette_bytes) + gap
    off = front if off_bits is None else off_bits
    return b"BM" + struct.pack("<IHHI", 0, 0, 0, off) + info + palette_bytes + bytes(gap) + payload


def palette_bytes(palette):
    pal = np.asarray(palette, np.uint8)
    quad = np.zeros((len(pal), 4), np.uint8)
    quad[:, 0], quad[:, 1], quad[:, 2] = pal[:, 2], pal[:, 1], pal[:, 0]
    quad[:, 3] = 0x55                                                              # (the fourth byte is nobody's)
    return quad.tobytes()


def write(pixels, bits, palette=None, top_down=False, header=40, clr_used=None, bitfields=False, gap=0, masks=MASKS):
    """An uncompressed file (compression 0, or 3 with `bitfields`).  palette: [n, 3] R G B for bits <= 8; clr_used: the
    field's value (default: 0 for a full palette, else its length); gap: bytes between the palette and the pixels."""
    pixels = np.asarray(pixels)
    h, w = pixels.shape[:2]
    rows = pack_rows(pixels, bits)
    if not top_down:
        rows = rows[::-1]
    pal = b""
    used = 0
    if bits <= 8:
        pal = palette_bytes(palette)
        used = (0 if len(palette) == 1 << bits else len(palette)) if clr_used is None else clr_used
    info = info_header(header, w, -h if top_down else h, bits, 3 if bitfields else 0, used, masks=masks)
    if bitfields and header == 40:
        info += struct.pack("<III", *masks)
    return assemble(info, pal, rows.tobytes(), gap)


# ---- RLE8 -------------------------------------------------------------------------------------------------------------
def rle8_encode(indices):
    """a plain encoder: per row (bottom row first) encoded runs, end of line; end of bitmap"""
    out = bytearray()
    for row in np.asarray(indices)[::-1]:
        x = 0
        while x < len(row):
            n = 1
            while x + n < len(row) and n < 255 and row[x + n] == row[x]:
                n += 1
            out += bytes([n, int(row[x])])
            x += n
        out += b"\x00\x00"
    return bytes(out) + b"\x00\x01"


def write_rle8(width, height, stream, palette, top_down=False, header=40, compression=1, bits=8):
    info = info_header(header, width, -height if top_down else height, bits, compression, 0 if len(palette) == 256 else len(palette))
    return assemble(info, palette_bytes(palette), bytes(stream))


def rle8_every_escape():
    """-> (width, height, stream, indices [h, w]): an encoded run, an absolute run of odd length with its pad byte, an end
    of line in mid-row, a delta, pixels never written (index 0), end of bitmap before the top row is full"""
    w, h = 9, 5
    want = np.zeros((h, w), np.uint8)
    s = bytearray()
    # bottom row (y = 0): a run of 4 x 7, an absolute run of 3 (odd: padded), end of line with two pixels unwritten
    s += bytes([4, 7]) + bytes([0, 3, 11, 12, 13, 0xAA]) + bytes([0, 0])
    want[h - 1, :4] = 7
    want[h - 1, 4:7] = [11, 12, 13]
    # y = 1: end of line at once; y = 2: delta (+2, +1) to (2, 3), a run of 5 x 200
    s += bytes([0, 0]) + bytes([0, 2, 2, 1]) + bytes([5, 200])
    want[h - 1 - 3, 2:7] = 200
    # a run that ends the row exactly, end of line; y = 4: an absolute run of 4 (even: no pad), end of bitmap in mid-row
    s += bytes([2, 9]) + bytes([0, 0]) + bytes([0, 4, 1, 2, 3, 4]) + bytes([0, 1])
    want[h - 1 - 3, 7:9] = 9
    want[h - 1 - 4, :4] = [1, 2, 3, 4]
    return w, h, bytes(s), want


# ---- files that break one rule each -----------------------------------------------------------------------------------
def broken_files():
    """-> ({name: bytes}, good): `good` is the readable 8-bit file most of them are made from"""
    pix = random_pixels(7, 5, 8, seed=3)
    pal = random_palette(256, seed=4)
    good = write(pix, 8, pal)
    off = struct.unpack_from("<I", good, 10)[0]
    assert off == 14 + 40 + 1024

    def patched(at, fmt, value, data=good):
        b = bytearray(data)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)
    out = {
        "payload_one_byte_short": good[:-1],
        "offbits_inside_the_palette": patched(10, "<I", off - 4),
        "offbits_beyond_the_file": patched(10, "<I", len(good) + 1),
        "palette_beyond_the_file": good[:14 + 40 + 1000],
        "clr_used_257": patched(46, "<I", 257),
        "planes_2": patched(26, "<H", 2),
        "bits_16": patched(28, "<H", 16),
        "bits_2": patched(28, "<H", 2),
        "width_0": patched(18, "<i", 0),
        "width_32768": patched(18, "<i", 32768),
        "height_0": patched(22, "<i", 0),
        "height_int_min": patched(22, "<i", -2 ** 31),
        "height_minus_32768": patched(22, "<i", -32768),
        "compression_4": patched(30, "<I", 4),
        "compression_5": patched(30, "<I", 5),
        "compression_6": patched(30, "<I", 6),
        "bitfields_at_8_bits": patched(30, "<I", 3),
        "header_size_41": patched(14, "<I", 41),
        "bm_and_six_bytes": b"BM" + bytes(6),
        "bm_and_the_file_header": good[:14],
        "header_cut": good[:14 + 39],
    }
    # the 12-byte core header (16-bit sizes, 3-byte palette entries) and the 64-byte OS/2 header
    core = struct.pack("<IHHHH", 12, 7, 5, 1, 8)
    out["core_header"] = b"BM" + struct.pack("<IHHI", 0, 0, 0, 14 + 12 + 768) + core + bytes(768) + pack_rows(pix, 8).tobytes()
    os2 = info_header(40, 7, 5, 8, 0, 0)[4:] + bytes(24)
    out["os2_header"] = b"BM" + struct.pack("<IHHI", 0, 0, 0, 14 + 64 + 1024) + struct.pack("<I", 64) + os2 + palette_bytes(pal) + pack_rows(pix, 8).tobytes()
    # RLE4; top-down RLE8; RLE8 at 4 bits
    stream = rle8_encode(pix)
    out["rle4"] = write_rle8(7, 5, stream, random_palette(16, 5), compression=2, bits=4)
    out["rle8_top_down"] = write_rle8(7, 5, stream, pal, top_down=True)
    out["rle8_at_4_bits"] = write_rle8(7, 5, stream, random_palette(16, 5), bits=4)
    # an encoded and an absolute run across the row end, a run above the top row, a delta out of the image, streams cut
    # before end-of-bitmap while rows are missing, an absolute run whose bytes the file does not hold
    out["rle8_run_across_the_row_end"] = write_rle8(7, 5, bytes([5, 1, 3, 2, 0, 1]), pal)
    out["rle8_absolute_run_across_the_row_end"] = write_rle8(7, 5, bytes([5, 1, 0, 3, 1, 2, 3, 0, 0, 1]), pal)
    out["rle8_run_above_the_top_row"] = write_rle8(7, 2, bytes([7, 1, 0, 0, 7, 2, 0, 0, 1, 3, 0, 1]), pal)
    out["rle8_delta_out_of_the_image"] = write_rle8(7, 5, bytes([0, 2, 8, 0, 0, 1]), pal)
    out["rle8_cut_before_end_of_bitmap"] = write_rle8(7, 5, stream[:8], pal)
    out["rle8_empty_stream"] = write_rle8(7, 5, b"", pal)
    out["rle8_absolute_run_cut"] = write_rle8(7, 1, bytes([0, 5, 1, 2]), pal)
    # 32 bits with other masks, behind a 40-byte header and inside a 108-byte one
    rgbx = random_pixels(5, 3, 32, seed=6)
    out["masks_bgr_behind_40"] = write(rgbx, 32, bitfields=True, masks=(0x000000FF, 0x0000FF00, 0x00FF0000))
    out["masks_565_inside_108"] = write(rgbx, 32, bitfields=True, header=108, masks=(0xF800, 0x07E0, 0x001F))
    out["masks_cut"] = write(rgbx, 32, bitfields=True)[:14 + 40 + 8]
    # 24 bits whose pixel array begins inside the header
    rgb = write(random_pixels(5, 3, 24, seed=7), 24)
    out["offbits_inside_the_header_24"] = patched(10, "<I", 30, rgb) + bytes(64)
    return out, good
