"""A PNG writer for the tests of the PNG device route (png_scanlines, Detector.png_reconstruct / read_pngs,
find_boards_files(png="device")): any colour type and depth the library reads, a chosen filter type per row, any number
of IDAT chunks -- and the pieces to assemble files that break a rule.  PNG is lossless: the array handed to the writer
is the yardstick for whatever reads the file back."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# (colour type, bits) of the eight pixel sizes the device route takes: bpp 1, 3, 2, 4 and 2, 6, 4, 8 bytes
TAKEN = [(0, 8), (2, 8), (4, 8), (6, 8), (0, 16), (2, 16), (4, 16), (6, 16)]


def bpp_of(color_type, bits):
    return CHANNELS[color_type] * bits // 8


def chunk(kind, data=b""):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def ihdr(width, height, bits, color_type, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, bits, color_type, 0, 0, interlace))


def idat_chunks(compressed, n):
    """The compressed stream cut into n IDAT chunks (the first n - 1 of equal length; chunks may be short)."""
    step = max(1, len(compressed) // n)
    cuts = [compressed[i * step:(i + 1) * step] for i in range(n - 1)] + [compressed[(n - 1) * step:]]
    return b"".join(chunk(b"IDAT", c) for c in cuts)


def random_image(width, height, color_type, bits, seed=0):
    """Smooth ramps plus noise (every predictor gets something to do), uint8 / uint16 [H, W] or [H, W, channels]."""
    rng = np.random.default_rng(seed)
    ch = CHANNELS[color_type]
    top = (1 << bits) - 1
    y, x = np.mgrid[0:height, 0:width]
    planes = [((x * (3 + k) + y * (5 - k)) * (top // 97) + rng.integers(0, top // 3 + 1, (height, width))) % (top + 1) for k in range(ch)]
    img = np.stack(planes, axis=-1).astype(np.uint8 if bits == 8 else np.uint16)
    return img[:, :, 0] if ch == 1 else img


def grey_of(img, color_type):
    """What the library makes of the image: the first channel, or (r*4899 + g*9617 + b*1868 + 8192) >> 14; alpha ignored."""
    if color_type == 0:
        return img
    if color_type == 4:
        return img[:, :, 0]
    v = img.astype(np.uint64)
    return ((v[:, :, 0] * 4899 + v[:, :, 1] * 9617 + v[:, :, 2] * 1868 + 8192) >> 14).astype(img.dtype)


def row_filters(height, filters):
    """filters: an int 0..4 (every row), "rotate" (row y: y % 5), ("random", seed), or a sequence (repeated)."""
    if isinstance(filters, int):
        return np.full(height, filters, np.int64)
    if isinstance(filters, str) and filters == "rotate":
        return np.arange(height) % 5
    if isinstance(filters, tuple) and filters[0] == "random":
        return np.random.default_rng(filters[1]).integers(0, 5, height)
    return np.resize(np.asarray(filters, np.int64), height)


def scanlines(img, color_type, bits, filters="rotate"):
    """-> uint8 [H, rowbytes + 1]: the filtered rows, each behind its filter byte, as they go into zlib."""
    h, w = img.shape[:2]
    bpp = bpp_of(color_type, bits)
    rows = np.frombuffer(np.ascontiguousarray(img).astype(">u2" if bits == 16 else np.uint8).tobytes(), np.uint8)
    rows = rows.reshape(h, w * bpp).astype(np.int32)
    fts = row_filters(h, filters)
    out = np.empty((h, w * bpp + 1), np.uint8)
    prev = np.zeros(w * bpp, np.int32)
    zeros = np.zeros(bpp, np.int32)
    for y in range(h):
        cur, ft = rows[y], int(fts[y])
        left = np.concatenate([zeros, cur[:-bpp]])[:w * bpp]
        upleft = np.concatenate([zeros, prev[:-bpp]])[:w * bpp]
        if ft == 0:
            pred = np.zeros_like(cur)
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (left + prev) >> 1
        else:
            p = left + prev - upleft
            pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
        out[y, 0] = ft
        out[y, 1:] = (cur - pred) & 0xff
        prev = cur
    return out


def assemble(width, height, bits, color_type, scan, nidat=1, level=6, palette=None):
    comp = zlib.compress(np.ascontiguousarray(scan).tobytes(), level)
    plte = chunk(b"PLTE", np.ascontiguousarray(palette, np.uint8).tobytes()) if palette is not None else b""
    return SIGNATURE + ihdr(width, height, bits, color_type) + plte + idat_chunks(comp, nidat) + chunk(b"IEND")


def encode(img, color_type, bits, filters="rotate", nidat=1, level=6, palette=None):
    """-> (the file's bytes, its filtered scanlines uint8 [H, rowbytes + 1]).  color_type 3: img holds palette indices
    (uint8 [H, W]) and `palette` uint8 [n, 3]."""
    scan = scanlines(img, color_type, bits, filters)
    h, w = img.shape[:2]
    return assemble(w, h, bits, color_type, scan, nidat, level, palette), scan


def write(path, img, color_type, bits, **kw):
    data, scan = encode(img, color_type, bits, **kw)
    with open(path, "wb") as f:
        f.write(data)
    return scan


def broken_files():
    """{name: bytes} of files that break one rule each (png_scanlines and read_image must both call them unreadable), all
    cut from one good 8-bit grey image of 9 x 7."""
    img = random_image(9, 7, 0, 8, seed=3)
    scan = scanlines(img, 0, 8, "rotate")
    comp = zlib.compress(scan.tobytes(), 6)
    good_idat = chunk(b"IDAT", comp)
    end = chunk(b"IEND")
    out = {}
    out["interlace"] = SIGNATURE + ihdr(9, 7, 8, 0, interlace=1) + good_idat + end
    out["depth4"] = SIGNATURE + ihdr(9, 7, 4, 0) + chunk(b"IDAT", zlib.compress(bytes((9 * 4 + 7) // 8 + 1) * 7)) + end
    bad = scan.copy()
    bad[4, 0] = 5
    out["filter5"] = assemble(9, 7, 8, 0, bad)
    out["truncated_idat"] = SIGNATURE + ihdr(9, 7, 8, 0) + chunk(b"IDAT", comp[:len(comp) // 2]) + end
    out["row_too_few"] = assemble(9, 7, 8, 0, scan[:6])
    out["row_too_many"] = assemble(9, 7, 8, 0, np.concatenate([scan, scan[:1]]))
    out["ihdr_not_first"] = SIGNATURE + chunk(b"tEXt", b"Comment\0first") + ihdr(9, 7, 8, 0) + good_idat + end
    out["two_ihdr"] = SIGNATURE + ihdr(9, 7, 8, 0) + ihdr(9, 7, 8, 0) + good_idat + end
    out["side_32768"] = SIGNATURE + ihdr(32768, 7, 8, 0) + good_idat + end
    return out, assemble(9, 7, 8, 0, scan), img
