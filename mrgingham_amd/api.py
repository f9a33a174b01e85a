"""Python face of the C-ABI.

Single-image functions mirror the reference module (names, arguments, error
behaviour: mrgingham_pywrap.c:40-112 ChESS_response_5, :128-212 find_points).
`Detector` is the batch interface over device-resident torch tensors.
"""
import contextlib
import ctypes
import os

import numpy as np

from . import _lib


def level_dims(width, height, level):
    """Size (w, h) of pyramid level `level` (find_chessboard_corners.cc:449-450)."""
    w, h = ctypes.c_int(), ctypes.c_int()
    if _lib.lib().mrgingham_amd_level_dims(width, height, level, ctypes.byref(w), ctypes.byref(h)) != 0:
        raise RuntimeError(f"Got an unreasonable image_pyramid_level = {level}")
    return w.value, h.value


def _require_device():
    """The C symbols can only report a missing device as "nothing found"; the Python face fails loudly."""
    if _lib.lib().mrgingham_amd_device_count() <= 0:
        raise RuntimeError("mrgingham_amd: no usable HIP device, and there is no CPU fallback")


def _check_image(image, exact_2d):
    image = np.asarray(image) if not isinstance(image, np.ndarray) else image
    # same checks, same messages as mrgingham_pywrap.c:53-68 / :163-178
    if exact_2d and image.ndim != 2:
        raise RuntimeError("The input image array must have exactly 2 dims (broadcasting not supported here); "
                           f"got {image.ndim}")
    if not exact_2d and image.ndim < 2:
        raise RuntimeError("The input image array must have at least 2 dims (extra ones will be broadcasted); "
                           f"got {image.ndim}")
    if image.dtype != np.uint8:
        raise RuntimeError("The input image array must contain 8-bit unsigned data")
    if image.shape[-1] > 1 and image.strides[-1] != 1:
        raise RuntimeError("Image rows must live in contiguous memory")
    return image


def ChESS_response_5(image):
    """int16 ChESS response, broadcasting over leading dims (mrgingham_pywrap.c:40-112).

    Like the reference, only the interior [7,W-7) x [7,H-7) of each slice is
    computed; the reference leaves the 7-pixel frame uninitialised, here it is 0.
    """
    image = _check_image(image, exact_2d=False)
    _require_device()
    L = _lib.lib()
    out = np.zeros(image.shape, dtype=np.int16)
    H, W = image.shape[-2:]
    lead = image.shape[:-2]
    for idx in np.ndindex(*lead):
        src = image[idx]
        dst = out[idx]
        stride = src.strides[0] if H > 1 else W
        L.mrgingham_ChESS_response_5(dst.ctypes.data, src.ctypes.data, W, H, stride)
    return out


def find_points(image, image_pyramid_level=0, blobs=False, debug=False):
    """Unordered corner candidates, float64 (N,2); (0,2) when none (mrgingham_pywrap.c:128-212)."""
    if blobs and image_pyramid_level != 0:
        raise RuntimeError("blob detector requires that image_pyramid_level == 0")
    image = _check_image(image, exact_2d=True)
    _require_device()
    result = []

    @_lib.ADD_POINTS_INT
    def add_points(xy, n, scale, cookie):  # add_points__find_points, mrgingham_pywrap.c:115-127
        a = np.ctypeslib.as_array(xy, shape=(2 * n,)).astype(np.float64)
        result.append((a * scale).reshape(n, 2))
        return True

    H, W = image.shape
    stride = image.strides[0] if H > 1 else W
    ok = _lib.lib().find_chessboard_corners_from_image_array_C(H, W, stride, image.ctypes.data,
                                                              int(image_pyramid_level), bool(blobs), bool(debug),
                                                              add_points, None)
    if not ok:
        if not result:
            return np.zeros((0, 2), dtype=np.float64)
        raise RuntimeError("find_chessboard_corners_from_image_array_C() failed")
    return result[0]


find_chessboard_corners = find_points  # compatibility alias, mrgingham_pywrap.c:365


def refine_points(points, levels, image, image_pyramid_level):
    """refine_chessboard_corners_from_image_array (find_chessboard_corners.hh:51-72):
    returns (points', levels', Nrefined); inputs are not modified."""
    image = _check_image(image, exact_2d=True)
    _require_device()
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2).copy()
    lv = np.ascontiguousarray(levels, dtype=np.int8).copy()
    assert len(lv) == len(pts)
    H, W = image.shape
    stride = image.strides[0] if H > 1 else W
    n = _lib.lib().refine_chessboard_corners_from_image_array_C(H, W, stride, image.ctypes.data, pts.ctypes.data,
                                                                lv.ctypes.data, len(lv), int(image_pyramid_level),
                                                                False)
    return pts, lv, n


def jpeg_coefficients(data):
    """Marker parse + Huffman decode of a baseline JPEG held in memory (host only): -> (coef int16 [bh, bw, 64], quant
    uint16 [64], (height, width)) -- the quantised luma coefficients, row-major inside a block, blocks in raster order and
    padded to whole MCUs, and the luma table in the same order (what Detector.jpeg_idct takes).  None when the data is
    not a JPEG this library reads (mrgingham_amd_jpeg_coefficients: progressive, arithmetic, multi-scan, malformed, ...)."""
    L = _lib.lib()
    buf = bytes(data)
    w, h, bw, bh = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    quant = np.zeros(64, dtype=np.uint16)
    sizes = (ctypes.byref(w), ctypes.byref(h), ctypes.byref(bw), ctypes.byref(bh))
    if L.mrgingham_amd_jpeg_coefficients(buf, len(buf), None, 0, quant.ctypes.data, *sizes) != 0:
        return None
    coef = np.empty((bh.value, bw.value, 64), dtype=np.int16)
    if L.mrgingham_amd_jpeg_coefficients(buf, len(buf), coef.ctypes.data, coef.size, quant.ctypes.data, *sizes) != 0:
        return None
    return coef, quant, (h.value, w.value)


def jpeg_coefficients_size(data):
    """(height, width) of a baseline JPEG held in memory, from its header alone; None when it is not one this library reads."""
    buf = bytes(data)
    w, h = ctypes.c_int(), ctypes.c_int()
    if _lib.lib().mrgingham_amd_jpeg_coefficients(buf, len(buf), None, 0, None, ctypes.byref(w), ctypes.byref(h), None, None) != 0:
        return None
    return h.value, w.value


def jpeg_restart_intervals(data):
    """The restart intervals of a baseline JPEG held in memory (host only; mrgingham_amd_jpeg_restart_intervals):
    -> (restart_interval, offsets int64 [n, 2]) -- MCUs per interval and the [begin, end) byte offsets of the
    n = ceil(MCUs / restart_interval) independent streams; (0, empty [0, 2]) for a file without a DRI segment; None when
    the file is not one this library reads."""
    L = _lib.lib()
    buf = bytes(data)
    ri, n = ctypes.c_int(), ctypes.c_size_t()
    if L.mrgingham_amd_jpeg_restart_intervals(buf, len(buf), ctypes.byref(ri), None, 0, ctypes.byref(n)) != 0:
        return None
    offsets = np.zeros((n.value, 2), dtype=np.int64)
    if L.mrgingham_amd_jpeg_restart_intervals(buf, len(buf), ctypes.byref(ri), offsets.ctypes.data, n.value, ctypes.byref(n)) != 0:
        return None
    return ri.value, offsets


def jpeg_sync_rounds(data, subsequence=128):
    """How the self-synchronising decoder of files without restart intervals fares on a baseline JPEG held in memory (host
    only; mrgingham_amd_jpeg_sync_rounds): the entropy-coded segment cut into subsequences of `subsequence` bytes (a
    multiple of 4 in 8..1024) -> (rounds, subsequences): the update rounds that change a record before the parallel decode
    equals the serial one -- the device takes the file iff that is at most option "jpeg_sync_max_rounds" -- and how many
    subsequences there are.  None when the file is not one this library reads; ValueError for a file that has restart
    intervals (the device decodes those one lane per interval), for one whose entropy-coded segment has 2^29 bytes or more
    (left to the host) and for a bad subsequence size."""
    subsequence = int(subsequence)
    if subsequence < 8 or subsequence > 1024 or subsequence % 4:
        raise ValueError("jpeg_sync_rounds: subsequence is a multiple of 4 in 8..1024")
    buf = bytes(data)
    rounds, n = ctypes.c_int(), ctypes.c_size_t()
    rc = _lib.lib().mrgingham_amd_jpeg_sync_rounds(buf, len(buf), subsequence, ctypes.byref(rounds), ctypes.byref(n))
    if rc == -3:
        raise ValueError("jpeg_sync_rounds: the file has restart intervals")
    if rc == -4:
        raise ValueError("jpeg_sync_rounds: an entropy-coded segment of 2^29 bytes or more is left to the host decoder")
    if rc != 0:
        return None
    return rounds.value, n.value


class _PngNotTaken:
    """What png_scanlines returns for a readable PNG that the device route leaves to read_image (a palette file)."""
    def __repr__(self):
        return "PNG_NOT_TAKEN"


PNG_NOT_TAKEN = _PngNotTaken()
_PNG_BPP = {(8, 0): 1, (8, 2): 3, (8, 4): 2, (8, 6): 4, (16, 0): 2, (16, 2): 6, (16, 4): 4, (16, 6): 8}


def png_scanlines(data):
    """Chunk walk + inflate of a PNG held in memory (host only; mrgingham_amd_png_scanlines): -> (scanlines uint8
    [height, rowbytes + 1], (height, width), bits, color_type) -- the FILTERED rows as they leave zlib, each behind its
    filter byte (0 .. 4), rowbytes = width * bpp; what Detector.png_reconstruct takes.  PNG_NOT_TAKEN for a readable file
    the device route does not take (colour type 3, palette: read_image decodes it).  None when the data is not a PNG this
    library reads (interlace, depths other than 8 / 16, chunk order, inflate errors, a filter byte above 4, ...)."""
    L = _lib.lib()
    buf = bytes(data)
    w, h, b, ct = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    sizes = (ctypes.byref(w), ctypes.byref(h), ctypes.byref(b), ctypes.byref(ct))
    rc = L.mrgingham_amd_png_scanlines(buf, len(buf), None, 0, *sizes)
    if rc == -3:
        return PNG_NOT_TAKEN
    if rc != 0:
        return None
    scan = np.empty((h.value, w.value * _PNG_BPP[b.value, ct.value] + 1), dtype=np.uint8)
    if L.mrgingham_amd_png_scanlines(buf, len(buf), scan.ctypes.data, scan.size, *sizes) != 0:
        return None
    return scan, (h.value, w.value), b.value, ct.value


def png_scanlines_size(data):
    """(height, width, bits, color_type) of a PNG held in memory from its chunks alone (nothing is inflated; palette files
    included); None when it is not one this library reads."""
    buf = bytes(data)
    w, h, b, ct = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = _lib.lib().mrgingham_amd_png_scanlines(buf, len(buf), None, 0, ctypes.byref(w), ctypes.byref(h), ctypes.byref(b), ctypes.byref(ct))
    if rc not in (0, -3):
        return None
    return h.value, w.value, b.value, ct.value


PGM_HEADER_CUT = -2   # pgm_header: the bytes end inside the header


def pgm_header(data):
    """The header of a binary PGM held in memory, whole or only its first bytes (mrgingham_amd_pgm_header; host only):
    (height, width, bits, payload_offset) -- the file is readable when it holds height*width*bits/8 bytes from
    payload_offset on --, None for what is not a PGM or breaks a rule, PGM_HEADER_CUT where the bytes end inside the
    header (of a whole file: unreadable; of a file's first bytes: more are needed)."""
    buf = bytes(data)
    w, h, b, off = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    rc = _lib.lib().mrgingham_amd_pgm_header(buf, len(buf), ctypes.byref(w), ctypes.byref(h), ctypes.byref(b), ctypes.byref(off))
    if rc == PGM_HEADER_CUT:
        return PGM_HEADER_CUT
    if rc != 0:
        return None
    return h.value, w.value, b.value, off.value


def png_reconstruct_geometry():
    """(rows_in_flight, segment_pixels) of the PNG reconstruction kernel's schedule (mrgingham_amd_png_reconstruct_geometry)."""
    r, s = ctypes.c_int(), ctypes.c_int()
    _lib.lib().mrgingham_amd_png_reconstruct_geometry(ctypes.byref(r), ctypes.byref(s))
    return r.value, s.value


class TiffLayout:
    """What tiff_layout found in a TIFF file: height, width, bits, samples, photometric, compression, predictor, big_endian;
    nstrips and strips, a structured array (offset, nbytes, first_row, rows) of the records that fitted the capacity;
    taken: the device route (Detector.tiff_decode) takes the file, False: read_image's decoder alone reads it; rc: the
    C call's return value (0, TIFF_NOT_TAKEN, or -2 where a given capacity was too small).  tile_width, tile_length: 0 for a
    strip file; for a tiled file (tiff_layout(tiles=True)) the tile sizes, and `strips` holds one record per tile, row-major,
    rows = tile_length each."""
    FIELDS = ("width", "height", "bits", "samples", "photometric", "compression", "predictor", "big_endian")

    def __init__(self, info, strips, nstrips, rc, tile_width=0, tile_length=0):
        for n in self.FIELDS:
            setattr(self, n, int(getattr(info, n)))
        self.strips, self.nstrips, self.rc, self.taken = strips, int(nstrips), int(rc), rc == 0
        self.tile_width, self.tile_length = int(tile_width), int(tile_length)

    def key(self):
        return tuple(getattr(self, n) for n in self.FIELDS)

    def __repr__(self):
        return "TiffLayout(" + ", ".join(f"{n}={getattr(self, n)}" for n in self.FIELDS) + f", nstrips={self.nstrips}, tile={self.tile_width}x{self.tile_length}, rc={self.rc})"


TIFF_NOT_TAKEN = -3
TIFF_STRIP = np.dtype([("offset", "<i8"), ("nbytes", "<i8"), ("first_row", "<i4"), ("rows", "<i4")])


def tiff_layout(data, lzw_max_strip=0, capacity=None, deflate_max_strip=0, tiles=False):
    """The first image file directory of a TIFF held in memory (host only; mrgingham_amd_tiff_layout, which has the subset
    this library reads): -> TiffLayout, or None when the data is not a TIFF this library reads.  lzw_max_strip: the decoded
    bytes of an LZW strip above which the file is left to the host decoder (0: 1 MiB).  capacity: room for that many
    strip records (default: all of them); with fewer than the file has, rc is -2 and the counts are still reported.
    deflate_max_strip: above 0, Deflate files whose strips decode to at most that many bytes are taken as well
    (mrgingham_amd_tiff_layout_ex); 0: they are left to the host decoder.  tiles=True: tiled files are read as well
    (mrgingham_amd_tiff_layout_tiled: one record per tile, tile_width and tile_length in the result; taken with a tile width
    that is a multiple of 16); False: a file with any tile tag gives None, as before."""
    L = _lib.lib()
    buf = bytes(data)
    info, n = _lib.TiffInfo(), ctypes.c_size_t()
    tw, tl = ctypes.c_int32(), ctypes.c_int32()

    def call(strips, cap):
        if tiles:
            return L.mrgingham_amd_tiff_layout_tiled(buf, len(buf), int(lzw_max_strip), int(deflate_max_strip), ctypes.byref(info),
                                                     ctypes.byref(tw), ctypes.byref(tl), strips, cap, ctypes.byref(n))
        if int(deflate_max_strip) > 0:
            return L.mrgingham_amd_tiff_layout_ex(buf, len(buf), int(lzw_max_strip), int(deflate_max_strip), ctypes.byref(info), strips, cap,
                                                  ctypes.byref(n))
        return L.mrgingham_amd_tiff_layout(buf, len(buf), int(lzw_max_strip), ctypes.byref(info), strips, cap, ctypes.byref(n))
    rc = call(None, 0)
    if rc not in (0, TIFF_NOT_TAKEN):
        return None
    cap = n.value if capacity is None else int(capacity)
    strips = np.zeros(cap, dtype=TIFF_STRIP)
    rc = call(strips.ctypes.data if cap else None, cap)
    if cap == 0 and n.value > 0 and capacity is not None:
        rc = -2   # (no array to write into is "counts only" at the C boundary)
    if rc not in (0, TIFF_NOT_TAKEN, -2):
        return None
    return TiffLayout(info, strips[:min(cap, n.value)], n.value, rc, tw.value, tl.value)


def tiff_geometry():
    """(lzw_lanes, segment_pixels, step_pixels) of the TIFF kernels' schedules (mrgingham_amd_tiff_geometry): the lanes in
    flight of the LZW launch, the pixels of a row a lane of the finish kernel takes and the pixels a wave takes per step."""
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.lib().mrgingham_amd_tiff_geometry(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value


BMP_NOT_TAKEN = -3


class BmpLayout:
    """What bmp_layout found in a Windows Bitmap: height, width, bits (1, 4, 8, 24, 32), compression (0, 1 RLE8, 3 the one
    set of masks), top_down, payload_offset, row_bytes, lut (uint8 [256]: the grey of every palette index, 0 where the
    file defines none), lut_identity; taken: the device route (Detector.bmp_unpack) takes the file, False: read_image's
    decoder alone reads it (RLE8); rc: the C call's return value (0 or BMP_NOT_TAKEN)."""
    FIELDS = ("width", "height", "bits", "compression", "top_down", "row_bytes", "payload_offset", "lut_identity")

    def __init__(self, info, rc):
        for n in self.FIELDS:
            setattr(self, n, int(getattr(info, n)))
        self.lut = np.frombuffer(bytes(info.lut), np.uint8).copy()
        self.rc, self.taken = int(rc), rc == 0

    def __repr__(self):
        return "BmpLayout(" + ", ".join(f"{n}={getattr(self, n)}" for n in self.FIELDS) + f", rc={self.rc})"


def bmp_layout(data):
    """The headers and the palette of a Windows Bitmap held in memory, whole (host only; mrgingham_amd_bmp_layout, which has
    the subset this library reads): -> BmpLayout, or None when the data is not a BMP this library reads."""
    buf = bytes(data)
    info = _lib.BmpInfo()
    rc = _lib.lib().mrgingham_amd_bmp_layout(buf, len(buf), ctypes.byref(info))
    if rc not in (0, BMP_NOT_TAKEN):
        return None
    return BmpLayout(info, rc)


def bmp_unpack_geometry():
    """(lanes_per_workgroup, max_workgroups_per_cu) of the BMP unpack launch (mrgingham_amd_bmp_unpack_geometry)."""
    a, b = ctypes.c_int(), ctypes.c_int()
    _lib.lib().mrgingham_amd_bmp_unpack_geometry(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


class PnmHeader:
    """What pnm_header found in a binary Netpbm header: height, width, bits of a sample in the file (1 for P4, 8, 16),
    channels (samples per pixel, 1 .. 4), black_and_white, magic (the digit: 4 .. 7), row_bytes, payload_offset; depth: of
    the grey read_image gives (8, or 16 for 16-bit samples)."""
    FIELDS = ("width", "height", "bits", "channels", "black_and_white", "magic", "row_bytes", "payload_offset")

    def __init__(self, info):
        for n in self.FIELDS:
            setattr(self, n, int(getattr(info, n)))
        self.depth = 16 if self.bits == 16 else 8

    def __repr__(self):
        return "PnmHeader(" + ", ".join(f"{n}={getattr(self, n)}" for n in self.FIELDS) + ")"


def pnm_header(data):
    """The header of a binary Netpbm file (P4, P5, P7; P6 is not read) held in memory, whole or only its first bytes
    (mrgingham_amd_pnm_header, which has the subset this library reads; host only): -> PnmHeader; None for what is not such
    a file, breaks a rule or -- P4, P7 -- holds less than its header promises; PGM_HEADER_CUT where the bytes end inside
    the header (of a whole file: unreadable; of a file's first bytes: more are needed).  A P5 header gets pgm_header's
    verdict: its payload is not measured."""
    buf = bytes(data)
    info = _lib.PnmInfo()
    rc = _lib.lib().mrgingham_amd_pnm_header(buf, len(buf), ctypes.byref(info))
    if rc == PGM_HEADER_CUT:
        return PGM_HEADER_CUT
    if rc != 0:
        return None
    return PnmHeader(info)


def pnm_unpack_geometry():
    """(lanes_per_workgroup, max_workgroups_per_cu) of the Netpbm unpack launch (mrgingham_amd_pnm_unpack_geometry)."""
    a, b = ctypes.c_int(), ctypes.c_int()
    _lib.lib().mrgingham_amd_pnm_unpack_geometry(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


# the packed camera formats (MRGINGHAM_AMD_RAW_*): GenICam Mono10p / Mono12p / Mono14p, GigE Vision Mono10Packed / Mono12Packed
RAW_FORMATS = {"p10": 0, "p12": 1, "p14": 2, "gev10": 3, "gev12": 4}


def _raw_format(fmt, who):
    if not isinstance(fmt, str) or fmt not in RAW_FORMATS:
        raise ValueError(f'{who}: fmt is one of "p10", "p12", "p14", "gev10", "gev12"')
    return RAW_FORMATS[fmt]


def raw_row_bytes(width, fmt):
    """The fewest bytes that hold a row of `width` packed samples (mrgingham_amd_raw_row_bytes): ceil(width*N/8) for the
    bit streams "p10", "p12", "p14", 3*ceil(width/2) for the pixel pairs "gev10", "gev12".  width 1 .. 32767."""
    n = _lib.lib().mrgingham_amd_raw_row_bytes(int(width), _raw_format(fmt, "raw_row_bytes"))
    if n < 0:
        raise ValueError("raw_row_bytes: width 1 .. 32767")
    return int(n)


def raw_unpack(data, height, width, fmt, row_bytes=None):
    """One packed 10 / 12 / 14-bit camera frame to np.uint16 [height, width] on the host (mrgingham_amd_raw_unpack_image,
    no device needed): data is bytes or a uint8 array, row y begins at byte y*row_bytes (None: raw_row_bytes(width, fmt)),
    the values are the samples as they are, 0 .. 2^N - 1.  Detector.raw_unpack is the device's route for batches."""
    f = _raw_format(fmt, "raw_unpack")
    buf = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data)
    if buf.dtype != np.uint8:
        raise ValueError("raw_unpack: data is bytes or a uint8 array")
    rowb = raw_row_bytes(width, fmt) if row_bytes is None else int(row_bytes)
    if not (1 <= height <= 32767):
        raise ValueError("raw_unpack: height 1 .. 32767")
    out = np.empty((height, width), dtype=np.uint16)
    if _lib.lib().mrgingham_amd_raw_unpack_image(buf.ctypes.data, buf.size, int(width), int(height), rowb, f, out.ctypes.data, int(width)) != 0:
        raise ValueError("raw_unpack: row_bytes is at least raw_row_bytes(width, fmt) and data holds (height-1)*row_bytes + raw_row_bytes(width, fmt) bytes")
    return out


def raw_unpack_geometry():
    """(lanes_per_workgroup, max_workgroups_per_cu) of the packed-frame unpack launch (mrgingham_amd_raw_unpack_geometry)."""
    a, b = ctypes.c_int(), ctypes.c_int()
    _lib.lib().mrgingham_amd_raw_unpack_geometry(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


# the Bayer patterns (MRGINGHAM_AMD_BAYER_*): the colours of pixels (0,0), (0,1), (1,0), (1,1); GenICam BayerRG / GR / GB / BG
BAYER_PATTERNS = {"rggb": 0, "grbg": 1, "gbrg": 2, "bggr": 3}


def _bayer_pattern(pattern, who):
    if not isinstance(pattern, str) or pattern not in BAYER_PATTERNS:
        raise ValueError(f'{who}: pattern is one of "rggb", "grbg", "gbrg", "bggr"')
    return BAYER_PATTERNS[pattern]


def bayer_grey(image, pattern):
    """One Bayer mosaic to grey on the host (mrgingham_amd_bayer_grey_image, no device needed): image np.uint8 or np.uint16
    [H, W], sides 2 .. 32767 -> the same dtype and shape: bilinear demosaicing and the luma 4899 R + 9617 G + 1868 B over
    16384 in one rounding, borders by reflect-101 (include/mrgingham_amd.h has the definition).  Detector.bayer_grey is
    the device's route for batches."""
    p = _bayer_pattern(pattern, "bayer_grey")
    image = np.asarray(image)
    if image.dtype not in (np.uint8, np.uint16) or image.ndim != 2:
        raise ValueError("bayer_grey: image is a uint8 or uint16 [H,W] array")
    image = np.ascontiguousarray(image)
    H, W = image.shape
    out = np.empty((H, W), dtype=image.dtype)
    if _lib.lib().mrgingham_amd_bayer_grey_image(image.ctypes.data, 8 * image.itemsize, W, H, W, p, out.ctypes.data, W) != 0:
        raise ValueError("bayer_grey: sides 2 .. 32767")
    return out


def bayer_grey_geometry():
    """(lanes_per_workgroup, rows_per_slab, max_workgroups_per_cu) of the Bayer launch (mrgingham_amd_bayer_grey_geometry);
    the last is 0: the grid is not capped."""
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.lib().mrgingham_amd_bayer_grey_geometry(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value


# the colour formats (MRGINGHAM_AMD_COLOUR_*): interleaved with 3 or 4 samples per pixel, three planes, packed YUV 4:2:2
COLOUR_FORMATS = {"rgb": 0, "bgr": 1, "rgba": 2, "bgra": 3, "rgb_planar": 4, "bgr_planar": 5, "yuyv": 6, "uyvy": 7}
# the samples of a pixel along the last axis of a frame (the planar formats: 1, the three planes lie on an axis of their own)
_COLOUR_SAMPLES = {0: 3, 1: 3, 2: 4, 3: 4, 4: 1, 5: 1, 6: 2, 7: 2}


def _colour_format(format, who):
    if not isinstance(format, str) or format not in COLOUR_FORMATS:
        raise ValueError(f'{who}: format is one of "rgb", "bgr", "rgba", "bgra", "rgb_planar", "bgr_planar", "yuyv", "uyvy"')
    return COLOUR_FORMATS[format]


def colour_grey(image, format):
    """One colour frame to grey on the host (mrgingham_amd_colour_grey_image, no device needed): image np.uint8 or np.uint16
    [H, W, C] with C = 3 ("rgb", "bgr"), 4 ("rgba", "bgra": the fourth sample is ignored) or 2 ("yuyv", "uyvy": uint8 only,
    the Y byte as it is), or [3, H, W] for "rgb_planar" and "bgr_planar"; sides 1 .. 32767 -> [H, W] of the same dtype:
    (4899 R + 9617 G + 1868 B + 8192) >> 14, the grey of the colour file readers (include/mrgingham_amd.h has the
    definition).  Detector.colour_grey is the device's route for batches."""
    f = _colour_format(format, "colour_grey")
    image = np.asarray(image)
    C = _COLOUR_SAMPLES[f]
    planar = C == 1
    if (image.dtype not in (np.uint8, np.uint16) or image.ndim != 3 or (image.shape[0] if planar else image.shape[2]) != (3 if planar else C)
            or (f >= 6 and image.dtype != np.uint8)):
        raise ValueError("colour_grey: image is a uint8 or uint16 [H,W,C] array with C = 3, 4, or 2 (4:2:2, uint8), or [3,H,W] for the planar formats")
    image = np.ascontiguousarray(image)
    H, W = image.shape[1:] if planar else image.shape[:2]
    out = np.empty((H, W), dtype=image.dtype)
    if _lib.lib().mrgingham_amd_colour_grey_image(image.ctypes.data, 8 * image.itemsize, f, W, H, C * W, H * W, out.ctypes.data, W) != 0:
        raise ValueError("colour_grey: sides 1 .. 32767")
    return out


def colour_grey_geometry():
    """(lanes_per_workgroup, max_workgroups_per_cu) of the colour launch (mrgingham_amd_colour_grey_geometry)."""
    a, b = ctypes.c_int(), ctypes.c_int()
    _lib.lib().mrgingham_amd_colour_grey_geometry(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def read_image(filename, cli_scaling=False):
    """Decode a binary PGM, non-interlaced PNG, baseline JPEG, strip or tiled TIFF (uncompressed, LZW, PackBits, Deflate; grey or
    RGB, 8 or 16 bit), Windows Bitmap (1, 4, 8 bit palette, RLE8, 24 and 32 bit; bmp_layout has the subset) or binary PBM or PAM
    (pnm_header has the subset; ASCII Netpbm and P6 are not read) to uint8 [H, W]
    with the library's own decoder (host only).
    16-bit files: the high byte (cv::imread(IMREAD_GRAYSCALE)) or, with cli_scaling, the CLI's
    convertTo(255/65535).  None when the file is unreadable, unsupported or malformed."""
    L = _lib.lib()
    w, h, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    name = os.fsencode(filename)
    if L.mrgingham_amd_read_image(name, int(bool(cli_scaling)), None, 0, ctypes.byref(w), ctypes.byref(h),
                                  ctypes.byref(d)) != 0:
        return None
    out = np.empty((h.value, w.value), dtype=np.uint8)
    if L.mrgingham_amd_read_image(name, int(bool(cli_scaling)), out.ctypes.data, out.size, ctypes.byref(w),
                                  ctypes.byref(h), ctypes.byref(d)) != 0:
        return None
    return out


# probe_image's kinds (MRGINGHAM_AMD_KIND_* of include/mrgingham_amd.h)
KIND_PGM, KIND_PNG, KIND_JPEG, KIND_TIFF, KIND_BMP, KIND_PNM = 1, 2, 3, 4, 5, 6


def probe_image(filename):
    """What read_image would produce for the file, from its header alone (mrgingham_amd_probe_image; host only, nothing is
    decoded): (height, width, bits, kind) with kind KIND_PGM binary PGM, KIND_PNG, KIND_JPEG baseline JPEG, KIND_TIFF, KIND_BMP
    (always 8 bits: the grey read_image gives; the stream of an RLE8 file is walked), KIND_PNM binary PBM or PAM (8 bits for
    PBM); None for a file that is unreadable at header level."""
    w, h, b, k = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if _lib.lib().mrgingham_amd_probe_image(os.fsencode(filename), ctypes.byref(w), ctypes.byref(h), ctypes.byref(b),
                                            ctypes.byref(k)) != 0:
        return None
    return h.value, w.value, b.value, k.value


def files_plan(keys, batch):
    """How find_boards_files cuts a list into chunks (mrgingham_amd_files_plan; host only): keys int32 [n], files of equal
    key >= 0 can share a chunk, key < 0 is not batched -> (chunk_of_file int32 [n], slot_in_chunk int32 [n], nchunks);
    -1 / -1 for the files that are not batched."""
    keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1)
    chunk = np.empty(keys.shape, dtype=np.int32)
    slot = np.empty(keys.shape, dtype=np.int32)
    n = ctypes.c_int32()
    if _lib.lib().mrgingham_amd_files_plan(keys.ctypes.data, len(keys), int(batch), chunk.ctypes.data, slot.ctypes.data,
                                           ctypes.byref(n)) != 0:
        raise ValueError("files_plan: batch must be at least 1")
    return chunk, slot, n.value


FILES_STATS = ("chunks", "files_device_loader", "files_host_decoded", "files_one_image", "files_unreadable",
               "ms_detector_waited_for_chunk", "ms_loader_waited_for_slot")


def find_boards_files(paths, gridn=10, image_pyramid_level=-1, clahe=True, blur_radius=1, refine=True, batch=64, nthreads=0,
                      entropy="host", device=None, progress=None, png="host", deep="one", tiff="host",
                      tiff_deflate="host", bmp="host", pnm="host"):
    """A list of image files (binary PGM, PBM and PAM, PNG, baseline JPEG, TIFF, BMP; any sizes) to boards (mrgingham_amd_find_boards_files): a
    loader thread fills chunks of `batch` equally-sized frames on the device -- JPEG through the batch loader,
    entropy="device": Huffman-decoded on the device as well -- while the calling thread preprocesses and searches the
    chunks before them.  Per file the same numbers as read_image + the one-image path with the same options.
    -> (boards float64 [n, gridn*gridn, 2], NaN where no board was found; levels int8 [n, gridn*gridn], the pyramid
    level every corner ended at; found int8 [n], the level the board was found at or -1; status int32 [n], 0 processed,
    -1 unreadable; stats dict, FILES_STATS).  progress(nfinal, boards, levels, found, status) is called from this thread
    with non-decreasing values of nfinal and the arrays the call is going to return: their entries [0, nfinal) are final,
    the last call passes n.  device None: the calling thread's device.  png="device": the runs of 8-bit PNG files of a chunk
    go through the PNG batch loader (Detector.read_pngs: the host threads only inflate) and count as files_device_loader;
    same numbers.  deep="one": 16-bit files go one at a time through the one-image path on this thread; deep="chunks":
    16-bit PGM and PNG files of one size share chunks of their own -- PGM through Detector.read_pgms (files_device_loader),
    PNG through the PNG batch loader with png="device", else decoded on the loader's host threads (files_host_decoded) --
    and are preprocessed at 16 bit a chunk at a time; same numbers.  TIFF files behave as PNG files do: 8-bit files share
    chunks and are decoded on the loader's host threads, 16-bit files follow `deep`; tiff="device": the runs of TIFF files
    of a chunk go through the TIFF batch loader (Detector.read_tiffs: the host threads only read the files, LZW strips are
    decoded one lane each) and count as files_device_loader; same numbers.  tiff_deflate="device", with tiff="device" only:
    the Deflate strips of those files are decoded on the device as well, else the loader's host threads inflate them.
    BMP files behave as 8-bit PGM files do: they share chunks and are decoded on the loader's host threads
    (files_host_decoded); bmp="device": the runs of BMP files of a chunk go through the BMP batch loader (Detector.read_bmps:
    the host threads only read the files, the device unpacks the pixel arrays) and count as files_device_loader; same
    numbers.
    Binary PBM and PAM files behave as PGM files do: 8-bit ones share chunks and are decoded on the loader's host threads
    (files_host_decoded), 16-bit ones follow `deep`; pnm="device": the runs of such files of a chunk go through the Netpbm
    batch loader (Detector.read_pnms: the host threads only read the files, the device unpacks the rasters) and count as
    files_device_loader; same numbers.  PGM files keep their routes."""
    if pnm not in ("host", "device"):
        raise ValueError('find_boards_files: pnm is "host" or "device"')
    if bmp not in ("host", "device"):
        raise ValueError('find_boards_files: bmp is "host" or "device"')
    if tiff not in ("host", "device"):
        raise ValueError('find_boards_files: tiff is "host" or "device"')
    if tiff_deflate not in ("host", "device") or (tiff_deflate == "device" and tiff != "device"):
        raise ValueError('find_boards_files: tiff_deflate is "host" or "device", "device" only with tiff="device"')
    if entropy not in ("host", "device"):
        raise ValueError('find_boards_files: entropy is "host" or "device"')
    if png not in ("host", "device"):
        raise ValueError('find_boards_files: png is "host" or "device"')
    if deep not in ("one", "chunks"):
        raise ValueError('find_boards_files: deep is "one" or "chunks"')
    _require_device()
    L = _lib.lib()
    names = [os.fsencode(p) for p in paths]
    n, N = len(names), int(gridn) * int(gridn)
    boards = np.full((n, N, 2), np.nan, dtype=np.float64)
    levels = np.zeros((n, N), dtype=np.int8)
    found = np.full((n,), -1, dtype=np.int8)
    status = np.full((n,), -1, dtype=np.int32)
    stats = np.zeros(len(FILES_STATS), dtype=np.float64)
    o = _lib.FilesOptions(int(bool(clahe)), int(blur_radius), int(gridn), int(image_pyramid_level), int(bool(refine)), int(batch),
                          int(nthreads), int(entropy == "device"), -1 if device is None else int(device))
    raised = []

    def on_progress(nfinal, cookie):
        if progress is not None and not raised:
            try:
                progress(nfinal, boards, levels, found, status)
            except BaseException as e:   # (an exception cannot cross the C frames: it is raised after the call)
                raised.append(e)
    cb = _lib.PROGRESS_F(on_progress)
    arr = (ctypes.c_char_p * max(n, 1))(*names)
    rc = L.mrgingham_amd_find_boards_files_ex5(arr, n, ctypes.byref(o), boards.ctypes.data, levels.ctypes.data, found.ctypes.data,
                                               status.ctypes.data, cb, None, stats.ctypes.data, len(stats),
                                               int(png == "device") | 2 * int(deep == "chunks") | 4 * int(tiff == "device") |
                                               8 * int(tiff_deflate == "device") | 16 * int(bmp == "device") | 32 * int(pnm == "device"))
    if raised:
        raise raised[0]
    if rc == -1:
        raise ValueError("find_boards_files: bad argument (gridn >= 2, image_pyramid_level <= 10, blur_radius 0..64, an existing device)")
    if rc != 0:
        e = RuntimeError(f"mrgingham_amd_find_boards_files failed: {rc}")
        e.code = rc
        raise e
    return boards, levels, found, status, dict(zip(FILES_STATS, stats.tolist()))


def set_wait_policy(policy):
    """How this process's threads wait for the device: 0 runtime default, 1 spin, 2 yield, 3 block
    (mrgingham_amd_set_wait_policy; before the first context -- inside a PyTorch process the runtime is usually
    running already and refuses)."""
    return _lib.lib().mrgingham_amd_set_wait_policy(int(policy))


def device_for_thread(thread_index, ndevices, env_value=None):
    """The library's policy for the device of the k-th thread that calls a reference symbol (include/mrgingham_amd.h,
    "several GPUs"): MRGINGHAM_AMD_DEVICE if set, else k modulo the number of devices.  Host only."""
    env = None if env_value is None else str(env_value).encode()
    return _lib.lib().mrgingham_amd_device_for_thread(int(thread_index), int(ndevices), env)


def shard_range(total, k, n):
    """(first, count) of shard k of n over `total` frames (mrgingham_amd_shard_range).  Host only."""
    a, b = ctypes.c_int(), ctypes.c_int()
    if _lib.lib().mrgingham_amd_shard_range(int(total), int(k), int(n), ctypes.byref(a), ctypes.byref(b)) != 0:
        raise ValueError("bad shard arguments")
    return a.value, b.value


def set_thread_device(device):
    """The calling thread's single-image calls (ChESS_response_5, find_points, find_board ...) run on this device."""
    if _lib.lib().mrgingham_amd_set_thread_device(int(device)) != 0:
        raise ValueError(f"no such device: {device}")


def thread_device():
    """Device of the calling thread's context (created on first use: see device_for_thread); -1 without a device."""
    return _lib.lib().mrgingham_amd_thread_device()


class PinnedArray:
    """A numpy array over page-locked host memory (mrgingham_amd_host_alloc): a frame handed to find_points /
    find_board / ChESS_response_5 out of it is uploaded at the speed of the link, with no pinning on the fly.
    Keep the object alive as long as `.array` is in use."""

    def __init__(self, shape, dtype=np.uint8):
        self._L = _lib.lib()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = self._L.mrgingham_amd_host_alloc(max(n, 1))
        if not self._p:
            raise RuntimeError("mrgingham_amd_host_alloc failed (no device?)")
        buf = (ctypes.c_char * max(n, 1)).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            self._L.mrgingham_amd_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chain_multi(detectors, shards, start_level=3, max_points=1024, sync=True):
    """mrgingham_amd_chain_multi: Detector k (its own device, or several on one) takes shards[k], a uint8 tensor
    [B_k, H, W] on that device; -> (points f64 [sum B, P, 2], levels int8 [sum B, P], npoints int32 [sum B]) on the
    FIRST detector's device, shard after shard -- one call, one gather."""
    import torch
    assert len(detectors) == len(shards) and len(detectors) > 0
    L = _lib.lib()
    root = detectors[0]
    frs = (_lib.Frames * len(shards))()
    total = 0
    for k, (d, fr) in enumerate(zip(detectors, shards)):
        assert fr.device == d.device, "every shard must live on its detector's device"
        f, B, H, W = d._frames(fr)
        frs[k] = f
        total += B
        torch.cuda.current_stream(fr.device).synchronize()
    P = int(max_points)
    pts = torch.empty((total, P, 2), dtype=torch.float64, device=root.device)
    lv = torch.empty((total, P), dtype=torch.int8, device=root.device)
    npts = torch.empty((total,), dtype=torch.int32, device=root.device)
    torch.cuda.current_stream(root.device).synchronize()
    ctxs = (ctypes.c_void_p * len(detectors))(*[d.ctx for d in detectors])
    for attempt in range(4):
        root._check(L.mrgingham_amd_chain_multi(ctxs, len(detectors), frs, int(start_level), pts.data_ptr(), lv.data_ptr(),
                                                npts.data_ptr(), P))
        if not sync:
            break
        rc = L.mrgingham_amd_sync_multi(ctxs, len(detectors))
        if rc == 0:
            break
        if rc != Detector.ERR_CAPACITY or attempt == 3:     # (the tables have grown: the same call again)
            root._check(rc)
    return pts, lv, npts


def find_grid_from_points(points_scaled, gridn=10):
    """mrgingham::find_grid_from_points (find_grid.cc:1216-1445), host only: int (N,2) candidates
    (pixel coordinates * 1000) -> float64 (gridn*gridn, 2) corners in board order, or None."""
    pts = np.ascontiguousarray(points_scaled, dtype=np.int32).reshape(-1, 2)
    out = np.empty((gridn * gridn, 2), dtype=np.float64)
    ok = _lib.lib().mrgingham_amd_find_grid_from_points(pts.ctypes.data, len(pts), int(gridn), out.ctypes.data)
    return out if ok else None


def find_grid_from_points_traced(points_scaled, gridn=10, debug_sequence=(-1, -1), debug=False):
    """find_grid_from_points with the reference's debug arguments: `debug` writes the /tmp/mrgingham-[2-6]-* vnlog
    dumps and reports progress on stderr; debug_sequence = (x, y) >= 0 traces the sequences from the candidate
    nearest to that pixel on stderr."""
    pts = np.ascontiguousarray(points_scaled, dtype=np.int32).reshape(-1, 2)
    out = np.empty((gridn * gridn, 2), dtype=np.float64)
    ok = _lib.lib().mrgingham_amd_find_grid_from_points_traced(pts.ctypes.data, len(pts), int(gridn), out.ctypes.data,
                                                              int(bool(debug)), int(debug_sequence[0]),
                                                              int(debug_sequence[1]))
    return out if ok else None


def find_grid_from_points_perturbed(points_scaled, gridn=10, ring_seed=0, last_match=False, canonical_start=False):
    """Test hook: find_grid_from_points with the neighbour-ring start of every site randomised (ring_seed != 0)
    and / or the last instead of the first matching neighbour taken along a sequence.  canonical_start: every
    site's ring starts at its first neighbour counter-clockwise from +x (ring_seed then rotates it from there),
    the rule of the stand-in Voronoi diagram that the parity tests run upstream's find_grid.cc on."""
    pts = np.ascontiguousarray(points_scaled, dtype=np.int32).reshape(-1, 2)
    out = np.empty((gridn * gridn, 2), dtype=np.float64)
    ok = _lib.lib().mrgingham_amd_find_grid_from_points_perturbed(pts.ctypes.data, len(pts), int(gridn),
                                                                 out.ctypes.data, int(ring_seed),
                                                                 int(bool(last_match)) | (int(bool(canonical_start)) << 1))
    return out if ok else None


# statuses below 0 of the device grid finder and its host model: the list is the host finder's (include/mrgingham_amd.h)
GRID_DECLINES = {-1: "count", -2: "ring", -3: "guard", -4: "table", -5: "coordinate"}


def find_grids_host(xy, counts, gridn=10, guard_bits=33):
    """The host model of the device grid finder (mrgingham_amd_find_grids_host; no device): candidate lists xy int32
    [nlists, capacity, 2] (pixel coordinates * 1000) with counts int32 [nlists] -> (index int32 [nlists, gridn * gridn]
    candidate indices in board order, -1 where there is no board; status int32 [nlists]: 1 board, 0 none, below 0
    declined, GRID_DECLINES).  It answers what Detector.find_grids answers, list for list."""
    xy = np.ascontiguousarray(xy, dtype=np.int32)
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if xy.ndim != 3 or xy.shape[2] != 2 or xy.shape[0] != len(counts):
        raise ValueError("find_grids_host: xy is [nlists, capacity, 2], counts is [nlists]")
    nlists, capacity = xy.shape[0], xy.shape[1]
    index = np.full((nlists, gridn * gridn), -1, dtype=np.int32)
    status = np.zeros((nlists,), dtype=np.int32)
    rc = _lib.lib().mrgingham_amd_find_grids_host(xy.ctypes.data, counts.ctypes.data, nlists, capacity, int(gridn), int(guard_bits),
                                                  index.ctypes.data, status.ctypes.data)
    if rc != 0:
        raise ValueError("find_grids_host: gridn 2 .. 16, guard_bits 8 .. 45")
    return index, status


def find_grids_geometry():
    """mrgingham_amd_find_grids_geometry as a dict: the caps of the device grid finder."""
    v = [ctypes.c_int() for _ in range(5)]
    b = ctypes.c_int64()
    _lib.lib().mrgingham_amd_find_grids_geometry(*[ctypes.byref(x) for x in v], ctypes.byref(b))
    names = ("lanes_per_workgroup", "max_candidates", "min_gridn", "max_gridn", "max_workgroups")
    return dict(zip(names, (x.value for x in v)), scratch_bytes_per_workgroup=b.value)


def boards_of_indices(xy, index, status):
    """What find_grids / find_grids_host answered, as corners: float64 [nlists, gridn * gridn, 2] = xy[index] / 1000.0
    (find_grid.cc:353-354) where status is 1, NaN rows elsewhere.  numpy arrays, or torch tensors (copied to the host)."""
    xy, index, status = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (xy, index, status))
    boards = np.full(index.shape + (2,), np.nan, dtype=np.float64)
    for l in np.nonzero(status == 1)[0]:
        boards[l] = xy[l][index[l]].astype(np.float64) / 1000.0
    return boards


def preprocess(image, clahe=True, blur_radius=1):
    """The CLI's preprocessing of an 8-bit image on the GPU (mrgingham-from-image.cc:71-111; the cv2
    recipe of find_board.docstring:8-10): normalize + CLAHE(8) when `clahe`, then a box blur of
    `blur_radius` (0 = none).  -> uint8 [H, W]."""
    _require_device()
    image = _check_image(image, exact_2d=True)
    H, W = image.shape
    out = np.empty((H, W), dtype=np.uint8)
    L = _lib.lib()
    L.mrgingham_amd_preprocess_image.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_void_p]
    rc = L.mrgingham_amd_preprocess_image(image.ctypes.data, W, H, image.strides[0], int(bool(clahe)), int(blur_radius),
                                          out.ctypes.data)
    if rc != 0:
        raise RuntimeError("mrgingham_amd: preprocessing failed (bad arguments or no device)")
    return out


def preprocess16(image16, clahe=True, blur_radius=1):
    """The CLI's preprocessing of a 16-bit image on the GPU (mrgingham-from-image.cc:85-111): normalize to
    0..65535 and CLAHE(8) on 16 bits when `clahe`, convertTo 8 bit with 255/65535, box blur.  -> uint8 [H, W]."""
    _require_device()
    image16 = np.ascontiguousarray(image16)
    if image16.dtype != np.uint16 or image16.ndim != 2:
        raise RuntimeError("preprocess16 takes a 2-D uint16 array")
    H, W = image16.shape
    out = np.empty((H, W), dtype=np.uint8)
    L = _lib.lib()
    L.mrgingham_amd_preprocess_image16.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_void_p]
    if L.mrgingham_amd_preprocess_image16(image16.ctypes.data, W, H, W, int(bool(clahe)), int(blur_radius),
                                          out.ctypes.data) != 0:
        raise RuntimeError("mrgingham_amd: 16-bit preprocessing failed (bad arguments or no device)")
    return out


def find_board(image, image_pyramid_level=-1, gridn=10, blobs=False, debug=False, debug_sequence=None):
    """The full detector: float64 (gridn*gridn, 2) board corners, or None (mrgingham_pywrap.c:227-337).

    image_pyramid_level < 0 (default): try levels 3, 2, 1, 0 until a grid is found, then refine the
    corners down to level 0 (mrgingham.cc:116-139, :81-99)."""
    if blobs and image_pyramid_level != 0:
        raise RuntimeError("blob detector requires that image_pyramid_level == 0")
    dsx = dsy = -1
    if debug_sequence is not None:
        try:
            dsx, dsy = (int(t) for t in str(debug_sequence).split(","))
        except ValueError:
            raise RuntimeError("Couldn't parse debug_sequence as an 'INTEGER,INTEGER' string") from None
    image = _check_image(image, exact_2d=True)
    if gridn < 2:
        raise RuntimeError("gridn value must be >= 2")
    _require_device()
    result = []

    @_lib.ADD_POINTS_F64
    def add_points(xy, n, cookie):  # add_points__find_board, mrgingham_pywrap.c:214-226
        result.append(np.ctypeslib.as_array(xy, shape=(2 * n,)).copy().reshape(n, 2))
        return True

    H, W = image.shape
    stride = image.strides[0] if H > 1 else W
    ok = _lib.lib().find_chessboard_from_image_array_C(H, W, stride, image.ctypes.data, int(gridn),
                                                       int(image_pyramid_level), bool(blobs), bool(debug), dsx, dsy,
                                                       add_points, None)
    return result[0] if ok and result else None  # "possibly found no chessboard": None (:322-330)


find_chessboard = find_board  # compatibility alias, mrgingham_pywrap.c:366


class Detector:
    """Batch interface: frames are a uint8 torch tensor [B,H,W] already on the GPU.

    Wraps one mrgingham_amd_ctx (streams + scratch).  All results stay on the
    device until the caller moves them.
    """

    def __init__(self, device=None):
        import torch
        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("mrgingham_amd.Detector needs a HIP device; there is no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.L = _lib.lib()
        self.ctx = self.L.mrgingham_amd_create(self.device.index)
        if not self.ctx:
            raise RuntimeError("mrgingham_amd_create failed")
        self._options = {}
        self._blobs_cap = 256    # keypoints per frame Detector.blobs makes room for (grows to the largest count seen)
        self._fb_live = {}       # find_boards jobs in flight: ticket -> (boards, found, frames), see find_boards_submit

    def close(self):
        if getattr(self, "ctx", None):
            self.L.mrgingham_amd_destroy(self.ctx)   # (joins the host threads of the jobs in flight: nothing writes after this)
            self.ctx = None
        self._fb_live = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        if self.L.mrgingham_amd_set_option(self.ctx, name.encode(), int(value)) != 0:
            raise ValueError(f"bad option {name}={value}")
        self._options[name] = int(value)

    def _check(self, rc):
        if rc != 0:
            e = RuntimeError(f"mrgingham_amd error {rc}: {self.L.mrgingham_amd_last_error(self.ctx).decode()}")
            e.code = rc
            raise e

    ERR_CAPACITY = -3

    def _sync_retrying(self, issue, retry, restore=None):
        """issue() + sync(); a frame that overflowed the component tables of its level makes the sync fail with
        ERR_CAPACITY *after the tables have grown to what it asked for* (include/mrgingham_amd.h,
        "hot_capacity_shift"), so the same call is simply made again -- like the reference-symbol wrappers of the
        library do it.  `restore` puts in/out arguments back first."""
        full = False
        try:
            for attempt in range(4):
                issue()
                try:
                    self.sync()
                    return
                except RuntimeError as e:
                    if not retry or getattr(e, "code", 0) != self.ERR_CAPACITY or attempt == 3:
                        raise
                    if restore:
                        restore()
                    if attempt == 2:      # the last try takes a table entry for every pixel, like the C wrappers
                        self.L.mrgingham_amd_set_option(self.ctx, b"hot_capacity_shift_temporary", 0)
                        full = True
        finally:
            if full:                      # (back to the caller's choice; what the tables have grown to is KEPT)
                self.L.mrgingham_amd_set_option(self.ctx, b"hot_capacity_shift_temporary", self._options.get("hot_capacity_shift", 7))

    def _frames(self, frames):
        t = self.torch
        assert frames.dtype == t.uint8 and frames.is_cuda and frames.dim() == 3 and frames.stride(2) == 1
        B, H, W = frames.shape
        fr = _lib.Frames(frames.data_ptr(), frames.stride(0) if B > 1 else H * frames.stride(1), B, W, H,
                         frames.stride(1) if H > 1 else W)
        return fr, B, H, W

    def sync(self):
        self._check(self.L.mrgingham_amd_sync(self.ctx))

    def stream_wait(self, stream=None):
        """Make a torch stream (default: the current one) wait, on the device, for every call queued so far (all of
        them, not the last alone: consecutive calls finish on different streams of the context)."""
        t = self.torch
        st = t.cuda.current_stream(self.device) if stream is None else stream
        self._check(self.L.mrgingham_amd_stream_wait(self.ctx, st.cuda_stream))

    def after_stream(self, stream=None):
        """The next queued call starts after what is queued so far on a torch stream (default: the
        current one), e.g. the upload of its frames; on the device, the host is not blocked.  Several calls, one per
        stream, before one queued call are all honoured.  The calls that do not wait for torch's stream themselves --
        detect(out=) and chain(out=) -- need this whenever torch work still queued wrote their frames or touches
        their buffers."""
        t = self.torch
        st = t.cuda.current_stream(self.device) if stream is None else stream
        self._check(self.L.mrgingham_amd_after_stream(self.ctx, st.cuda_stream))

    def chess_response(self, frames, level=0, clamp=False, out=None):
        """Dense int16 response [B,h,w] (border zero).  Runs on torch's current stream."""
        t = self.torch
        fr, B, H, W = self._frames(frames)
        w, h = level_dims(W, H, level)
        if out is None:
            out = t.empty((B, h, w), dtype=t.int16, device=frames.device)
        stream = t.cuda.current_stream(frames.device).cuda_stream
        self._check(self.L.mrgingham_amd_chess_response_batch(self.ctx, ctypes.byref(fr), level, int(clamp),
                                                              out.data_ptr(), stream))
        return out

    def decimate(self, frames, level):
        t = self.torch
        fr, B, H, W = self._frames(frames)
        w, h = level_dims(W, H, level)
        out = t.empty((B, h, w), dtype=t.uint8, device=frames.device)
        stream = t.cuda.current_stream(frames.device).cuda_stream
        self._check(self.L.mrgingham_amd_decimate_batch(self.ctx, ctypes.byref(fr), level, out.data_ptr(), stream))
        return out

    def box_blur(self, frames, radius=1):
        t = self.torch
        fr, B, H, W = self._frames(frames)
        out = t.empty((B, H, W), dtype=t.uint8, device=frames.device)
        stream = t.cuda.current_stream(frames.device).cuda_stream
        self._check(self.L.mrgingham_amd_box_blur_batch(self.ctx, ctypes.byref(fr), radius, out.data_ptr(), stream))
        return out

    def preprocess(self, frames, clahe=True, blur_radius=1):
        """The reference CLI's preprocessing (mrgingham-from-image.cc:71-111): normalize + CLAHE(8),
        then a box blur; on torch's current stream.  uint8 [B,H,W] frames, or uint16 ones (the tool's 16-bit branch,
        :85-92: normalize to 0..65535, CLAHE(8) on 16 bits, convertTo 8 bit with 255/65535) -> uint8 [B,H,W]."""
        t = self.torch
        if frames.dtype == t.uint16:
            return self._preprocess16(frames, clahe, blur_radius)
        fr, B, H, W = self._frames(frames)
        out = t.empty((B, H, W), dtype=t.uint8, device=frames.device)
        stream = t.cuda.current_stream(frames.device).cuda_stream
        self._check(self.L.mrgingham_amd_preprocess_batch(self.ctx, ctypes.byref(fr), int(bool(clahe)),
                                                          int(blur_radius), out.data_ptr(), stream))
        return out

    def _preprocess16(self, frames, clahe, blur_radius):
        t = self.torch
        if not frames.is_cuda or frames.dim() != 3 or frames.stride(2) != 1:
            raise ValueError("16-bit frames: a [B,H,W] uint16 tensor on the device with unit column stride")
        B, H, W = frames.shape
        out = t.empty((B, H, W), dtype=t.uint8, device=frames.device)
        stream = t.cuda.current_stream(frames.device).cuda_stream
        self._check(self.L.mrgingham_amd_preprocess16_batch(
            self.ctx, frames.data_ptr(), frames.stride(0) if B > 1 else H * frames.stride(1), B, W, H,
            frames.stride(1) if H > 1 else W, int(bool(clahe)), int(blur_radius), out.data_ptr(), stream))
        return out

    def detect(self, frames, level, capacity=4096, sync=True, retry=True, out=None):
        """-> (xy int32 [B,capacity,2], counts int32 [B]) on the device.  sync=True waits for the result and, with
        retry, repeats the call when a frame overflowed the (self-growing) component tables.  `out` = (xy, counts) of an
        earlier call to write into (a pipelined caller rotates a few: no allocation, no stream synchronisation per call).

        The caller's duty on the `out=` path: the call runs on the context's own streams and does NOT wait for torch's.
        Frames that torch work still queued produces (a non-blocking upload, preprocessing), and `out` buffers such work
        still reads or writes, need `after_stream()` (for each torch stream involved) BEFORE this call; it is not made
        here because a pipelined step has just told torch's stream to wait for the step before (stream_wait), and a wait
        for that stream would queue this step behind it.  With sync=False, whoever reads xy / counts needs
        `stream_wait()` (a torch stream, on the device) or `sync()` (the host) first.  Calls queued on one Detector
        that share a buffer run in the order they were made."""
        t = self.torch
        fr, B, H, W = self._frames(frames)
        if out is None:
            xy = t.empty((B, capacity, 2), dtype=t.int32, device=frames.device)
            counts = t.empty((B,), dtype=t.int32, device=frames.device)
            t.cuda.current_stream(frames.device).synchronize()  # inputs/outputs ready before the ctx streams run
        else:
            xy, counts = out
            assert xy.dtype == t.int32 and counts.dtype == t.int32 and xy.is_contiguous() and xy.shape[0] == B and counts.shape[0] == B
            capacity = xy.shape[1]

        def issue():
            self._check(self.L.mrgingham_amd_detect_batch(self.ctx, ctypes.byref(fr), level, xy.data_ptr(), capacity,
                                                          counts.data_ptr()))
        if sync:
            self._sync_retrying(issue, retry)
        else:
            issue()
        return xy, counts

    def refine(self, frames, level, points, levels, npoints, sync=True, retry=True):
        """In-place refine of points f64 [B,P,2], levels int8 [B,P], npoints int32 [B]; -> nrefined int32 [B].

        The call waits (on the host) for torch's CURRENT stream before it is queued: frames and points written there are
        complete.  What another torch stream still writes needs `after_stream(that stream)` first.  With sync=False the
        points, levels and nrefined are final only behind `stream_wait()` or `sync()`; a later queued call on the same
        buffers (the next level's refine, a chain into them) is ordered behind this one by the library."""
        t = self.torch
        fr, B, H, W = self._frames(frames)
        assert points.dtype == t.float64 and points.is_contiguous() and levels.dtype == t.int8
        P = points.shape[1]
        nref = t.empty((B,), dtype=t.int32, device=frames.device)
        keep = (points.clone(), levels.clone()) if (sync and retry) else None
        t.cuda.current_stream(frames.device).synchronize()

        def issue():
            self._check(self.L.mrgingham_amd_refine_batch(self.ctx, ctypes.byref(fr), level, points.data_ptr(),
                                                          levels.data_ptr(), npoints.data_ptr(), P, nref.data_ptr()))

        def restore():
            points.copy_(keep[0]); levels.copy_(keep[1])
            t.cuda.current_stream(frames.device).synchronize()
        if sync:
            self._sync_retrying(issue, retry, restore)
        else:
            issue()
        return nref

    def chain(self, frames, start_level=3, max_points=1024, out=None, sync=True, retry=True):
        """detect at start_level, refine down to 0 -> (points f64 [B,P,2], levels int8 [B,P], npoints int32 [B]).

        `out` = (points, levels, npoints) to write into.  As for detect(out=): that path does not wait for torch's stream,
        so frames or `out` buffers that queued torch work still writes or reads need `after_stream()` before the call
        (it is not made here: in a pipelined step torch's stream already waits for the step before, and this step would
        queue behind it); with sync=False a consumer needs `stream_wait()` or `sync()` before it reads the outputs."""
        t = self.torch
        fr, B, H, W = self._frames(frames)
        if out is None:
            out = (t.empty((B, max_points, 2), dtype=t.float64, device=frames.device),
                   t.empty((B, max_points), dtype=t.int8, device=frames.device),
                   t.empty((B,), dtype=t.int32, device=frames.device))
            t.cuda.current_stream(frames.device).synchronize()
        pts, lv, npts = out

        def issue():
            self._check(self.L.mrgingham_amd_chain_batch(self.ctx, ctypes.byref(fr), start_level, pts.data_ptr(),
                                                         lv.data_ptr(), npts.data_ptr(), pts.shape[1]))
        if sync:
            self._sync_retrying(issue, retry)    # (the chain writes all of its outputs: nothing to restore)
        else:
            issue()
        return pts, lv, npts

    def cc_detect_on_response(self, resp, level_images, level=0, capacity=4096, sync=True, retry=True):
        """The component search alone on caller-built responses (int16 [B,h,w], device) and level
        images (uint8 [B,h,w]): -> (xy int32 [B,capacity,2], counts int32 [B]).  For the rule tests."""
        t = self.torch
        assert resp.dtype == t.int16 and resp.is_cuda and resp.is_contiguous() and resp.dim() == 3
        assert level_images.dtype == t.uint8 and level_images.is_contiguous() and level_images.shape == resp.shape
        B, h, w = resp.shape
        xy = t.empty((B, capacity, 2), dtype=t.int32, device=resp.device)
        counts = t.empty((B,), dtype=t.int32, device=resp.device)
        t.cuda.current_stream(resp.device).synchronize()

        def issue():
            self._check(self.L.mrgingham_amd_cc_on_response_batch(self.ctx, resp.data_ptr(), level_images.data_ptr(), B,
                                                                  w, h, level, xy.data_ptr(), capacity,
                                                                  counts.data_ptr(), None, None, None, 0, None))
        if sync:
            self._sync_retrying(issue, retry)
        else:
            issue()
        return xy, counts

    def cc_refine_on_response(self, resp, level_images, level, points, levels, npoints, sync=True, retry=True):
        """In-place refinement of points f64 [B,P,2] / levels int8 [B,P] / npoints int32 [B] against
        caller-built responses; -> nrefined int32 [B]."""
        t = self.torch
        assert resp.dtype == t.int16 and resp.is_cuda and resp.is_contiguous() and resp.dim() == 3
        assert level_images.dtype == t.uint8 and level_images.is_contiguous() and level_images.shape == resp.shape
        assert points.dtype == t.float64 and points.is_contiguous() and levels.dtype == t.int8
        B, h, w = resp.shape
        nref = t.empty((B,), dtype=t.int32, device=resp.device)
        keep = (points.clone(), levels.clone()) if (sync and retry) else None   # (what a capacity retry restores)
        t.cuda.current_stream(resp.device).synchronize()

        def issue():
            self._check(self.L.mrgingham_amd_cc_on_response_batch(self.ctx, resp.data_ptr(), level_images.data_ptr(), B,
                                                                  w, h, level, None, 0, None, points.data_ptr(),
                                                                  levels.data_ptr(), npoints.data_ptr(),
                                                                  points.shape[1], nref.data_ptr()))

        def restore():
            points.copy_(keep[0]); levels.copy_(keep[1])
            t.cuda.current_stream(resp.device).synchronize()
        if sync:
            self._sync_retrying(issue, retry, restore if retry else None)
        else:
            issue()
        return nref

    def blobs(self, frames, nthreads=0):
        """The blob detector (find_blobs_from_image_array, find_blobs.cc:14-46: what find_points(blobs=True) gives one
        host image) over a batch on the device: -> a list of B int32 numpy arrays [n_f, 2], (x, y) * 1000 in
        SimpleBlobDetector's output order.  Synchronous; the last stage of the detector runs on `nthreads` host threads
        (0: all cores, at most 32)."""
        t = self.torch
        if not (isinstance(frames, t.Tensor) and frames.is_cuda and frames.dtype == t.uint8 and frames.dim() == 3
                and (frames.shape[2] <= 1 or frames.stride(2) == 1)):
            raise ValueError("blobs: a [B,H,W] uint8 tensor on the device with unit column stride")
        fr, B, H, W = self._frames(frames)
        if B == 0:
            return []
        t.cuda.current_stream(frames.device).synchronize()
        counts = np.zeros((B,), dtype=np.int32)
        cap = self._blobs_cap
        while True:
            xy = np.empty((B, cap, 2), dtype=np.int32)
            rc = self.L.mrgingham_amd_blobs_batch(self.ctx, ctypes.byref(fr), xy.ctypes.data, cap, counts.ctypes.data,
                                                  int(nthreads))
            self._check(rc)
            if counts.max() <= cap:
                return [xy[f, :counts[f]].copy() for f in range(B)]
            cap = self._blobs_cap = int(counts.max())   # (more keypoints than guessed: again, sized to the largest; remembered)

    def jpeg_idct(self, coef, quant, height, width, out=None):
        """Dequantisation + inverse DCT of entropy-decoded JPEG frames on the device (mrgingham_amd_jpeg_idct_batch), on
        torch's current stream: coef int16 [B, bh, bw, 64] and quant uint16 [B, 64] device tensors as jpeg_coefficients
        gives them per frame -> uint8 [B, height, width], the bytes read_image gives for the file.  `out`: a uint8
        [B, height, >= width] device tensor (unit column stride) to write into; what lies beyond `width` is not touched."""
        t = self.torch
        if not (coef.is_cuda and coef.dtype == t.int16 and coef.dim() == 4 and coef.shape[3] == 64 and coef.is_contiguous()):
            raise ValueError("jpeg_idct: coef is a contiguous int16 [B,bh,bw,64] tensor on the device")
        B, bh, bw, _ = coef.shape
        if not (quant.is_cuda and quant.dtype in (t.uint16, t.int16) and tuple(quant.shape) == (B, 64) and quant.is_contiguous()):
            raise ValueError("jpeg_idct: quant is a contiguous uint16 [B,64] tensor on the device")
        if out is None:
            out = t.empty((B, height, width), dtype=t.uint8, device=coef.device)
        if not (out.is_cuda and out.dtype == t.uint8 and out.dim() == 3 and out.shape[0] == B and out.shape[1] == height
                and out.shape[2] >= width and (out.shape[2] <= 1 or out.stride(2) == 1)):
            raise ValueError("jpeg_idct: out is a uint8 [B,height,>=width] tensor on the device with unit column stride")
        stream = t.cuda.current_stream(coef.device).cuda_stream
        self._check(self.L.mrgingham_amd_jpeg_idct_batch(
            self.ctx, coef.data_ptr(), bh * bw * 64, quant.data_ptr(), B, int(width), int(height), bw, bh, out.data_ptr(),
            out.stride(0) if B > 1 else height * out.stride(1), out.stride(1) if height > 1 else out.shape[2], stream))
        return out[:, :, :width]

    def _with_options(self, **values):
        """Context manager: the options set for the duration of a call, and what they were afterwards."""
        @contextlib.contextmanager
        def scope():
            defaults = {"jpeg_entropy": 0, "jpeg_sync": 0, "tiff_deflate": 0}
            before = {k: self._options.get(k, defaults[k]) for k in values}
            try:
                for k, v in values.items():
                    self.set_option(k, v)
                yield
            finally:
                for k, v in before.items():
                    self.set_option(k, v)
        return scope()

    def jpeg_entropy(self, datas, height, width, sync=False):
        """Huffman decode of baseline JPEG files held in memory ON THE DEVICE, one lane per restart interval
        (mrgingham_amd_jpeg_entropy_batch): `datas` are the files' bytes, all height x width.  -> (coef int16
        [B, bh, bw, 64], quant uint16 [B, 64]) device tensors as jpeg_idct takes them -- bh x bw the largest block counts
        any sampling gives the size -- and status int32 [B] (numpy): 0 decoded (what jpeg_coefficients gives, in the top
        left corner of the file's area), -1 unreadable, -2 another size, -3 readable but without restart intervals (or
        longer ones than option "jpeg_entropy_max_interval"): decode those with jpeg_coefficients.  Files whose status is
        not 0 have zero coefficients and tables.  Synchronous.  sync=True: option "jpeg_sync" is 1 for this call (and what
        it was afterwards) -- files without restart intervals are decoded as well, cut into subsequences of option
        "jpeg_sync_subsequence" bytes that synchronise themselves; -3 then also means: not within "jpeg_sync_max_rounds"
        update rounds (jpeg_sync_rounds tells how many a file needs).  sync=False sets the option to 0 for the call, whatever
        set_option has made it (as read_jpegs treats `entropy`)."""
        t = self.torch
        bufs = [bytes(d) for d in datas]
        B = len(bufs)

        def padded(side):
            return max(-(-side // (8 * h)) * h for h in (1, 2, 3, 4))
        bh, bw = padded(int(height)), padded(int(width))
        coef = t.empty((B, bh, bw, 64), dtype=t.int16, device=self.device)
        quant = t.empty((B, 64), dtype=t.uint16, device=self.device)
        status = np.full((B,), -1, dtype=np.int32)
        if B == 0:
            return coef, quant, status
        ptrs = (ctypes.c_char_p * B)(*bufs)
        sizes = (ctypes.c_size_t * B)(*[len(b) for b in bufs])
        t.cuda.current_stream(self.device).synchronize()
        with self._with_options(jpeg_sync=int(bool(sync))):
            self._check(self.L.mrgingham_amd_jpeg_entropy_batch(self.ctx, ptrs, sizes, B, int(width), int(height), coef.data_ptr(),
                                                                bh * bw * 64, bw, bh, quant.data_ptr(), status.ctypes.data))
        return coef, quant, status

    def read_jpegs(self, paths, nthreads=0, entropy="host", sync=False):
        """Baseline JPEG files of one size straight into device frames (mrgingham_amd_read_jpegs_batch): `nthreads` host
        threads (0: all cores, at most 32) entropy-decode, the device runs the inverse DCT; the decoded pixels never exist
        on the host.  -> (frames uint8 [B,H,W] on the device, status int32 [B] numpy: 0 decoded, -1 unreadable /
        unsupported / malformed, -2 a JPEG of another size; failed frames are zero).  The size is that of the first file
        whose header parses (none does: frames are [B,0,0]).  Synchronous.  entropy="device": option "jpeg_entropy" is 1
        for this call (and what it was afterwards) -- files with restart intervals are Huffman-decoded on the device as
        well, the host threads only find their markers; same frames, same statuses.  sync=True (with entropy="device"):
        option "jpeg_sync" is 1 for this call as well -- files without restart intervals are Huffman-decoded on the device
        too (see jpeg_entropy); one that does not converge within the cap is decoded by the host threads afterwards."""
        if entropy not in ("host", "device"):
            raise ValueError('read_jpegs: entropy is "host" or "device"')
        if sync and entropy != "device":
            raise ValueError('read_jpegs: sync=True needs entropy="device"')
        t = self.torch
        names = [os.fsencode(p) for p in paths]
        B = len(names)
        status = np.full((B,), -1, dtype=np.int32)
        H = W = 0
        for name in names:
            try:
                with open(name, "rb") as f:
                    head = jpeg_coefficients_size(f.read())
            except OSError:
                head = None
            if head is not None:
                H, W = head
                break
        frames = t.zeros((B, H, W), dtype=t.uint8, device=self.device)
        if B == 0 or H == 0:
            return frames, status
        arr = (ctypes.c_char_p * B)(*names)
        t.cuda.current_stream(self.device).synchronize()
        with self._with_options(jpeg_entropy=int(entropy == "device"), jpeg_sync=int(bool(sync))):
            self._check(self.L.mrgingham_amd_read_jpegs_batch(self.ctx, arr, B, W, H, frames.data_ptr(), H * W, W, int(nthreads),
                                                              status.ctypes.data))
        return frames, status

    def _check_payload(self, who, payload, need_bytes, message):
        """the [B,P] payload tensor of an *_unpack method; `message`: what P is at least, for the error"""
        if not (payload.is_cuda and payload.dtype == self.torch.uint8 and payload.dim() == 2 and payload.is_contiguous()
                and payload.shape[1] % 16 == 0 and payload.shape[1] >= need_bytes and payload.data_ptr() % 16 == 0):
            raise ValueError(f"{who}: payload is a contiguous, 16-byte aligned uint8 [B,P] tensor on the device, P a multiple of 16 and at least {message}")

    def _out_frames(self, who, payload, out, height, width, dtype, message):
        """`out` of a method that writes [B,height,width] frames for the B rows of `payload`, on its device (None: new
        frames), checked -> (out, frame_pitch, stride) in samples, as the _batch entry points take them"""
        B = payload.shape[0]
        if out is None:
            out = self.torch.empty((B, height, width), dtype=dtype, device=payload.device)
        if not (out.is_cuda and out.dtype == dtype and out.dim() == 3 and out.shape[0] == B and out.shape[1] == height
                and out.shape[2] >= width and (out.shape[2] <= 1 or out.stride(2) == 1)):
            raise ValueError(f"{who}: {message}")
        return out, out.stride(0) if B > 1 else height * out.stride(1), out.stride(1) if height > 1 else out.shape[2]

    def _read_files(self, entry, names, H, W, bits, nthreads, pass_bits):
        """the tail of the read_* methods: `names` (encoded) through the batch loader `entry` into new H x W frames of
        `bits` bits (pass_bits: the loader takes the depth) -> (frames, status)"""
        t = self.torch
        B = len(names)
        status = np.full((B,), -1, dtype=np.int32)
        frames = t.zeros((B, H, W), dtype=t.uint8 if bits == 8 else t.uint16, device=self.device)
        if B == 0 or H == 0:
            return frames, status
        arr = (ctypes.c_char_p * B)(*names)
        t.cuda.current_stream(self.device).synchronize()
        self._check(entry(self.ctx, arr, B, W, H, *((bits,) if pass_bits else ()), frames.data_ptr(), H * W, W, int(nthreads),
                          status.ctypes.data))
        return frames, status

    def png_reconstruct(self, scan, height, width, bits, color_type, out=None):
        """The row filters of inflated PNG scanlines undone and the samples reduced to grey on the device
        (mrgingham_amd_png_reconstruct_batch), on torch's current stream: scan uint8 [B, height, width*bpp + 1] device tensor,
        frame by frame what png_scanlines gives (bits 8 or 16, color_type 0, 2, 4 or 6) -> uint8 (bits 8) or uint16 (bits 16)
        [B, height, width], the samples read_image's decoder gives for the file.  `out`: a [B, height, >= width] device
        tensor of that type (unit column stride) to write into; what lies beyond `width` is not touched."""
        t = self.torch
        bpp = _PNG_BPP.get((int(bits), int(color_type)))
        if bpp is None:
            raise ValueError("png_reconstruct: bits 8 or 16, color_type 0, 2, 4 or 6")
        if not (scan.is_cuda and scan.dtype == t.uint8 and scan.dim() == 3 and scan.is_contiguous()
                and tuple(scan.shape[1:]) == (height, width * bpp + 1)):
            raise ValueError("png_reconstruct: scan is a contiguous uint8 [B,height,width*bpp+1] tensor on the device")
        out, frame_pitch, stride = self._out_frames(
            "png_reconstruct", scan, out, height, width, t.uint8 if bits == 8 else t.uint16,
            "out is a [B,height,>=width] tensor on the device with unit column stride, uint8 or uint16 by bits")
        stream = t.cuda.current_stream(scan.device).cuda_stream
        self._check(self.L.mrgingham_amd_png_reconstruct_batch(
            self.ctx, scan.data_ptr(), height * (width * bpp + 1), scan.shape[0], int(width), int(height), int(bits), int(color_type),
            out.data_ptr(), frame_pitch, stride, stream))
        return out[:, :, :width]

    def read_pngs(self, paths, nthreads=0):
        """PNG files of one size and depth straight into device frames (mrgingham_amd_read_pngs_batch): `nthreads` host
        threads (0: all cores, at most 32) inflate, the device undoes the row filters and reduces colour to grey.  ->
        (frames uint8 or uint16 [B,H,W] on the device, status int32 [B] numpy: 0 decoded, -1 unreadable / unsupported /
        malformed, -2 a PNG of another size or depth; failed frames are zero).  Size and depth are those of the first file
        whose header parses (none does: uint8 frames [B,0,0]).  Palette files are decoded by the host threads: same bytes.
        Synchronous."""
        names = [os.fsencode(p) for p in paths]
        H = W = 0
        bits = 8
        for name in names:
            try:
                with open(name, "rb") as f:
                    head = png_scanlines_size(f.read())
            except OSError:
                head = None
            if head is not None:
                H, W, bits, _ = head
                break
        return self._read_files(self.L.mrgingham_amd_read_pngs_batch, names, H, W, bits, nthreads, True)

    def pgm_unpack(self, payload, height, width, bits, out=None):
        """The payloads of binary PGM files to frames on the device (mrgingham_amd_pgm_unpack_batch), on torch's current
        stream: payload uint8 [B, P] device tensor, contiguous and 16-byte aligned, P a multiple of 16 and at least
        height*width*bits/8 -- row f holds file f's samples as they lie behind its header, bytes (bits 8) or big-endian
        pairs (bits 16) -> uint8 or uint16 [B, height, width].  `out`: a [B, height, >= width] device tensor of that type
        (unit column stride) to write into; what lies beyond `width` is not touched.  It may be a view of `payload` itself
        where the layouts coincide (a dense [B, height, width] view of a payload with P == height*width*bits/8)."""
        t = self.torch
        if bits not in (8, 16):
            raise ValueError("pgm_unpack: bits 8 or 16")
        self._check_payload("pgm_unpack", payload, height * width * (bits // 8), "height*width*bits/8")
        out, frame_pitch, stride = self._out_frames(
            "pgm_unpack", payload, out, height, width, t.uint8 if bits == 8 else t.uint16,
            "out is a [B,height,>=width] tensor on the device with unit column stride, uint8 or uint16 by bits")
        stream = t.cuda.current_stream(payload.device).cuda_stream
        self._check(self.L.mrgingham_amd_pgm_unpack_batch(
            self.ctx, payload.data_ptr(), payload.shape[1], payload.shape[0], int(width), int(height), int(bits), out.data_ptr(), frame_pitch,
            stride, stream))
        return out[:, :, :width]

    def read_pgms(self, paths, nthreads=0):
        """Binary PGM files of one size and depth straight into device frames (mrgingham_amd_read_pgms_batch): `nthreads`
        host threads (0: all cores, at most 32) read the payloads from the files into page-locked staging, the device
        swaps the bytes of 16-bit samples and lays out the frames.  -> (frames uint8 or uint16 [B,H,W] on the device,
        status int32 [B] numpy: 0 loaded, -1 unreadable or not a PGM (a file shorter than its header promises included),
        -2 a PGM of another size or depth; failed frames are zero).  Size and depth are those of the first file whose
        header parses (none does: uint8 frames [B,0,0]).  Synchronous."""
        names = [os.fsencode(p) for p in paths]
        H = W = 0
        bits = 8
        for name in names:
            try:
                with open(name, "rb") as f:
                    data = f.read(4096)
                    head = pgm_header(data)
                    if head == PGM_HEADER_CUT:
                        head = pgm_header(data + f.read())
            except OSError:
                head = None
            if head is not None and head != PGM_HEADER_CUT:
                H, W, bits, _ = head
                break
        return self._read_files(self.L.mrgingham_amd_read_pgms_batch, names, H, W, bits, nthreads, True)

    def bmp_unpack(self, payload, lut, height, width, bits, top_down=False, out=None):
        """The pixel arrays of Windows Bitmap files to grey frames on the device (mrgingham_amd_bmp_unpack_batch), on torch's
        current stream: payload uint8 [B, P] device tensor, contiguous and 16-byte aligned, P a multiple of 16 and at least
        row_bytes*height with row_bytes = ((width*bits + 31) // 32) * 4 -- row f holds file f's pixel array as it lies in
        the file from bfOffBits on; lut uint8 [B, 256] device tensor, contiguous: the grey tables (bmp_layout(..).lut) for
        bits 1, 4 and 8 -- None at 8 bits: the identity table, a flipped copy; not looked at for bits 24 and 32
        -> uint8 [B, height, width].  top_down: row 0 of the array is the top row (a negative height in the file).  `out`: a
        [B, height, >= width] uint8 device tensor (unit column stride, any byte address) to write into; what lies beyond
        `width` is not touched."""
        t = self.torch
        if bits not in (1, 4, 8, 24, 32):
            raise ValueError("bmp_unpack: bits 1, 4, 8, 24 or 32")
        rowb = (width * bits + 31) // 32 * 4
        self._check_payload("bmp_unpack", payload, height * rowb, "row_bytes*height")
        B = payload.shape[0]
        need_lut = bits < 8 or (bits == 8 and lut is not None)
        if bits < 8 and lut is None:
            raise ValueError("bmp_unpack: bits 1 and 4 need the grey tables")
        if need_lut and not (lut.is_cuda and lut.dtype == t.uint8 and tuple(lut.shape) == (B, 256) and lut.is_contiguous()):
            raise ValueError("bmp_unpack: lut is a contiguous uint8 [B,256] tensor on the device")
        out, frame_pitch, stride = self._out_frames("bmp_unpack", payload, out, height, width, t.uint8,
                                                    "out is a uint8 [B,height,>=width] tensor on the device with unit column stride")
        stream = t.cuda.current_stream(payload.device).cuda_stream
        self._check(self.L.mrgingham_amd_bmp_unpack_batch(
            self.ctx, payload.data_ptr(), payload.shape[1], lut.data_ptr() if need_lut else None, B, int(width), int(height), int(bits),
            int(bool(top_down)), int(bits == 8 and lut is None), out.data_ptr(), frame_pitch, stride, stream))
        return out[:, :, :width]

    def read_bmps(self, paths, nthreads=0):
        """Windows Bitmap files of one size straight into device frames (mrgingham_amd_read_bmps_batch); depth, row order and
        palette may differ from file to file: `nthreads` host threads (0: all cores, at most 32) read the grey tables and
        the pixel arrays from the files into page-locked staging, the device flips and unpads the rows, unpacks the indices,
        looks up the palette and reduces colour to grey (option "bmp_unpack" 0: the host threads decode instead); RLE8 files
        are decoded by their host thread.  -> (frames uint8 [B,H,W] on the device, status int32 [B] numpy: 0 loaded, -1
        unreadable or not a BMP, -2 a BMP of another size; failed frames are zero).  The size is that of the first file
        whose header parses (none does: frames [B,0,0]).  Synchronous."""
        names = [os.fsencode(p) for p in paths]
        H = W = 0
        for name in names:
            probe = probe_image(name)
            if probe is not None and probe[3] == KIND_BMP:
                H, W = probe[0], probe[1]
                break
        return self._read_files(self.L.mrgingham_amd_read_bmps_batch, names, H, W, 8, nthreads, False)

    def pnm_unpack(self, payload, height, width, bits, channels, black_and_white=False, out=None):
        """The rasters of binary Netpbm files to grey frames on the device (mrgingham_amd_pnm_unpack_batch), on torch's current
        stream: payload uint8 [B, P] device tensor, contiguous and 16-byte aligned, P a multiple of 16 and at least
        row_bytes*height with row_bytes = (width + 7) // 8 for bits 1 and width*channels*bits/8 otherwise -- row f holds file
        f's raster as it lies behind its header -> uint8 [B, height, width] for bits 1 and 8, uint16 for bits 16.  channels
        1 .. 4 (1 at bits 1): the grey is the first sample, or the fixed-point BT.601 grey of the first three; a second or
        fourth sample is ignored.  black_and_white (bits 8, channels 1 or 2): 255 where the first sample is non-zero.
        `out`: a [B, height, >= width] device tensor of that type (unit column stride, any sample address) to write into;
        what lies beyond `width` is not touched."""
        t = self.torch
        if bits not in (1, 8, 16) or channels not in (1, 2, 3, 4) or (bits == 1 and channels != 1):
            raise ValueError("pnm_unpack: bits 1 (one channel), 8 or 16 with 1 .. 4 channels")
        if black_and_white and (bits != 8 or channels > 2):
            raise ValueError("pnm_unpack: black_and_white with bits 8 and 1 or 2 channels")
        rowb = (width + 7) // 8 if bits == 1 else width * channels * bits // 8
        self._check_payload("pnm_unpack", payload, height * rowb, "row_bytes*height")
        out, frame_pitch, stride = self._out_frames(
            "pnm_unpack", payload, out, height, width, t.uint16 if bits == 16 else t.uint8,
            "out is a [B,height,>=width] tensor on the device with unit column stride, uint8 or uint16 by bits")
        stream = t.cuda.current_stream(payload.device).cuda_stream
        self._check(self.L.mrgingham_amd_pnm_unpack_batch(
            self.ctx, payload.data_ptr(), payload.shape[1], payload.shape[0], int(width), int(height), int(bits), int(channels),
            int(bool(black_and_white)), out.data_ptr(), frame_pitch, stride, stream))
        return out[:, :, :width]

    def raw_unpack(self, payload, height, width, fmt, row_bytes=None, out=None):
        """Packed 10 / 12 / 14-bit camera frames to uint16 frames on the device (mrgingham_amd_raw_unpack_batch), on torch's
        current stream: payload uint8 [B, P] device tensor, contiguous and 16-byte aligned, P a multiple of 16 and at least
        (height-1)*row_bytes + raw_row_bytes(width, fmt) -- row f holds frame f as the camera delivered it, row y at byte
        y*row_bytes (None: raw_row_bytes(width, fmt), rows without padding) -> uint16 [B, height, width], the samples as they
        are (0 .. 2^N - 1).  fmt: "p10", "p12", "p14" (GenICam Mono10p / Mono12p / Mono14p: an LSB-first bit stream per row),
        "gev10", "gev12" (GigE Vision Mono10Packed / Mono12Packed: 3-byte pixel pairs).  `out`: a [B, height, >= width]
        uint16 device tensor (unit column stride) to write into; what lies beyond `width` is not touched; it must not
        overlap `payload`.

            frames = det.raw_unpack(payload, 3072, 4096, "p12")         # what the grabber wrote, uploaded as it is
            boards, found = det.find_boards(det.preprocess(frames), gridn=10)"""
        t = self.torch
        f = _raw_format(fmt, "raw_unpack")
        rmin = raw_row_bytes(width, fmt)
        rowb = rmin if row_bytes is None else int(row_bytes)
        if not (1 <= height <= 32767) or rowb < rmin:
            raise ValueError("raw_unpack: height 1 .. 32767, row_bytes at least raw_row_bytes(width, fmt)")
        self._check_payload("raw_unpack", payload, (height - 1) * rowb + rmin, "(height-1)*row_bytes + raw_row_bytes(width, fmt)")
        out, frame_pitch, stride = self._out_frames("raw_unpack", payload, out, height, width, t.uint16,
                                                    "out is a uint16 [B,height,>=width] tensor on the device with unit column stride")
        stream = t.cuda.current_stream(payload.device).cuda_stream
        self._check(self.L.mrgingham_amd_raw_unpack_batch(
            self.ctx, payload.data_ptr(), payload.shape[1], payload.shape[0], int(width), int(height), rowb, f, out.data_ptr(), frame_pitch,
            stride, stream))
        return out[:, :, :width]

    def bayer_grey(self, frames, pattern, out=None):
        """Bayer mosaics to grey frames on the device (mrgingham_amd_bayer_grey_batch), on torch's current stream: frames
        uint8 or uint16 [B,H,W] device tensor with unit column stride (views with any row and frame stride are taken as
        they are), sides 2 .. 32767 -> the same dtype and shape.  pattern: "rggb", "grbg", "gbrg", "bggr" (GenICam BayerRG /
        BayerGR / BayerGB / BayerBG): the colours of pixels (0,0), (0,1), (1,0), (1,1).  Bilinear demosaicing and the luma in
        one rounding, borders by reflect-101 (include/mrgingham_amd.h has the definition).  `out`: a [B,H,W] device tensor of
        the same dtype (unit column stride) to write into; it must not overlap `frames`.

            grey = det.bayer_grey(mosaics, "rggb")                      # uint8: straight into find_boards
            boards, found = det.find_boards(grey, gridn=10)
            frames = det.raw_unpack(payload, 3072, 4096, "p12")         # BayerRG12p as the grabber wrote it
            boards, found = det.find_boards(det.preprocess(det.bayer_grey(frames, "rggb")), gridn=10)"""
        t = self.torch
        p = _bayer_pattern(pattern, "bayer_grey")
        if not (t.is_tensor(frames) and frames.is_cuda and frames.dtype in (t.uint8, t.uint16) and frames.dim() == 3
                and 2 <= frames.shape[1] <= 32767 and 2 <= frames.shape[2] <= 32767 and frames.stride(2) == 1
                and frames.stride(1) >= frames.shape[2] and frames.stride(0) >= 0):
            raise ValueError("bayer_grey: frames is a uint8 or uint16 [B,H,W] tensor on the device, sides 2 .. 32767, unit column stride")
        B, H, W = frames.shape
        if out is None:
            out = t.empty((B, H, W), dtype=frames.dtype, device=frames.device)
        if not (t.is_tensor(out) and out.is_cuda and out.device == frames.device and out.dtype == frames.dtype and tuple(out.shape) == (B, H, W)
                and out.stride(2) == 1 and out.stride(1) >= W and (B <= 1 or out.stride(0) >= (H - 1) * out.stride(1) + W)):
            raise ValueError("bayer_grey: out is a [B,H,W] tensor of the frames' dtype on their device with unit column stride, its frames apart")
        stream = t.cuda.current_stream(frames.device).cuda_stream
        self._check(self.L.mrgingham_amd_bayer_grey_batch(
            self.ctx, frames.data_ptr(), 8 * frames.element_size(), B, W, H, frames.stride(0) if B > 1 else 0, frames.stride(1), p,
            out.data_ptr(), out.stride(0) if B > 1 else 0, out.stride(1), stream))
        return out

    def colour_grey(self, frames, format, out=None):
        """Colour frames to grey frames on the device (mrgingham_amd_colour_grey_batch), on torch's current stream: frames
        uint8 or uint16 device tensor, [B,H,W,C] with stride(3) == 1 and stride(2) == C -- C = 3 for "rgb" / "bgr", 4 for
        "rgba" / "bgra" (the fourth sample is ignored), 2 for "yuyv" / "uyvy" (uint8 only: the Y byte as it is) -- or
        [B,3,H,W] with stride(3) == 1 for "rgb_planar" / "bgr_planar" (torch's own layout for images); any row, plane and
        frame stride is taken as it is; sides 1 .. 32767 -> [B,H,W] of the same dtype:
        (4899 R + 9617 G + 1868 B + 8192) >> 14, the grey of the colour file readers (include/mrgingham_amd.h has the
        definition).  `out`: a [B,H,W] device tensor of the same dtype (unit column stride) to write into; it must not
        overlap `frames`.  The Y plane of an NV12 / 4:2:0 frame is a [B,H,W] view already: find_boards takes it as it is.

            boards, found = det.find_boards(det.colour_grey(rgb, "rgb_planar"), gridn=10)        # uint8 [B,3,H,W]
            boards, found = det.find_boards(det.preprocess(det.colour_grey(rgb16, "rgb")), gridn=10)   # uint16 [B,H,W,3]"""
        t = self.torch
        f = _colour_format(format, "colour_grey")
        C = _COLOUR_SAMPLES[f]
        planar = C == 1
        if not (t.is_tensor(frames) and frames.is_cuda and frames.dtype in (t.uint8, t.uint16) and frames.dim() == 4
                and (f < 6 or frames.dtype == t.uint8) and frames.stride(3) == 1 and frames.stride(0) >= 0
                and (frames.shape[1] == 3 and frames.stride(1) >= 0 if planar else frames.shape[3] == C and frames.stride(2) == C)):
            raise ValueError("colour_grey: frames is a uint8 or uint16 tensor on the device, [B,H,W,C] with strides (.., .., C, 1), C = 3, 4, or 2 "
                             "(4:2:2, uint8), or [B,3,H,W] with unit column stride for the planar formats")
        B = frames.shape[0]
        H, W = frames.shape[2:] if planar else frames.shape[1:3]
        row_stride = frames.stride(2) if planar else frames.stride(1)
        if not (1 <= H <= 32767 and 1 <= W <= 32767 and (H == 1 or row_stride >= C * W)):
            raise ValueError("colour_grey: sides 1 .. 32767, rows at least a row apart")
        if out is None:
            out = t.empty((B, H, W), dtype=frames.dtype, device=frames.device)
        if not (t.is_tensor(out) and out.is_cuda and out.device == frames.device and out.dtype == frames.dtype and tuple(out.shape) == (B, H, W)
                and out.stride(2) == 1 and (H == 1 or out.stride(1) >= W) and (B <= 1 or out.stride(0) >= (H - 1) * out.stride(1) + W)):
            raise ValueError("colour_grey: out is a [B,H,W] tensor of the frames' dtype on their device with unit column stride, its frames apart")
        stream = t.cuda.current_stream(frames.device).cuda_stream
        self._check(self.L.mrgingham_amd_colour_grey_batch(
            self.ctx, frames.data_ptr(), 8 * frames.element_size(), f, B, W, H, frames.stride(0) if B > 1 else 0,
            frames.stride(1) if planar else 0, row_stride if H > 1 else C * W, out.data_ptr(), out.stride(0) if B > 1 else 0,
            out.stride(1) if H > 1 else W, stream))
        return out

    def read_pnms(self, paths, nthreads=0):
        """Binary Netpbm files (P4, P5, P7 in any mix) of one size and output depth straight into device frames
        (mrgingham_amd_read_pnms_batch): `nthreads` host threads (0: all cores, at most 32) read the rasters from the files
        into page-locked staging, the device unpacks bits, swaps the bytes of 16-bit samples and reduces colour to grey
        (option "pnm_unpack" 0: the host threads decode instead).  -> (frames uint8 or uint16 [B,H,W] on the device, status
        int32 [B] numpy: 0 loaded, -1 unreadable or not Netpbm, -2 another size or depth; failed frames are zero).  Size and
        depth are those of the first file whose header parses (none does: uint8 frames [B,0,0]).  Synchronous."""
        names = [os.fsencode(p) for p in paths]
        H = W = 0
        bits = 8
        for name in names:
            probe = probe_image(name)
            if probe is not None and probe[3] in (KIND_PGM, KIND_PNM):
                H, W, bits = probe[0], probe[1], probe[2]
                break
        return self._read_files(self.L.mrgingham_amd_read_pnms_batch, names, H, W, bits, nthreads, True)

    def tiff_decode(self, datas, layouts=None, out=None):
        """TIFF files held in memory to grey frames on the device (mrgingham_amd_tiff_decode_batch_tiled), on torch's current
        stream: datas, a list of bytes; layouts, their tiff_layout results (default: computed here, with tiles=True), which must
        all be taken by the device route and agree in every field, the tile sizes among them -> (frames uint8 or uint16 [B, height, width], the samples
        read_image's decoder gives; status int32 [B] numpy: 0, or -1 for a file whose LZW or Deflate strips broke a rule -- its frame
        is zero; strip_status int32 [B, P] numpy: per strip what stopped its lane, 0 for none).  `out`: a [B, height,
        >= width] device tensor of that type (unit column stride) to write into; what lies beyond `width` is not touched.
        Synchronises (the status words come back)."""
        t = self.torch
        datas = [bytes(d) for d in datas]
        if layouts is None:
            layouts = [tiff_layout(d, tiles=True) for d in datas]
        B = len(datas)
        if (B == 0 or len(layouts) != B or any(l is None or not l.taken for l in layouts)
                or len({l.key() + (l.tile_width, l.tile_length) for l in layouts}) != 1):
            raise ValueError("tiff_decode: at least one file, all taken by the device route (tiff_layout) and equal in every field")
        lay = layouts[0]
        W, H, P = lay.width, lay.height, max(l.nstrips for l in layouts)
        pitch = (max(len(d) for d in datas) + 15) // 16 * 16
        h_files = np.zeros((B, pitch), dtype=np.uint8)
        h_strips = np.zeros((B, P), dtype=TIFF_STRIP)
        for i, (d, l) in enumerate(zip(datas, layouts)):
            h_files[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
            h_strips[i, :l.nstrips] = l.strips
        d_files = t.from_numpy(h_files).to(self.device)
        d_strips = t.from_numpy(h_strips.view(np.uint8).reshape(B, -1)).to(self.device)
        d_ns = t.tensor([l.nstrips for l in layouts], dtype=t.int32, device=self.device)
        d_status = t.full((B,), -7, dtype=t.int32, device=self.device)
        d_sstatus = t.zeros((B, P), dtype=t.int32, device=self.device)
        out, frame_pitch, stride = self._out_frames(
            "tiff_decode", d_files, out, H, W, t.uint8 if lay.bits == 8 else t.uint16,
            "out is a [B,height,>=width] tensor on the device with unit column stride, uint8 or uint16 by bits")
        info = _lib.TiffInfo(*lay.key())
        stream = t.cuda.current_stream(self.device).cuda_stream
        self._check(self.L.mrgingham_amd_tiff_decode_batch_tiled(
            self.ctx, d_files.data_ptr(), pitch, d_strips.data_ptr(), P, d_ns.data_ptr(), B, ctypes.byref(info), lay.tile_width,
            lay.tile_length, out.data_ptr(), frame_pitch, stride, d_status.data_ptr(), d_sstatus.data_ptr(), stream))
        return out[:, :, :W], d_status.cpu().numpy(), d_sstatus.cpu().numpy()

    def read_tiffs(self, paths, nthreads=0, deflate=None):
        """TIFF files of one size and depth straight into device frames (mrgingham_amd_read_tiffs_batch): `nthreads` host
        threads (0: all cores, at most 32) read the files into page-locked staging and parse their directories, the device
        decodes the LZW strips one lane each, undoes the predictor and reduces colour to grey.  -> (frames uint8 or uint16
        [B,H,W] on the device, status int32 [B] numpy: 0 decoded, -1 unreadable / unsupported / malformed, -2 a TIFF of
        another size or depth; failed frames are zero).  Size and depth are those of the first file whose directory
        parses (none does: uint8 frames [B,0,0]).  PackBits and Deflate files, and LZW files with a strip above option
        "tiff_lzw_max_strip", are decoded by the host threads: same bytes.  Tiled files go the same ways tile by tile, and may
        share a list with strip files; one whose tile width is no multiple of 16, or with more tiles than rows, keeps the host
        threads.  deflate="device": Deflate files whose strips
        decode to at most option "tiff_deflate_max_strip" go through the device like LZW files; "host": the host threads
        inflate them; None (default): as option "tiff_deflate" of this detector says.  Either value holds for this call
        only: the option is afterwards what it was.  Synchronous."""
        if deflate not in (None, "host", "device"):
            raise ValueError('read_tiffs: deflate is None, "host" or "device"')
        if deflate is not None:
            with self._with_options(tiff_deflate=int(deflate == "device")):
                return self.read_tiffs(paths, nthreads)
        names = [os.fsencode(p) for p in paths]
        H = W = 0
        bits = 8
        for p in paths:
            head = probe_image(p)
            if head is not None and head[3] == KIND_TIFF:
                H, W, bits, _ = head
                break
        return self._read_files(self.L.mrgingham_amd_read_tiffs_batch, names, H, W, bits, nthreads, True)

    BLOBS_STATS = ("calls", "chunks", "nodes", "contours", "points", "device_ms", "host_ms", "frames")

    def blobs_stats(self, reset=True):
        """mrgingham_amd_blobs_stats as a dict (totals since the last reset; device_ms only while kernel timing is on)."""
        out = np.zeros(len(self.BLOBS_STATS), dtype=np.float64)
        n = self.L.mrgingham_amd_blobs_stats(self.ctx, out.ctypes.data, len(out), int(bool(reset)))
        if n < 0:
            self._check(n)
        return dict(zip(self.BLOBS_STATS, out.tolist()))

    def find_boards(self, frames, gridn=10, image_pyramid_level=-1, nthreads=0, blobs=False, refine=True, levels=False):
        """Full detector over a batch: -> (boards float64 [B, gridn*gridn, 2] (numpy, host),
        found_level int8 [B], -1 where no board was found).  Synchronous.  blobs=True (level 0 only): a grid of dark
        circles instead of a chessboard -- the blob detector, then the grid finder, no refinement
        (find_circle_grid_from_image_array, bridge.cc:104-113); found is 0 or -1.  refine=False: the boards stay as the
        grid finder made them; levels=True: a third array, int8 [B, gridn*gridn], the pyramid level every corner of a
        found board ended at (mrgingham_amd_find_boards_submit_ex)."""
        t = self.torch
        if blobs and image_pyramid_level != 0:
            raise RuntimeError("blob detector requires that image_pyramid_level == 0")
        if blobs and (levels or not refine):
            raise ValueError("find_boards: blobs=True has neither refinement nor levels")
        if levels or not refine:
            return self.find_boards_collect(self.find_boards_submit(frames, gridn, image_pyramid_level, nthreads, refine, levels))
        fr, B, H, W = self._frames(frames)
        boards = np.full((B, gridn * gridn, 2), np.nan, dtype=np.float64)
        found = np.full((B,), -1, dtype=np.int8)
        t.cuda.current_stream(frames.device).synchronize()
        if blobs:
            self._check(self.L.mrgingham_amd_find_circle_grids_batch(self.ctx, ctypes.byref(fr), int(gridn),
                                                                     boards.ctypes.data, found.ctypes.data, int(nthreads)))
            return boards, found
        self._check(self.L.mrgingham_amd_find_boards_batch(self.ctx, ctypes.byref(fr), int(gridn),
                                                           int(image_pyramid_level), boards.ctypes.data,
                                                           found.ctypes.data, int(nthreads)))
        return boards, found

    def find_boards_submit(self, frames, gridn=10, image_pyramid_level=-1, nthreads=0, refine=True, levels=False):
        """First half of find_boards: queues the device passes of the batch and returns a job to hand to
        find_boards_collect.  Submit the next batch(es) before collecting this one and the device passes, the host's
        grid finder and the refinement of consecutive batches overlap (include/mrgingham_amd.h).  refine / levels: as
        find_boards; with levels=True find_boards_collect returns the third array."""
        t = self.torch
        fr, B, H, W = self._frames(frames)
        boards = np.full((B, gridn * gridn, 2), np.nan, dtype=np.float64)
        found = np.full((B,), -1, dtype=np.int8)
        lv = np.zeros((B, gridn * gridn), dtype=np.int8) if levels else None
        t.cuda.current_stream(frames.device).synchronize()
        if levels or not refine:
            ticket = self.L.mrgingham_amd_find_boards_submit_ex(self.ctx, ctypes.byref(fr), int(gridn), int(image_pyramid_level),
                                                                int(bool(refine)), boards.ctypes.data,
                                                                lv.ctypes.data if levels else None, found.ctypes.data, int(nthreads))
        else:
            ticket = self.L.mrgingham_amd_find_boards_submit(self.ctx, ctypes.byref(fr), int(gridn), int(image_pyramid_level),
                                                             boards.ctypes.data, found.ctypes.data, int(nthreads))
        if ticket < 0:
            self._check(ticket)
        # The library writes into `boards` / `found` (and reads `frames`) until the job is complete -- from inside ANY later
        # call on this context.  The Detector holds them until then, so a caller that drops the job tuple without
        # collecting it cannot make the library write into freed memory.
        self._fb_live[ticket] = (boards, found, frames, lv)
        if len(self._fb_live) > 64:            # jobs nobody collected: complete what is in flight, then let the old ones go
            self.find_boards_stats(reset=False)   # (completes every batch in flight: their outputs are final)
            for tk in sorted(self._fb_live)[:-8]:
                del self._fb_live[tk]
        return (ticket, boards, found, frames, lv) if levels else (ticket, boards, found, frames)

    def find_boards_collect(self, job):
        """Second half: waits for the job -> (boards float64 [B, gridn*gridn, 2], found_level int8 [B]), and the
        corners' levels int8 [B, gridn*gridn] when the job was submitted with levels=True."""
        try:
            self._check(self.L.mrgingham_amd_find_boards_collect(self.ctx, job[0]))
        finally:
            self._fb_live.pop(job[0], None)
        return (job[1], job[2], job[4]) if len(job) > 4 else (job[1], job[2])

    def find_grids(self, xy, counts, gridn=10, out=None, sync=True):
        """The grid finder on the device (mrgingham_amd_find_grids_batch): candidate lists as detect() leaves them -- xy
        int32 [nlists, capacity, 2], counts int32 [nlists], on the device -- to (index int32 [nlists, gridn * gridn],
        status int32 [nlists]) on the device: candidate indices in board order (-1 where there is no board) and 1 = board
        found, 0 = none, below 0 = declined (GRID_DECLINES): the list is the host finder's.  boards_of_indices turns them
        into corners.  One launch, one workgroup per list.  `out` = (index, status) to write into; queued and ordered like
        detect(out=): after_stream() in front where torch work still queued produces the lists, and with sync=False
        stream_wait() or sync() before anybody reads the results."""
        t = self.torch
        assert xy.dtype == t.int32 and counts.dtype == t.int32 and xy.is_cuda and counts.is_cuda
        assert xy.dim() == 3 and xy.shape[2] == 2 and xy.is_contiguous() and counts.is_contiguous() and counts.shape == (xy.shape[0],)
        nlists, capacity = xy.shape[0], xy.shape[1]
        if out is None:
            index = t.empty((nlists, gridn * gridn), dtype=t.int32, device=xy.device)
            status = t.empty((nlists,), dtype=t.int32, device=xy.device)
            t.cuda.current_stream(xy.device).synchronize()  # inputs/outputs ready before the ctx streams run
        else:
            index, status = out
            assert index.dtype == t.int32 and status.dtype == t.int32 and index.is_contiguous() and status.is_contiguous()
            assert index.shape == (nlists, gridn * gridn) and status.shape == (nlists,)
        self._check(self.L.mrgingham_amd_find_grids_batch(self.ctx, xy.data_ptr(), counts.data_ptr(), nlists, capacity, int(gridn),
                                                          index.data_ptr(), status.data_ptr()))
        if sync:
            self.sync()
        return index, status

    FIND_GRIDS_STATS = ("lists", "found", "none", "declined_count", "declined_ring", "declined_guard", "declined_table",
                        "declined_coordinate", "host_fallbacks")

    def find_grids_stats(self, reset=True):
        """mrgingham_amd_find_grids_stats as a dict: lists the device grid finder has answered since the last reset (in
        find_grids and in find_boards under option "find_boards_grid"), by status, and the lists of find_boards jobs the
        host finder answered because the device had declined them.  Synchronises."""
        out = np.zeros(len(self.FIND_GRIDS_STATS), dtype=np.float64)
        n = self.L.mrgingham_amd_find_grids_stats(self.ctx, out.ctypes.data, len(out), int(bool(reset)))
        if n < 0:
            self._check(n)
        return dict(zip(self.FIND_GRIDS_STATS, out.tolist()))

    FB_STATS = ("batches", "host_threads", "ms_submit_checks", "ms_submit_prev_host_begin", "ms_submit_device_queued",
                "ms_grid_finder_joined", "ms_refinement_queued", "ms_collect_wait_refinement", "ms_collect_boards_copied",
                "grid_calls", "grid_found", "grid_us_graph", "grid_us_adjacency", "grid_us_sequences", "grid_us_cycles_rows",
                "device_ms_first_pass", "device_ms_refinement")

    def find_boards_stats(self, reset=True):
        """mrgingham_amd_find_boards_stats as a dict (totals since the last reset; completes the batches in flight)."""
        out = np.zeros(len(self.FB_STATS), dtype=np.float64)
        n = self.L.mrgingham_amd_find_boards_stats(self.ctx, out.ctypes.data, len(out), int(bool(reset)))
        if n < 0:
            self._check(n)
        return dict(zip(self.FB_STATS, out.tolist()))

    def sparse_fallbacks(self):
        """Frames the sparse refinement (option "sparse_refine") handed back to the dense kernels since the last
        call of this method; the library repeats them inside the call that met them.  Synchronises."""
        n = self.L.mrgingham_amd_sparse_fallbacks(self.ctx)
        if n < 0:
            self._check(n)
        return n

    def debug_paths(self, level, nframes):
        """Test hook: per frame of the most recent call at `level`, 1 = component search out of LDS, 0 = the
        global-memory kernels."""
        out = np.zeros((nframes,), dtype=np.int32)
        self._check(self.L.mrgingham_amd_debug_paths(self.ctx, int(level), int(nframes), out.ctypes.data))
        return out

    PIXELS_CHAIN, PIXELS_LEVEL, PIXELS_RESPONSE = 0, 1, 2

    def pixel_products(self, frames, level=3, mode="chain", max_points=1024):
        """Test hook (mrgingham_amd_debug_pixel_stage / _debug_pixel_products): runs the PIXEL STAGE alone of
        chain(frames, level) (mode "chain"), of detect(frames, level) ("level"), or of cc_detect_on_response(frames, ..)
        ("response": `frames` is the int16 response [B,h,w]) -- no component search -- and returns what that stage hands
        over, as numpy arrays: {level: {"w", "h", "cap", and where they are products of the stage "image" u8 [B,h,w],
        "response" i16 [B,h,w], "hot_cnt" i32 [B] (entries made: may exceed cap), "hot_xy" a list of B u32 arrays of
        min(hot_cnt, cap) entries (y << 16) | x, "gidx" u32 [B,h,gw,2] (first index, mask: only the pairs of groups with
        a hot pixel are ever written)}}."""
        t = self.torch
        mode = {"chain": self.PIXELS_CHAIN, "level": self.PIXELS_LEVEL, "response": self.PIXELS_RESPONSE}[mode]
        if mode == self.PIXELS_RESPONSE:
            assert frames.dtype == t.int16 and frames.is_cuda and frames.is_contiguous() and frames.dim() == 3
            B, H, W = frames.shape
            fr, resp, level = _lib.Frames(None, 0, B, W, H, W), frames.data_ptr(), 0
        else:
            (fr, B, H, W), resp = self._frames(frames), None
        t.cuda.current_stream(frames.device).synchronize()
        self._check(self.L.mrgingham_amd_debug_pixel_stage(self.ctx, mode, ctypes.byref(fr), int(level), int(max_points), resp))
        out = {}
        for L in (range(level + 1) if mode == self.PIXELS_CHAIN else (level,)):
            w, h = level_dims(W, H, L)
            gw = (w + 7) // 8
            p = {"w": w, "h": h}
            cnt, cap = ctypes.c_int32(), ctypes.c_int32()
            img = np.empty((B, h, w), np.uint8)
            lists = self.L.mrgingham_amd_debug_pixel_products(self.ctx, L, 0, None, None, None, ctypes.byref(cap), None, None) == 0
            if self.L.mrgingham_amd_debug_pixel_products(self.ctx, L, 0, img.ctypes.data, None, None, None, None, None) == 0:
                p["image"] = img
            if lists:
                p.update(cap=cap.value, response=np.empty((B, h, w), np.int16), hot_cnt=np.empty(B, np.int32), hot_xy=[],
                         gidx=np.empty((B, h, gw, 2), np.uint32))
            for f in range(B):
                if "image" in p:
                    self._check(self.L.mrgingham_amd_debug_pixel_products(self.ctx, L, f, img[f].ctypes.data, None, None, None, None, None))
                if lists:
                    self._check(self.L.mrgingham_amd_debug_pixel_products(self.ctx, L, f, None, None, ctypes.byref(cnt), None, None, None))
                    xy = np.empty(max(0, min(cnt.value, cap.value)), np.uint32)
                    self._check(self.L.mrgingham_amd_debug_pixel_products(
                        self.ctx, L, f, None, p["response"][f].ctypes.data, ctypes.byref(cnt), ctypes.byref(cap), xy.ctypes.data,
                        p["gidx"][f].ctypes.data))
                    p["hot_cnt"][f] = cnt.value
                    p["hot_xy"].append(xy)
            out[L] = p
        return out

    def debug_refine_clock(self):
        """Phase clock of the most recent refinement (option cc_lds = 1 | 512): 12 int64, see the header."""
        out = np.zeros(12, dtype=np.int64)
        self._check(self.L.mrgingham_amd_debug_refine_clock(self.ctx, out.ctypes.data))
        return out

    def chain_info(self):
        """(fused_pyramid, merged_levels) of the most recent chain() call: whether the level-0 response kernel
        also wrote the level images, and how many levels shared one response launch."""
        f, m = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self.L.mrgingham_amd_chain_info(self.ctx, ctypes.byref(f), ctypes.byref(m)))
        return bool(f.value), int(m.value)

    def scratch_bytes(self):
        """Device memory the context holds right now."""
        return int(self.L.mrgingham_amd_scratch_bytes(self.ctx))

    def set_kernel_timing(self, enable):
        """True / 1: hipEvents around the level-0 response launches + the engine-clock probe; 2: the probe alone; False: off."""
        self.L.mrgingham_amd_set_kernel_timing(self.ctx, int(enable))

    def sclk_mhz(self):
        """Engine clock (MHz) the level-0 response launches since the last call ran at (kernel timing on); 0.0 = none probed."""
        return float(self.L.mrgingham_amd_sclk_mhz(self.ctx))

    def chess_kernel_ms(self):
        n = ctypes.c_int()
        ms = self.L.mrgingham_amd_chess_kernel_ms(self.ctx, ctypes.byref(n))
        return ms, n.value
