"""A TIFF writer for the tests of the TIFF reader and its device route (read_image, probe_image, tiff_layout,
Detector.tiff_decode / read_tiffs, find_boards_files(tiff="device")): both byte orders, any RowsPerStrip, strips in any
file order and at odd offsets, no compression / LZW / PackBits / Deflate, predictor 2, extra samples, WhiteIsZero -- and
the pieces to assemble files that break a rule.  TIFF here is lossless: the array handed to the writer is the yardstick for
whatever reads the file back (test_tiff_io.py checks the writer itself against Pillow's libtiff).

The LZW encoder is TIFF's: MSB-first codes, ClearCode 256, EOI 257, and the width grows when the encoder's next free code
reaches 512, 1024, 2048 (one code "early" for the decoder, whose table lags one entry behind); it clears at 4094."""
import struct
import zlib

import numpy as np

BYTE, SHORT, LONG = 1, 3, 4
SIZE = {BYTE: 1, SHORT: 2, LONG: 4}
NONE, LZW, PACKBITS, DEFLATE, ADOBE_DEFLATE = 1, 5, 32773, 32946, 8


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, width):
        self.acc = (self.acc << width) | code
        self.n += width
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 255)
        return bytes(self.out)


def pack_codes(codes):
    """[(code, width), ...] -> bytes: a stream made by hand."""
    w = BitWriter()
    for c, n in codes:
        w.put(c, n)
    return w.done()


def lzw_encode(data, open_with_clear=True, never_clear=False, trailing=b"", stats=None):
    """data -> one LZW strip.  never_clear: the table fills and stays full (a stream this library calls unreadable once a
    code follows the full table).  stats: a dict that receives codes / clears / widths."""
    w = BitWriter()
    width, nxt, table = 9, 258, {}
    ncodes, nclears, widths = 0, 0, set()

    def emit(code):
        nonlocal ncodes
        w.put(code, width)
        widths.add(width)
        ncodes += 1

    if open_with_clear:
        emit(256)
    prefix = None
    for b in data:
        if prefix is None:
            prefix = b
            continue
        key = (prefix, b)
        if key in table:
            prefix = table[key]
            continue
        emit(prefix)
        if nxt < 4096:
            table[key] = nxt
            nxt += 1
        if nxt in (512, 1024, 2048):
            width += 1
        if nxt == 4094 and not never_clear:
            emit(256)
            nclears += 1
            width, nxt, table = 9, 258, {}
        prefix = b
    if prefix is not None:
        emit(prefix)
        nxt += 1
        if nxt in (512, 1024, 2048):
            width += 1
    emit(257)
    if stats is not None:
        stats.update(codes=ncodes, clears=nclears, widths=sorted(widths))
    return w.done() + trailing


def packbits_encode(row):
    """One row, literal runs of up to 128 and repeats of up to 128."""
    out, i, n = bytearray(), 0, len(row)
    while i < n:
        j = i
        while j + 1 < n and row[j + 1] == row[i] and j - i < 127:
            j += 1
        if j > i:
            out += bytes([257 - (j - i + 1), row[i]])
            i = j + 1
            continue
        j = i
        while j + 1 < n and (j + 2 >= n or row[j + 1] != row[j + 2]) and j - i < 127:
            j += 1
        out += bytes([j - i]) + bytes(row[i:j + 1])
        i = j + 1
    return bytes(out)


def random_image(width, height, samples, bits, seed=0):
    """Smooth ramps plus noise, uint8 / uint16 [H, W] or [H, W, samples]."""
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1
    y, x = np.mgrid[0:height, 0:width]
    planes = [((x * (3 + k) + y * (5 - k)) * (top // 97) + rng.integers(0, top // 3 + 1, (height, width))) % (top + 1) for k in range(samples)]
    img = np.stack(planes, axis=-1).astype(np.uint8 if bits == 8 else np.uint16)
    return img[:, :, 0] if samples == 1 else img


def grey_of(img, photometric):
    """What the library makes of the image handed to the writer: the first sample, or -- photometric 2 -- the weighted first
    three (png_cases.grey_of's weights); further samples are ignored.  (WhiteIsZero is the writer's business: it stores
    maxval - v, so the file reads back as the array.)"""
    if img.ndim == 2:
        return img
    if photometric != 2:
        return img[:, :, 0]
    v = img.astype(np.uint64)
    return ((v[:, :, 0] * 4899 + v[:, :, 1] * 9617 + v[:, :, 2] * 1868 + 8192) >> 14).astype(img.dtype)


def strip_rows(img, y0, y1, order, predictor, photometric):
    """Rows [y0, y1) as they go into the compressor: uint8 [rows, rowbytes]."""
    a = img[y0:y1].reshape(y1 - y0, img.shape[1], -1)
    bits = 8 * a.dtype.itemsize
    if photometric == 0:
        a = ((1 << bits) - 1 - a.astype(np.int64)).astype(a.dtype)
    if predictor == 2:
        d = a.astype(np.int64)
        d[:, 1:] -= a[:, :-1].astype(np.int64)
        a = (d & ((1 << bits) - 1)).astype(a.dtype)
    raw = a.astype((order + "u2") if bits == 16 else np.uint8).tobytes()
    return np.frombuffer(raw, np.uint8).reshape(y1 - y0, -1)


def compress(rows, compression, **lzw):
    if compression == NONE:
        return rows.tobytes()
    if compression == LZW:
        return lzw_encode(rows.tobytes(), **lzw)
    if compression == PACKBITS:
        return b"".join(packbits_encode(r.tobytes()) for r in rows)
    return zlib.compress(rows.tobytes(), 6)


def encode(img, order="<", compression=NONE, predictor=1, rows_per_strip=None, rps_tag="same", photometric=None,
           reverse=False, odd=False, tags=None, strip_bytes=None, magic=42, lzw=None):
    """-> (the file's bytes, [(offset, nbytes, first_row, rows), ...] as laid out).  img: uint8 / uint16 [H, W] or
    [H, W, samples].  rows_per_strip None: one strip and no RowsPerStrip tag; rps_tag: the value written into the tag where
    it differs from the rows actually put into a strip (2**32 - 1, or anything above the height, with rows_per_strip None).
    reverse: the strips lie in reverse order in the file; odd: every strip begins at an odd offset.  tags: {tag: (type,
    [values]) to add or replace, None to leave out, ("raw", type, count, value_field) to write an entry as it stands}.
    strip_bytes: the compressed strips, made by hand.  lzw: keyword arguments of lzw_encode."""
    h, w = img.shape[:2]
    samples = 1 if img.ndim == 2 else img.shape[2]
    bits = 8 * img.dtype.itemsize
    if photometric is None:
        photometric = 2 if samples >= 3 else 1
    rps = h if rows_per_strip is None else min(rows_per_strip, h)
    spans = [(y, min(y + rps, h)) for y in range(0, h, rps)]
    if strip_bytes is None:
        strip_bytes = [compress(strip_rows(img, a, b, order, predictor, photometric), compression, **(lzw or {})) for a, b in spans]
    body, where = bytearray(), [None] * len(spans)
    for i in (reversed(range(len(spans))) if reverse else range(len(spans))):
        if (8 + len(body)) % 2 == (1 if not odd else 0):
            body += b"\0"
        where[i] = 8 + len(body)
        body += strip_bytes[i]
    strips = [(where[i], len(strip_bytes[i]), a, b - a) for i, (a, b) in enumerate(spans)]
    entries = {256: (LONG, [w]), 257: (LONG, [h]), 258: (SHORT, [bits] * samples), 259: (SHORT, [compression]),
               262: (SHORT, [photometric]), 273: (LONG, where), 277: (SHORT, [samples]), 279: (LONG, [len(s) for s in strip_bytes]),
               284: (SHORT, [1])}
    if rows_per_strip is not None or rps_tag != "same":
        entries[278] = (LONG, [rps if rps_tag == "same" else rps_tag])
    if predictor != 1:
        entries[317] = (SHORT, [predictor])
    nextra = samples - (3 if photometric == 2 else 1)
    if nextra > 0:
        entries[338] = (SHORT, [2 if photometric == 2 and nextra == 1 else 0] * nextra)  # (RGB + one: unassociated alpha)
    for tag, v in (tags or {}).items():
        if v is None:
            entries.pop(tag, None)
        else:
            entries[tag] = v
    fmt = {BYTE: "B", SHORT: "H", LONG: "I"}
    extra = bytearray()
    base = 8 + len(body)
    if base % 2:
        body += b"\0"
        base += 1
    ifd = bytearray()
    for tag in sorted(entries):
        v = entries[tag]
        if v[0] == "raw":
            ifd += struct.pack(order + "HHI", tag, v[1], v[2]) + struct.pack(order + "I", v[3])
            continue
        typ, vals = v
        data = struct.pack(order + fmt[typ] * len(vals), *vals)
        if len(data) <= 4:
            field = data.ljust(4, b"\0")
        else:
            field = struct.pack(order + "I", base + len(extra))
            extra += data + (b"\0" if len(data) % 2 else b"")
        ifd += struct.pack(order + "HHI", tag, typ, len(vals)) + field
    ifd_at = base + len(extra)
    head = (b"II" if order == "<" else b"MM") + struct.pack(order + "HI", magic, ifd_at)
    return head + bytes(body) + bytes(extra) + struct.pack(order + "H", len(entries)) + bytes(ifd) + struct.pack(order + "I", 0), strips


def write(path, img, **kw):
    data, strips = encode(img, **kw)
    with open(path, "wb") as f:
        f.write(data)
    return strips


# the crafted LZW strips share one size with noise(): a batch can hold them next to good files
CRAFT_W, CRAFT_H = 67, 131


def noise():
    return np.random.default_rng(5).integers(0, 256, (CRAFT_H, CRAFT_W)).astype(np.uint8)


def broken_lzw_strips():
    """{name: bytes of the one strip of a 67 x 131 8-bit grey file} -- one rule of the LZW decoder broken in each."""
    good = lzw_encode(noise().tobytes())
    return {
        "lzw_code_above_next": pack_codes([(256, 9), (65, 9), (66, 9), (300, 9)] + [(65, 9)] * 40),
        "lzw_early_eoi": pack_codes([(256, 9), (65, 9), (66, 9), (257, 9)] + [(65, 9)] * 40),
        "lzw_cut_short": good[:len(good) // 2],
        "lzw_table_full": lzw_encode(noise().tobytes(), never_clear=True),
    }


def broken_files():
    """-> ({name: (bytes, in_header)}, a good file, its image): files that break one rule each.  in_header: the fault lies in
    the directory (probe_image and tiff_layout call the file unreadable as well); else only decoding finds it."""
    img = random_image(9, 7, 1, 8, seed=3)
    rgb = random_image(9, 7, 3, 8, seed=4)
    good, _ = encode(img, rows_per_strip=3)
    out = {}

    def header(name, data):
        out[name] = (data, True)

    header("truncated_ifd", good[:-20])
    header("offset_past_end", encode(img, rows_per_strip=3, tags={273: ("raw", LONG, 3, len(good) + 64)})[0])
    header("count_past_end", encode(img, rows_per_strip=3, tags={273: ("raw", LONG, 4000, 8)})[0])
    header("count_size_overflow", encode(img, rows_per_strip=3, tags={258: ("raw", LONG, 0x40000001, 8)})[0])
    header("zero_side", encode(img, tags={256: (LONG, [0])})[0])
    header("side_32768", encode(img, tags={257: (LONG, [32768])})[0])
    header("bits_4", encode(img, tags={258: (SHORT, [4])})[0])
    header("unequal_bits", encode(rgb, tags={258: (SHORT, [8, 8, 16])})[0])
    header("planar_2", encode(rgb, tags={284: (SHORT, [2])})[0])
    header("tiles", encode(img, tags={322: (SHORT, [16]), 323: (SHORT, [16])})[0])
    header("palette", encode(img, tags={262: (SHORT, [3]), 320: (SHORT, [0] * 768)})[0])
    header("bigtiff_magic", encode(img, magic=43)[0])
    header("orientation_6", encode(img, tags={274: (SHORT, [6])})[0])
    header("predictor_3", encode(img, tags={317: (SHORT, [3])})[0])
    header("strip_past_end", encode(img, tags={279: (LONG, [len(good) + 1])})[0])
    for name, strip in broken_lzw_strips().items():
        out[name] = (encode(noise(), compression=LZW, strip_bytes=[strip])[0], False)
    rows = strip_rows(img, 0, 7, "<", 1, 1)
    over = b"".join(packbits_encode(r.tobytes()) for r in rows[:6]) + bytes([9]) + bytes(10)  # a literal run of 10 in a row of 9
    out["packbits_overrun"] = (encode(img, compression=PACKBITS, strip_bytes=[over])[0], False)
    out["deflate_other_length"] = (encode(img, compression=ADOBE_DEFLATE, strip_bytes=[zlib.compress(rows.tobytes() + b"\0")])[0], False)
    return out, good, img
