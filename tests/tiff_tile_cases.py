"""A tiled TIFF writer for the tests of the tile reader and its device route (read_image, probe_image,
tiff_layout(tiles=True), Detector.tiff_decode / read_tiffs, find_boards_files(tiff="device")), on the helpers of
tests/tiff_cases.py: any tile width and length, both byte orders, no compression / LZW / PackBits / Deflate, predictor 2
(along each row of a tile), 1 to 4 samples, WhiteIsZero, tiles in reverse file order and at odd offsets -- and hooks to
break one rule.  The padding of the edge tiles is RANDOM NON-ZERO bytes (put in before the predictor runs, so the
differences at a tile's right edge are arbitrary too): a reader that leaks padding into the image fails.  TIFF here is
lossless: the array handed to the writer is the yardstick (test_tiff_tiles.py checks the writer itself against Pillow's
libtiff)."""
import struct
import zlib

import numpy as np

from tests import tiff_cases as tc

NONE, LZW, PACKBITS, DEFLATE, ADOBE_DEFLATE = tc.NONE, tc.LZW, tc.PACKBITS, tc.DEFLATE, tc.ADOBE_DEFLATE
BYTE, SHORT, LONG = tc.BYTE, tc.SHORT, tc.LONG


def lzw_literal(data):
    """data -> one LZW strip that compresses nothing, at numpy's speed: every byte as a 9-bit code of its own, a ClearCode
    in front of every 250 of them (the table never reaches the 511 entries at which codes grow to 10 bits), EOI.  A stream
    TIFF's rules allow -- libtiff reads it -- for the large shapes, where tiff_cases.lzw_encode takes a second per MiB."""
    a = np.frombuffer(bytes(data), np.uint8).astype(np.uint16)
    codes = np.append(np.insert(a, np.arange(0, len(a), 250), 256), np.uint16(257))
    bits = ((codes[:, None] >> np.arange(8, -1, -1)) & 1).astype(np.uint8)
    return np.packbits(bits.ravel()).tobytes()


def tile_array(img, tx, ty, tw, tl, rng):
    """Tile (tx, ty) of img padded to [tl, tw(, samples)] with random non-zero samples."""
    h, w = img.shape[:2]
    top = (1 << (8 * img.dtype.itemsize)) - 1
    shape = (tl, tw) + img.shape[2:]
    t = rng.integers(1, top + 1, shape).astype(img.dtype)
    part = img[ty * tl:min((ty + 1) * tl, h), tx * tw:min((tx + 1) * tw, w)]
    t[:part.shape[0], :part.shape[1]] = part
    return t


def encode(img, tw, tl, order="<", compression=NONE, predictor=1, photometric=None, reverse=False, odd=False, tags=None,
           tile_bytes=None, seed=0, lzw=None, literal_lzw=False):
    """-> (the file's bytes, [(offset, nbytes, first_row, rows), ...]: one record per tile, row-major, rows = tl, what
    tiff_layout(tiles=True) reports).  tags: as tiff_cases.encode ({tag: (type, [values]), None to leave out, or ("raw",
    type, count, value_field)}).  tile_bytes: {tile index: compressed bytes made by hand}.  literal_lzw: LZW tiles through
    lzw_literal."""
    h, w = img.shape[:2]
    samples = 1 if img.ndim == 2 else img.shape[2]
    bits = 8 * img.dtype.itemsize
    if photometric is None:
        photometric = 2 if samples >= 3 else 1
    across, down = -(-w // tw), -(-h // tl)
    rng = np.random.default_rng(1000 + seed)
    blobs = []
    for i in range(across * down):
        t = tile_array(img, i % across, i // across, tw, tl, rng)
        rows = tc.strip_rows(t, 0, tl, order, predictor, photometric)
        blobs.append(lzw_literal(rows.tobytes()) if literal_lzw and compression == LZW else tc.compress(rows, compression, **(lzw or {})))
    for i, b in (tile_bytes or {}).items():
        blobs[i] = b
    body, where = bytearray(), [None] * len(blobs)
    for i in (reversed(range(len(blobs))) if reverse else range(len(blobs))):
        if (8 + len(body)) % 2 == (1 if not odd else 0):
            body += b"\0"
        where[i] = 8 + len(body)
        body += blobs[i]
    records = [(where[i], len(blobs[i]), (i // across) * tl, tl) for i in range(len(blobs))]
    entries = {256: (LONG, [w]), 257: (LONG, [h]), 258: (SHORT, [bits] * samples), 259: (SHORT, [compression]),
               262: (SHORT, [photometric]), 277: (SHORT, [samples]), 284: (SHORT, [1]),
               322: (LONG if tw > 65535 else SHORT, [tw]), 323: (LONG if tl > 65535 else SHORT, [tl]), 324: (LONG, where),
               325: (LONG, [len(b) for b in blobs])}
    if predictor != 1:
        entries[317] = (SHORT, [predictor])
    nextra = samples - (3 if photometric == 2 else 1)
    if nextra > 0:
        entries[338] = (SHORT, [2 if photometric == 2 and nextra == 1 else 0] * nextra)
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
    head = (b"II" if order == "<" else b"MM") + struct.pack(order + "HI", 42, ifd_at)
    return head + bytes(body) + bytes(extra) + struct.pack(order + "H", len(entries)) + bytes(ifd) + struct.pack(order + "I", 0), records


def write(path, img, tw, tl, **kw):
    data, records = encode(img, tw, tl, **kw)
    with open(path, "wb") as f:
        f.write(data)
    return records


def photometric_of(kw, img):
    return kw.get("photometric", 2 if img.ndim == 3 and img.shape[2] >= 3 else 1)


def taken(tw, tl, img, compression, lzw_max_strip=0, deflate_max_strip=0):
    """The rule of mrgingham_amd_tiff_layout_tiled for return code 0 (files the writer made: a Deflate tile never exceeds
    tiff_inflate_max_bytes)."""
    tile = tl * tw * (1 if img.ndim == 2 else img.shape[2]) * img.dtype.itemsize
    if tw % 16:
        return False
    if compression == NONE:
        return True
    if compression == LZW:
        return tile <= (lzw_max_strip if 0 < lzw_max_strip <= 1 << 20 else 1 << 20)
    if compression in (DEFLATE, ADOBE_DEFLATE):
        return deflate_max_strip > 0 and tile <= min(deflate_max_strip, 1 << 20)
    return False


def broken_files():
    """-> ({name: (bytes, in_header)}, a good file, its image): tiled files that break one rule each.  in_header: the fault
    lies in the directory (probe_image and tiff_layout(tiles=True) call the file unreadable as well); else only decoding
    finds it."""
    img = tc.random_image(37, 29, 1, 8, seed=21)
    good, recs = encode(img, 16, 16)
    ntiles = len(recs)
    out = {}

    def header(name, data):
        out[name] = (data, True)

    header("counts_one_short", encode(img, 16, 16, tags={325: (LONG, [256] * (ntiles - 1))})[0])
    header("offsets_one_more", encode(img, 16, 16, tags={324: (LONG, [8] * (ntiles + 1))})[0])
    header("tile_offset_past_end", encode(img, 16, 16, tags={324: (LONG, [r[0] for r in recs[:-1]] + [len(good) + 64])})[0])
    header("tile_width_0", encode(img, 16, 16, tags={322: (SHORT, [0])})[0])
    header("tile_length_32768", encode(img, 16, 16, tags={323: (LONG, [32768])})[0])
    header("tiles_beside_strips", encode(img, 16, 16, tags={273: (LONG, [8]), 279: (LONG, [37 * 29])})[0])
    header("tiles_beside_strip_offsets", encode(img, 16, 16, tags={273: (LONG, [8])})[0])
    header("three_of_four_no_counts", encode(img, 16, 16, tags={325: None})[0])
    header("three_of_four_no_width", encode(img, 16, 16, tags={322: None})[0])
    header("uncompressed_one_byte_short", encode(img, 16, 16, tags={325: (LONG, [256] * (ntiles - 1) + [255])})[0])
    # 8 bytes of LZW give at most 8 codes of fewer than 4096 bytes each: a 128 x 512 tile (65536 bytes) cannot come out
    wide = tc.random_image(37, 29, 1, 8, seed=22)
    header("lzw_count_cannot_give_tile", encode(wide, 128, 512, compression=LZW, tile_bytes={0: b"\x80\x00\x00\x00\x00\x00\x00\x00"})[0])
    header("deflate_count_cannot_give_tile", encode(wide, 128, 512, compression=ADOBE_DEFLATE, tile_bytes={0: zlib.compress(b"\0" * 40)})[0])
    header("packbits_count_cannot_give_tile", encode(img, 16, 16, compression=PACKBITS, tile_bytes={1: b"\xf1\x07\xf1"})[0])
    rng = np.random.default_rng(5)
    t3 = tc.strip_rows(tile_array(img, 1, 1, 16, 16, rng), 0, 16, "<", 1, 1)
    out["deflate_one_byte_longer"] = (encode(img, 16, 16, compression=ADOBE_DEFLATE, tile_bytes={4: zlib.compress(t3.tobytes() + b"\x07")})[0], False)
    out["deflate_one_byte_shorter"] = (encode(img, 16, 16, compression=ADOBE_DEFLATE, tile_bytes={4: zlib.compress(t3.tobytes()[:-1])})[0], False)
    cut = tc.lzw_encode(t3.tobytes())
    out["lzw_tile_cut"] = (encode(img, 16, 16, compression=LZW, tile_bytes={2: cut[:len(cut) // 2]})[0], False)
    # a literal run of 17 in a tile row of 16 bytes
    over = b"".join(tc.packbits_encode(r.tobytes()) for r in t3[:15]) + bytes([16]) + bytes(17)
    out["packbits_run_crosses_tile_row"] = (encode(img, 16, 16, compression=PACKBITS, tile_bytes={3: over})[0], False)
    return out, good, img
