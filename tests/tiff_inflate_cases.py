"""Deflate streams for the tests of the TIFF Deflate strip decoder (csrc/tiff_inflate.h and its kernel): a bit writer for
stored, fixed and dynamic blocks with the zlib wrapper around them, a block walker that says what a stream holds, and the
lists every test draws from -- the sanitizer program of test_tiff_inflate.py and the device tests of
test_gpu_tiff_inflate.py walk the same ones.  zlib is the judge of every stream here; nothing in this module decides what is
accepted."""
import struct
import zlib

import numpy as np

from tests import tiff_cases as tc

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
# a complete code-length code that has every symbol: 0..15 in five bits, 16 in two, 17 and 18 in three
CL_ALL = [5] * 16 + [2, 3, 3]


class BitOut:
    """Deflate's bit order: values LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):
        code, length = c
        for i in reversed(range(length)):
            self.bits((code >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """[length per symbol] -> {symbol: (code, length)}, RFC 1951 3.2.2 (whatever the lengths: a set that is not a prefix
    code gets the codes the rule gives it)."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n] & ((1 << n) - 1), n)
            nxt[n] += 1
    return out


def complete_lens(symbols, size):
    """Lengths of a complete code over `symbols` (two or more), zero for the rest of `size` symbols."""
    k = len(symbols)
    p = max(1, (k - 1).bit_length())
    short = (1 << p) - k
    lens = [0] * size
    for i, s in enumerate(sorted(symbols)):
        lens[s] = p - 1 if i < short else p
    return lens


def put_tokens(w, toks, lit, dist):
    """A token: a literal byte; (length, distance); ("L", symbol) a bare literal/length code; ("D", symbol) a bare
    distance code."""
    for t in toks:
        if isinstance(t, int):
            w.code(lit[t])
        elif t[0] == "L":
            w.code(lit[t[1]])
        elif t[0] == "D":
            w.code(dist[t[1]])
        else:
            length, d = t
            i = max(k for k in range(29) if LBASE[k] <= length)
            w.code(lit[257 + i])
            w.bits(length - LBASE[i], LEXTRA[i])
            j = max(k for k in range(30) if DBASE[k] <= d)
            w.code(dist[j])
            w.bits(d - DBASE[j], DEXTRA[j])


def stored(w, data, final, nlen=None):
    w.bits(final, 1)
    w.bits(0, 2)
    w.align()
    w.out += struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + data


def fixed(w, toks, final, end=True):
    w.bits(final, 1)
    w.bits(1, 2)
    lit = canonical(FIXED_LIT)
    put_tokens(w, toks, lit, canonical(FIXED_DIST))
    if end:
        w.code(lit[256])


def dynamic_header(w, final, hlit, hdist, cl_lens, cl_syms):
    """cl_lens: the 19 lengths of the code-length code; cl_syms: [(symbol, value of its extra bits)]."""
    w.bits(final, 1)
    w.bits(2, 2)
    w.bits(hlit, 5)
    w.bits(hdist, 5)
    w.bits(15, 4)
    for s in CL_ORDER:
        w.bits(cl_lens[s], 3)
    cl = canonical(cl_lens)
    for s, extra in cl_syms:
        w.code(cl[s])
        w.bits(extra, {16: 2, 17: 3, 18: 7}.get(s, 0))


def dynamic(w, toks, final, lit_lens, dist_lens, end=True):
    """lit_lens: 257..286 lengths, dist_lens: 1..30; every length written plainly with CL_ALL."""
    dynamic_header(w, final, len(lit_lens) - 257, len(dist_lens) - 1, CL_ALL, [(n, 0) for n in lit_lens + dist_lens])
    lit = canonical(lit_lens)
    put_tokens(w, toks, lit, canonical(dist_lens))
    if end:
        w.code(lit[256])


def wrap(raw, data, cmf=0x78, fdict=0, fcheck=None, adler=None):
    """The zlib wrapper around a raw stream that gives `data`."""
    flg = 0x20 if fdict else 0
    flg += (31 - (cmf << 8 | flg) % 31) % 31 if fcheck is None else fcheck
    return bytes([cmf, flg]) + raw + struct.pack(">I", zlib.adler32(data) if adler is None else adler)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, raw=False):
    c = zlib.compressobj(level, zlib.DEFLATED, -15 if raw else 15, 8, strategy)
    return c.compress(data) + c.flush()


def walk(stream, raw=False):
    """What a VALID stream holds: {"kinds": set of 0 / 1 / 2, "repeats": set of 16 / 17 / 18, "max_distance", "max_length",
    "overlap": a copy that reads what it writes, "blocks", "out": the bytes, "end_bit": where the final block ends, in bits
    from the first block's first}."""
    pos = 0 if raw else 16
    src = stream + b"\0\0\0\0"

    def take(n):
        nonlocal pos
        v = (int.from_bytes(src[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def decoder(lens):
        by_len = {}
        for s, (code, n) in canonical(lens).items():
            by_len.setdefault(n, {})[int(format(code, "0%db" % n)[::-1], 2)] = s
        order = sorted(by_len)

        def get():
            nonlocal pos
            v = (int.from_bytes(src[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & 0xFFFF
            for n in order:
                s = by_len[n].get(v & ((1 << n) - 1))
                if s is not None:
                    pos += n
                    return s
            raise ValueError("a code that is not there")
        return get

    info = {"kinds": set(), "repeats": set(), "max_distance": 0, "max_length": 0, "overlap": False, "blocks": 0}
    out = bytearray()
    final = 0
    while not final:
        final, kind = take(1), take(2)
        info["kinds"].add(kind)
        info["blocks"] += 1
        if kind == 0:
            pos = (pos + 7) & ~7
            n = take(16)
            take(16)
            out += src[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
            continue
        if kind == 1:
            lit, dist = decoder(FIXED_LIT), decoder(FIXED_DIST)
        else:
            nlen, ndist, ncode = take(5) + 257, take(5) + 1, take(4) + 4
            cl = [0] * 19
            for i in range(ncode):
                cl[CL_ORDER[i]] = take(3)
            get, lens = decoder(cl), []
            while len(lens) < nlen + ndist:
                s = get()
                if s < 16:
                    lens.append(s)
                    continue
                info["repeats"].add(s)
                if s == 16:
                    lens += [lens[-1]] * (3 + take(2))
                else:
                    lens += [0] * (3 + take(3) if s == 17 else 11 + take(7))
            lit, dist = decoder(lens[:nlen]), decoder(lens[nlen:])
        while True:
            s = lit()
            if s < 256:
                out.append(s)
                continue
            if s == 256:
                break
            length = LBASE[s - 257] + take(LEXTRA[s - 257])
            j = dist()
            d = DBASE[j] + take(DEXTRA[j])
            info["max_distance"] = max(info["max_distance"], d)
            info["max_length"] = max(info["max_length"], length)
            info["overlap"] |= d < length
            for _ in range(length):
                out.append(out[-d])
    info["out"] = bytes(out)
    info["end_bit"] = pos - (0 if raw else 16)
    return info


# ---- the payloads and what zlib makes of them

def ramp_noise(rows, width=300, seed=1):
    """x // 3 plus noise 0..2: low entropy, matches at the distance of a row and further."""
    rng = np.random.default_rng(seed)
    return ((np.arange(width) // 3)[None, :] + rng.integers(0, 3, (rows, width))).astype(np.uint8)


def payloads():
    return [ramp_noise(40).tobytes(), (ramp_noise(60) // 8).astype(np.uint8).tobytes(),
            np.random.default_rng(2).integers(0, 256, 3000).astype(np.uint8).tobytes(), b"ab" * 20, bytes([7]) * 5000]


LEVELS = (0, 1, 6, 9)
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED)


def good_streams():
    """[(stream, is_raw, the bytes it gives)]: every payload x level x strategy, wrapped and raw."""
    out = []
    for data in payloads():
        for level in LEVELS:
            for strategy in STRATEGIES:
                for raw in (False, True):
                    out.append((deflate(data, level, strategy, raw), raw, data))
    return out


def mutations(streams, per_stream=20, seed=11):
    """Of each (stream, is_raw, data) `per_stream` copies with one to three random bytes replaced."""
    rng = np.random.default_rng(seed)
    out = []
    for stream, raw, data in streams:
        for _ in range(per_stream):
            b = bytearray(stream)
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            out.append((bytes(b), raw, data))
    return out


# ---- streams made by hand.  Each is the ONE strip of an 8-bit grey file of `shape` (width, height).

CRAFT_SHAPE = (tc.CRAFT_W, tc.CRAFT_H)


def craft_payload():
    return tc.noise().tobytes()


def crafted_accepted():
    """{name: (zlib stream, the bytes it gives, (width, height))}."""
    out = {}
    lits = np.random.default_rng(3).integers(0, 256, 32768).astype(np.uint8).tobytes()
    w = BitOut()
    fixed(w, list(lits) + [(258, 32768)], 1)
    data = lits + lits[:258]
    out["far_and_long_match"] = (wrap(w.done(), data), data, (337, 98))
    # the same under a header that promises a window of 256 bytes: zlib, not built strict, does not hold a stream to it
    out["window_smaller_than_distance"] = (wrap(w.done(), data, cmf=0x08), data, (337, 98))
    w = BitOut()
    fixed(w, [65, (3, 1)], 1)
    out["length_3_distance_1"] = (wrap(w.done(), b"AAAA"), b"AAAA", (4, 1))
    # literals a, b, the end code and length 3 / 4: a complete set; the only distance code (distance 1) in one bit
    lens = complete_lens([97, 98, 256, 257, 258], 259)
    data = b"ab" + b"b" * 3 + b"a" + b"a" * 4
    w = BitOut()
    dynamic(w, [97, 98, (3, 1), 97, (4, 1)], 1, lens, [1])
    out["one_distance_code_of_one_bit"] = (wrap(w.done(), data), data, (10, 1))
    w = BitOut()
    dynamic(w, list(b"abcabcab"), 1, complete_lens([97, 98, 99, 256], 257), [0])
    out["no_distance_code"] = (wrap(w.done(), b"abcabcab"), b"abcabcab", (8, 1))
    data = craft_payload()
    w = BitOut()
    stored(w, data[:4000], 0)
    stored(w, b"", 0)
    stored(w, data[4000:], 1)
    out["empty_stored_block"] = (wrap(w.done(), data), data, CRAFT_SHAPE)
    ramp = ramp_noise(tc.CRAFT_H, tc.CRAFT_W).tobytes()
    c = zlib.compressobj(6)
    z = c.compress(ramp) + c.flush(zlib.Z_SYNC_FLUSH) + c.flush()
    assert z[-10:-4] == bytes([0, 0, 0xFF, 0xFF, 3, 0])
    out["sync_flush_then_finish"] = (z, ramp, CRAFT_SHAPE)
    out["bytes_behind_trailer"] = (zlib.compress(ramp) + b"xyz", ramp, CRAFT_SHAPE)
    # fixed blocks that follow one another take the tables as they are; a dynamic block in between (its literal/length set
    # the end code alone, in one bit) makes the next fixed block build them again; stored blocks leave them alone
    w = BitOut()
    fixed(w, list(b"abc") + [(3, 3)], 0)
    fixed(w, list(b"de"), 0)
    dynamic(w, [], 0, [0] * 256 + [1], [0])
    fixed(w, [(4, 2)], 0)
    stored(w, b"xyz", 0)
    fixed(w, [(3, 3), 0x71], 1)
    data = b"abcabcde" + b"dede" + b"xyz" + b"xyz" + b"q"
    out["fixed_dynamic_fixed_stored_fixed"] = (wrap(w.done(), data), data, (19, 1))
    z = with_empty_blocks(ramp, 700)
    assert len(z) <= max_bytes(len(ramp))
    out["empty_blocks_within_the_byte_limit"] = (z, ramp, CRAFT_SHAPE)
    return out


def max_bytes(decoded):
    """The bytes of a strip up to which the device route takes it (csrc/tiff_inflate.h: tiff_inflate_max_bytes)."""
    return decoded + decoded // 8 + 512


def with_empty_blocks(data, n):
    """A zlib stream that gives `data` and then goes through n empty fixed blocks, 10 bits each, to the final one: zlib
    accepts it whatever n is; the device route takes it while its bytes stay within max_bytes."""
    raw = deflate(data, level=9, raw=True)
    info = walk(raw, raw=True)
    assert info["blocks"] == 1 and info["out"] == data
    whole, rest = divmod(info["end_bit"], 8)
    # zlib's one block with its final bit cleared, to the bit where it ends; the empty blocks go on from there
    w = BitOut()
    w.out += bytes([raw[0] & 0xFE]) + raw[1:whole]
    if rest:
        w.acc, w.n = raw[whole] & ((1 << rest) - 1), rest
    for k in range(n):
        fixed(w, [], 1 if k == n - 1 else 0)
    return wrap(w.done(), data)


def broken_streams():
    """{name: zlib stream}: one rule broken in each; the one strip of a CRAFT_SHAPE file."""
    data = craft_payload()
    ramp = ramp_noise(tc.CRAFT_H, tc.CRAFT_W).tobytes()
    good = zlib.compress(ramp, 6)
    body = good[2:-4]
    out = {
        "header_cm_7": wrap(body, ramp, cmf=0x77),
        "header_fcheck": wrap(body, ramp, fcheck=(good[1] + 1) & 31),
        "header_fdict": wrap(body, ramp, fdict=1),
        "header_cinfo_8": wrap(body, ramp, cmf=0x88),
        "input_cut_in_block": good[:len(good) // 2],
        "input_cut_in_trailer": good[:-2],
        "wrong_adler": good[:-1] + bytes([good[-1] ^ 1]),
        "one_byte_more": zlib.compress(ramp + b"\0", 6),
        "one_byte_fewer": zlib.compress(ramp[:-1], 6),
    }

    def hand(name, fill):
        w = BitOut()
        fill(w)
        out[name] = wrap(w.done(), data)

    def block_type_3(w):
        stored(w, data[:100], 0)
        w.bits(1, 1)
        w.bits(3, 2)
    hand("block_type_3", block_type_3)
    hand("stored_len_nlen", lambda w: stored(w, data, 1, nlen=len(data) ^ 0xFFFE))
    plain = complete_lens([97, 98, 256], 257)
    hand("hlit_287", lambda w: dynamic_header(w, 1, 30, 0, CL_ALL, [(n, 0) for n in plain + [0] * 30 + [0]]))
    hand("hdist_31", lambda w: dynamic_header(w, 1, 0, 30, CL_ALL, [(n, 0) for n in plain + [5] * 31]))
    hand("cl_oversubscribed", lambda w: dynamic_header(w, 1, 0, 0, [1, 1, 1] + [0] * 16, [(0, 0)] * 258))
    hand("cl_incomplete", lambda w: dynamic_header(w, 1, 0, 0, [1] + [0] * 18, [(0, 0)] * 258))
    hand("repeat_16_first", lambda w: dynamic_header(w, 1, 0, 0, CL_ALL, [(16, 0)] + [(1, 0)] * 255))
    hand("repeat_over_the_end", lambda w: dynamic_header(w, 1, 0, 0, CL_ALL, [(1, 0), (1, 0), (18, 127), (18, 127)]))

    def no_end(w):
        lens = complete_lens([97, 98], 257)
        dynamic(w, [97, 98], 1, lens, [0], end=False)
    hand("no_end_of_block", no_end)

    def lit_over(w):
        lens = [0] * 257
        lens[97] = lens[98] = lens[256] = 1
        dynamic(w, [97, 98], 1, lens, [0])
    hand("lit_oversubscribed", lit_over)

    def lit_incomplete(w):
        lens = [0] * 257
        lens[97] = lens[256] = 2
        dynamic(w, [97, 97], 1, lens, [0])
    hand("lit_incomplete_two_codes", lit_incomplete)
    hand("distance_beyond_start", lambda w: fixed(w, [65, (3, 2)] + list(data), 1))
    hand("literal_length_symbol_286", lambda w: fixed(w, [65, ("L", 286)] + list(data), 1))
    hand("distance_symbol_30", lambda w: fixed(w, [65, ("L", 257), ("D", 30)] + list(data), 1))
    return out


def craft_file(stream, shape=CRAFT_SHAPE, compression=tc.ADOBE_DEFLATE):
    """The 8-bit grey file of one strip around a stream."""
    w, h = shape
    return tc.encode(np.zeros((h, w), np.uint8), compression=compression, strip_bytes=[stream])[0]


# ---- whole images for the device tests

def deflate_file(img, level=6, compression=tc.ADOBE_DEFLATE, **kw):
    """tc.encode with every strip compressed at `level` -> (file, [the strips' streams])."""
    h = img.shape[0]
    rps = min(kw.get("rows_per_strip") or h, h)
    bits = 8 * img.dtype.itemsize
    samples = 1 if img.ndim == 2 else img.shape[2]
    photometric = kw.get("photometric")
    if photometric is None:
        photometric = 2 if samples >= 3 else 1
    streams = [zlib.compress(tc.strip_rows(img, y, min(y + rps, h), kw.get("order", "<"), kw.get("predictor", 1), photometric).tobytes(), level)
               for y in range(0, h, rps)]
    assert bits in (8, 16)
    return tc.encode(img, compression=compression, strip_bytes=streams, **kw)[0], streams


def block_kind_images():
    """[(name, 300 x 300 image, zlib level)]: dynamic blocks with far matches, the same at level 9, one long overlapping
    run, stored blocks."""
    ramp = ramp_noise(300)
    return [("ramp", ramp, 6), ("ramp_over_8", (ramp // 8).astype(np.uint8), 9), ("constant", np.full((300, 300), 7, np.uint8), 6),
            ("noise", np.random.default_rng(4).integers(0, 256, (300, 300)).astype(np.uint8), 6)]


def fixed_block_rows():
    """A 40 x 6 image whose rows, a strip each, zlib writes as fixed blocks."""
    rows = [b"ab" * 20, b"abc" * 13 + b"a", bytes([5]) * 40, b"abcd" * 10, b"ab" * 20, b"xyxz" * 10]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(6, 40).copy()
