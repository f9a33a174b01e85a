"""Binary Netpbm files for the tests of the PBM / PAM reader (tests/test_pnm_io.py, tests/test_gpu_pnm.py): a writer
that shares nothing with the library or with Pillow, the grey a file must read to, and a corpus of files that each break
one rule of the subset (include/mrgingham_amd.h: mrgingham_amd_pnm_header)."""
import numpy as np

# (name, magic, sample bits in the file, channels, black_and_white): every layout the reader takes beyond P5 (P6 stays
# unreadable: tests/test_pgm_header.py pins it; the writer below still writes it, for the files that must not be read)
LAYOUTS = [
    ("p4", 4, 1, 1, False),
    ("p7_grey8", 7, 8, 1, False), ("p7_grey_alpha8", 7, 8, 2, False), ("p7_rgb8", 7, 8, 3, False), ("p7_rgb_alpha8", 7, 8, 4, False),
    ("p7_grey16", 7, 16, 1, False), ("p7_grey_alpha16", 7, 16, 2, False), ("p7_rgb16", 7, 16, 3, False), ("p7_rgb_alpha16", 7, 16, 4, False),
    ("p7_bw", 7, 8, 1, True), ("p7_bw_alpha", 7, 8, 2, True),
]
LAYOUT_IDS = [l[0] for l in LAYOUTS]
TUPLTYPE = {(1, False): "GRAYSCALE", (2, False): "GRAYSCALE_ALPHA", (3, False): "RGB", (4, False): "RGB_ALPHA",
            (1, True): "BLACKANDWHITE", (2, True): "BLACKANDWHITE_ALPHA"}


def grey(r, g, b):
    """the library's one set of grey weights (csrc/png_filter.h: png_grey), on integers or integer arrays"""
    return (np.asarray(r, np.int64) * 4899 + np.asarray(g, np.int64) * 9617 + np.asarray(b, np.int64) * 1868 + 8192) >> 14


def row_bytes(width, bits, channels):
    return (width + 7) // 8 if bits == 1 else width * channels * bits // 8


def default_maxval(bits, bw=False):
    return 1 if bw or bits == 1 else 255 if bits == 8 else 65535


def random_samples(width, height, bits, channels, bw=False, seed=0, maxval=None):
    """samples [h, w, channels]: bits 1 -> 0 / 1 (1 is black); else 0 .. maxval (black and white: 0 / 1)"""
    rng = np.random.default_rng(seed)
    top = default_maxval(bits, bw) if maxval is None else maxval
    return rng.integers(0, top + 1, (height, width, channels)).astype(np.uint16 if bits == 16 else np.uint8)


def expected(samples, bits, channels, bw=False):
    """the grey [h, w] the raster reads to: uint8, or uint16 for 16-bit samples; no rescaling by maxval"""
    s = np.asarray(samples)
    if bits == 1:
        return np.where(s[..., 0] != 0, 0, 255).astype(np.uint8)
    if bw:
        return np.where(s[..., 0] != 0, 255, 0).astype(np.uint8)
    g = s[..., 0] if channels <= 2 else grey(s[..., 0], s[..., 1], s[..., 2])
    return g.astype(np.uint16 if bits == 16 else np.uint8)


def raster(samples, bits):
    """[h, w, c] -> the raster as it lies in a file: rows without padding, bits packed most significant first (the unused
    low bits of a row's last byte are SET: they are nobody's), 16-bit samples as big-endian pairs"""
    s = np.asarray(samples)
    h, w, c = s.shape
    if bits == 1:
        padded = np.ones((h, (w + 7) // 8 * 8), np.uint8)
        padded[:, :w] = s[..., 0]
        return np.packbits(padded, axis=1).tobytes()
    return s.astype(">u2" if bits == 16 else np.uint8).tobytes()


def pnm_head(magic, width, height, maxval=None, sep=b"\n", last=b"\n"):
    """the header of a P4 / P5 / P6 file"""
    nums = [width, height] + ([] if magic == 4 else [maxval])
    return b"P%d" % magic + sep + sep.join(b"%d" % v for v in nums) + last


def pam_head(width, height, depth, maxval, tupltype=None, order=("WIDTH", "HEIGHT", "DEPTH", "MAXVAL"), extra=()):
    """the header of a P7 file: the fields in `order`, `extra` lines (bytes) behind line 1, then TUPLTYPE, ENDHDR"""
    values = {"WIDTH": width, "HEIGHT": height, "DEPTH": depth, "MAXVAL": maxval}
    lines = [b"P7"] + list(extra) + [b"%s %d" % (k.encode(), values[k]) for k in order]
    if tupltype is not None:
        lines.append(b"TUPLTYPE " + tupltype.encode())
    return b"\n".join(lines + [b"ENDHDR"]) + b"\n"


def write(samples, magic, bits, bw=False, maxval=None, head=None):
    """A file of one of the LAYOUTS (or P5 with magic 5).  samples [h, w, c]; head: its header instead of the plain one."""
    s = np.asarray(samples)
    h, w, c = s.shape
    maxval = default_maxval(bits, bw) if maxval is None else maxval
    if head is None:
        head = pam_head(w, h, c, maxval, TUPLTYPE[(c, bw)]) if magic == 7 else pnm_head(magic, w, h, maxval)
    return head + raster(s, bits)


def write_layout(layout, width, height, seed=0, maxval=None):
    """-> (file bytes, the grey it reads to, samples) for an entry of LAYOUTS"""
    _, magic, bits, ch, bw = layout
    s = random_samples(width, height, bits, ch, bw, seed, maxval)
    return write(s, magic, bits, bw, maxval), expected(s, bits, ch, bw), s


# ---- files that break one rule each -----------------------------------------------------------------------------------
def broken_files():
    """-> ({name: bytes}, [good files they are made from])"""
    rgb = random_samples(5, 3, 8, 3, seed=1)
    bits = random_samples(11, 3, 1, 1, seed=2)
    rgba16 = random_samples(5, 3, 16, 4, seed=3)
    one = random_samples(5, 3, 8, 1, bw=True, seed=4)
    p6, good4, good7 = write(rgb, 6, 8), write(bits, 4, 1), write(rgba16, 7, 16)
    body6, body4, body7, body1 = raster(rgb, 8), raster(bits, 1), raster(rgba16, 16), raster(one, 8)
    out = {
        "p6_binary_8_bit": p6,
        "p6_binary_16_bit": write(random_samples(5, 3, 16, 3, seed=5), 6, 16),
        "p6_with_a_comment": b"P6\n# colour\n5 3\n255\n" + body6,
        "p4_raster_one_byte_short": good4[:-1],
        "p7_raster_one_byte_short": good7[:-1],
        "p4_height_0": pnm_head(4, 11, 0) + body4,
        "p4_width_0": pnm_head(4, 0, 3) + body4,
        "p4_width_32768": pnm_head(4, 32768, 1) + bytes(4096),
        "p4_height_32768": pnm_head(4, 1, 32768) + bytes(32768),
        "p7_width_32768": pam_head(32768, 1, 1, 255, "GRAYSCALE") + bytes(32768),
        "p7_maxval_0": pam_head(5, 3, 4, 0, "RGB_ALPHA") + body7,
        "p7_maxval_65536": pam_head(5, 3, 4, 65536, "RGB_ALPHA") + body7,
        "p4_number_too_long": pnm_head(4, 11, 1 << 40) + body4,
        "p4_negative_width": b"P4\n-11 3\n" + body4,
        "p4_letter_in_a_number": b"P4\n11 3x\n" + body4,
        "p4_no_white_space_behind_height": b"P4\n11 3" + b"\xff" + body4,
        "p4_header_only": b"P4\n11 300",
        "p4_header_and_white": b"P4\n11 300\n",
        "p7_no_width": pam_head(5, 3, 4, 65535, "RGB_ALPHA", order=("HEIGHT", "DEPTH", "MAXVAL")) + body7,
        "p7_no_height": pam_head(5, 3, 4, 65535, "RGB_ALPHA", order=("WIDTH", "DEPTH", "MAXVAL")) + body7,
        "p7_no_depth": pam_head(5, 3, 4, 65535, "RGB_ALPHA", order=("WIDTH", "HEIGHT", "MAXVAL")) + body7,
        "p7_no_maxval": pam_head(5, 3, 4, 65535, "RGB_ALPHA", order=("WIDTH", "HEIGHT", "DEPTH")) + body7,
        "p7_width_twice": pam_head(5, 3, 4, 65535, "RGB_ALPHA", order=("WIDTH", "HEIGHT", "WIDTH", "DEPTH", "MAXVAL")) + body7,
        "p7_maxval_twice": pam_head(5, 3, 4, 65535, "RGB_ALPHA", order=("WIDTH", "HEIGHT", "DEPTH", "MAXVAL", "MAXVAL")) + body7,
        "p7_depth_0": pam_head(5, 3, 0, 65535, "RGB_ALPHA") + body7,
        "p7_depth_5": pam_head(5, 3, 5, 65535, "RGB_ALPHA") + body7 + body7,
        "p7_no_endhdr": pam_head(5, 3, 4, 65535, "RGB_ALPHA").replace(b"ENDHDR\n", b"") + body7,
        "p7_endhdr_without_newline": pam_head(5, 3, 4, 65535, "RGB_ALPHA")[:-1],
        "p7_unknown_token": pam_head(5, 3, 4, 65535, "RGB_ALPHA", extra=(b"COLOURS 3",)) + body7,
        "p7_field_without_a_number": pam_head(5, 3, 4, 65535, "RGB_ALPHA", extra=(b"WIDTH",), order=("HEIGHT", "DEPTH", "MAXVAL")) + body7,
        "p7_field_with_two_numbers": pam_head(5, 3, 4, 65535, "RGB_ALPHA", extra=(b"WIDTH 5 5",), order=("HEIGHT", "DEPTH", "MAXVAL")) + body7,
        "p7_negative_height": pam_head(5, 3, 4, 65535, "RGB_ALPHA", extra=(b"HEIGHT -3",), order=("WIDTH", "DEPTH", "MAXVAL")) + body7,
        "p7_word_behind_endhdr": pam_head(5, 3, 4, 65535, "RGB_ALPHA").replace(b"ENDHDR\n", b"ENDHDR now\n") + body7,
        "p7_magic_line_goes_on": pam_head(5, 3, 4, 65535, "RGB_ALPHA").replace(b"P7\n", b"P7 WIDTH 5\n", 1) + body7,
        "p7_black_and_white_maxval_255": pam_head(5, 3, 1, 255, "BLACKANDWHITE") + body1,
        "p7_black_and_white_depth_3": pam_head(5, 3, 3, 1, "BLACKANDWHITE") + body6,
        "p7_black_and_white_depth_4": pam_head(5, 3, 4, 1, "BLACKANDWHITE_ALPHA") + body6 + body6,
        "p1_ascii": b"P1\n5 3\n" + b"0 1 0 1 0\n" * 3,
        "p2_ascii": b"P2\n5 3\n255\n" + b"1 2 3 4 5\n" * 3,
        "p3_ascii": b"P3\n2 2\n255\n" + b"1 2 3 4 5 6\n" * 2,
        "p8": b"P8\n5 3\n255\n" + body6,
        "p_alone": b"P" + bytes(16),
        "p4_lower_case": b"p4\n11 3\n" + body4,
    }
    return out, [good4, good7]


def header_cuts():
    """every proper prefix of the headers of a P4 (with comments) and a P7 file, and the whole header without a
    raster: none is readable"""
    out = {}
    heads = {"p4": b"P4\n# bits\n11 3\n", "p4b": b"P4 # packed\n11\t# deep\n300\n",
             "p7": pam_head(5, 3, 2, 1, "BLACKANDWHITE_ALPHA", extra=(b"# a comment", b""))}
    for name, head in heads.items():
        for cut in range(len(head) + 1):
            out[f"{name}_cut{cut}"] = head[:cut]
    return out
