"""Files for the tests of mrgingham_amd.find_boards_files, probe_image and the tool's --batch mode, all out of the
committed fixtures (tests/golden/jpeg_golden.npz, jpeg_rst_golden.npz, jpeg_sync_golden.npz) and written to a directory
of the test: the JPEG files as they are, and PGM / PNG / 16-bit PGM copies of the decoded 640x480 board.  Nothing is
larger than 640x480."""
import os
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = ("jpeg_golden", "jpeg_rst_golden", "jpeg_sync_golden")
BOARD = "board_640x480_grey_q90"


def golden_jpegs():
    """-> [(name, bytes, readable, width, height)] over the three golden files, in their order."""
    out = []
    for stem in GOLDEN:
        g = np.load(os.path.join(ROOT, "tests", "golden", stem + ".npz"))
        for i, name in enumerate(g["name"]):
            out.append((str(name), g[f"jpg_{i}"].tobytes(), bool(g["readable"][i]), int(g["width"][i]), int(g["height"][i])))
    return out


def board_pixels():
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz"))
    i = list(g["name"]).index(BOARD)
    return g[f"luma_{i}"]


def write_pgm(path, img, maxval=255):      # (as tests/test_cli.py writes them)
    with open(path, "wb") as f:
        f.write(b"P5\n# a comment line\n%d %d\n%d\n" % (img.shape[1], img.shape[0], maxval))
        f.write(img.astype(">u2").tobytes() if maxval > 255 else img.astype(np.uint8).tobytes())


def write_png(path, img, bits=8, width=None, height=None):
    """Minimal grey PNG writer (8 or 16 bit), every row with a different filter type (as tests/test_cli.py's).  width /
    height: what the IHDR claims instead of the image's own size."""
    h, w = img.shape[:2]
    bpp = bits // 8
    rows = np.frombuffer(img.astype(">u2" if bits == 16 else np.uint8).tobytes(), np.uint8).reshape(h, w * bpp).astype(np.int32)
    raw = bytearray()
    prev = np.zeros(w * bpp, np.int32)
    for y in range(h):
        ft = y % 5
        cur = rows[y]
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])
        upleft = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])
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
        raw.append(ft)
        raw += ((cur - pred) & 0xff).astype(np.uint8).tobytes()
        prev = cur

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    comp = zlib.compress(bytes(raw), 6)
    half = len(comp) // 2                                   # two IDAT chunks
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width or w, height or h, bits, 0, 0, 0, 0)) +
                chunk(b"IDAT", comp[:half]) + chunk(b"IDAT", comp[half:]) + chunk(b"IEND", b""))


def write_all(directory):
    """Every file the tests use -> {name: path}: '<fixture>.jpg' for every golden JPEG, board.pgm, board.png,
    board16.pgm (16 bit), and 'missing.jpg', which is not written."""
    directory = str(directory)
    paths = {}
    for name, data, _, _, _ in golden_jpegs():
        paths[name] = os.path.join(directory, name + ".jpg")
        with open(paths[name], "wb") as f:
            f.write(data)
    board = board_pixels()
    paths["board.pgm"] = os.path.join(directory, "board.pgm")
    write_pgm(paths["board.pgm"], board)
    paths["board.png"] = os.path.join(directory, "board.png")
    write_png(paths["board.png"], board)
    paths["board16.pgm"] = os.path.join(directory, "board16.pgm")
    write_pgm(paths["board16.pgm"], board.astype(np.uint16) * 257, maxval=65535)
    paths["missing"] = os.path.join(directory, "missing.jpg")
    return paths


def mixed_list(paths):
    """The list of the equality tests: two sizes of board-bearing frames (640x480, 320x240), the three formats, the 16-bit
    file, the progressive file, tiny files and the missing path interleaved, the board JPEG several times: 24 names."""
    p = paths
    return [p[BOARD], p["blend_320x240_grey_q90"], p["board.pgm"], p["noise_48x64_grey_q75_r3"], p["missing"],
            p[BOARD + "_dri80"], p["blend_320x240_444_q95"], p["board16.pgm"], p["board.png"], p["progressive_48x64_420"],
            p["blend_640x480_420_q90"], p["noise_8x8_grey_q30_r0"], p["blend_320x240_422_q75"], p[BOARD],
            p["noise_48x64_420_q30_r3"], p["blend_320x240_420_q90"], p["board.pgm"], p["checker_8x8_420_q75_r1"],
            p["noise_48x64_444_q100_dri2"], p[BOARD], p["blend_320x240_420_q50"], p["board.png"], p["missing"],
            p["plain_320x240_420_q90"]]
