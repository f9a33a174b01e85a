"""The numpy yardstick of the Bayer-to-grey definition (include/mrgingham_amd.h), written from the definition alone, the
known answers it is held against (check_known), and the frames the host and the device tests share."""
import numpy as np

PATTERNS = ("rggb", "grbg", "gbrg", "bggr")
# the colours of pixels (0,0), (0,1), (1,0), (1,1)
COLOURS = {"rggb": "RGGB", "grbg": "GRBG", "gbrg": "GBRG", "bggr": "BGGR"}
CR, CG, CB = 4899, 9617, 1868
SHAPES = ((2, 2), (2, 3), (3, 2), (5, 3), (3, 15), (3, 16), (3, 17), (4, 31), (4, 32), (4, 33), (9, 17), (70, 33), (2, 300), (33, 130))
DTYPES = (np.uint8, np.uint16)


def colour_at(pattern, h, w, beside=False):
    """[h, w] array of 'R', 'G', 'B': the colour of every site; beside: that of its horizontal neighbours"""
    c = np.array(list(COLOURS[pattern])).reshape(2, 2)
    return np.tile(c[:, ::-1] if beside else c, ((h + 1) // 2, (w + 1) // 2))[:h, :w]


def grey(mosaic, pattern):
    """the definition: reflect-101 borders, the four sums, one rounding in unsigned 32-bit arithmetic"""
    m = np.asarray(mosaic)
    assert m.dtype in (np.uint8, np.uint16) and m.ndim == 2 and m.shape[0] >= 2 and m.shape[1] >= 2
    h, w = m.shape
    p = np.pad(m.astype(np.uint64), 1, mode="reflect")              # index -1 is 1, index n is n-2
    v = p[1:-1, 1:-1]
    N, S, W, E = p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    cross, hor, ver = N + S + W + E, W + E, N + S
    diag = p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:]
    col = colour_at(pattern, h, w)
    row_other = colour_at(pattern, h, w, beside=True)              # the other colour of a green site's row
    red = (4 * CR * v + CG * cross + CB * diag + 32768) >> 16
    blue = (4 * CB * v + CG * cross + CR * diag + 32768) >> 16
    green_r = (2 * CG * v + CR * hor + CB * ver + 16384) >> 15
    green_b = (2 * CG * v + CB * hor + CR * ver + 16384) >> 15
    assert max(int(a.max()) for a in (4 * CR * v + CG * cross + CB * diag + 32768, 4 * CB * v + CG * cross + CR * diag + 32768)) < 1 << 32
    out = np.where(col == "R", red, np.where(col == "B", blue, np.where(row_other == "R", green_r, green_b)))
    return out.astype(m.dtype)


def sample_scene(rgb, pattern):
    """an [h, w, 3] colour image through the filter: every site keeps its own colour's value"""
    h, w = rgb.shape[:2]
    col = colour_at(pattern, h, w)
    return np.where(col == "R", rgb[..., 0], np.where(col == "G", rgb[..., 1], rgb[..., 2]))


KNOWN_UNIFORM = ((np.uint8, 255, (76, 150, 29)), (np.uint16, 65535, (19596, 38467, 7472)), (np.uint16, 4095, (1224, 2404, 467)))
KNOWN_2X2 = {"rggb": [[22, 19], [25, 22]], "grbg": [[15, 24], [24, 33]], "gbrg": [[17, 26], [26, 35]], "bggr": [[28, 25], [31, 28]]}
KNOWN_SHAPES = ((2, 2), (3, 5), (6, 7), (4, 17))


def known_cases():
    """(mosaic, pattern, expected grey) of the issue's tables"""
    for dtype, top, answers in KNOWN_UNIFORM:
        for ch, want in enumerate(answers):
            for pat in PATTERNS:
                for h, w in KNOWN_SHAPES:
                    rgb = np.zeros((h, w, 3), dtype)
                    rgb[..., ch] = top
                    yield sample_scene(rgb, pat), pat, np.full((h, w), want, dtype)
    for pat, want in KNOWN_2X2.items():
        for dtype in DTYPES:
            yield np.array([[10, 20], [30, 40]], dtype), pat, np.array(want, dtype)


def check_known(fn=grey):
    for m, pat, want in known_cases():
        got = fn(m, pat)
        assert got.dtype == want.dtype and np.array_equal(got, want), (pat, m.dtype, m.shape, got.tolist())
    for dtype in DTYPES:                                             # a constant mosaic comes out unchanged
        for value in (0, 1, 77, np.iinfo(dtype).max):
            for pat in PATTERNS:
                m = np.full((5, 6), value, dtype)
                assert np.array_equal(fn(m, pat), m), (pat, value)


def random_frames(n, h, w, dtype, seed):
    return np.random.default_rng(seed).integers(0, int(np.iinfo(dtype).max) + 1, (n, h, w), dtype=dtype)


def impulse_frames(h, w, dtype):
    """the top value at one pixel and 0 elsewhere, for every pixel, and the complements: [2*h*w, h, w]"""
    top = np.iinfo(dtype).max
    a = np.zeros((h * w, h, w), dtype)
    a.reshape(h * w, h * w)[np.arange(h * w), np.arange(h * w)] = top
    return np.concatenate([a, top - a])


def tinted_board(seed, pattern, W=640, H=480, gridn=10, bits=8):
    """synth.board_frame tinted R : G : B = 1 : 3/4 : 1/2 and sampled through the pattern; bits 16: f*16 + (f >> 4) first"""
    from mrgingham_amd import synth
    f = synth.board_frame(W, H, gridn, seed).numpy().astype(np.uint32)
    dtype = np.uint8
    if bits == 16:
        f, dtype = f * 16 + (f >> 4), np.uint16
    rgb = np.stack([f, f * 3 // 4, f // 2], axis=-1).astype(dtype)
    return sample_scene(rgb, pattern)


def check_corners(points, lattice, what):
    """points [N,2] in pixels: exactly one within 0.4 lattice pitches of every lattice point, and that one within 0.4 px"""
    lat = lattice.reshape(-1, 2)
    pitch = float(np.hypot(*(lattice[0, 1] - lattice[0, 0])))
    d = np.hypot(points[None, :, 0] - lat[:, None, 0], points[None, :, 1] - lat[:, None, 1])     # [lattice, points]
    near = (d < 0.4 * pitch).sum(axis=1)
    assert (near == 1).all(), (what, near.tolist())
    worst = float(d.min(axis=1).max())
    print(f"{what}: worst distance {worst:.3f} px")
    assert worst <= 0.4, (what, worst)
    return worst
