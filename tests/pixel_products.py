"""What the pixel stage of a chain / detect call hands to the component search (CompTables, csrc/common.h), checked in
plain numpy against the CPU oracle.  Shared by the CPU self-test of this checker (tests/test_pixel_products_checker.py)
and the GPU tests that read the products of every launch path through Detector.pixel_products
(tests/test_gpu_pixel_products.py).

The products of ONE frame at ONE level are a dict:
    "image"     u8  [h, w]      the level image (levels >= 1; absent at level 0)
    "response"  i16 [h, w]      the clamped response
    "hot_cnt"   int             hot-list entries made (may exceed cap)
    "cap"       int             capacity of the list
    "hot_xy"    u32 [min(hot_cnt, cap)]   the stored entries, (y << 16) | x
    "gidx"      u32 [h, gw, 2]  per aligned 8-pixel group (index of its first hot pixel, 8-bit mask); groups without a
                                hot pixel are never written and hold anything

The contract ("What the pixel stage hands over"):
 a. image == oracle.decimate(frame, level) at every pixel, borders included
 b. response == max(oracle.chess_response_5(level image, fill=0), 0) at every pixel (the 7-pixel frame is 0)
 c. hot_cnt == count(oracle response > 15), also when it exceeds cap
 d. the stored entries are pairwise distinct, each is a hot pixel of the oracle, bit 31 is clear on every one
 e. hot_cnt <= cap: the stored entries are exactly the oracle's set
 f. the hot pixels of a group sit in consecutive entries in ascending x, as far as they lie below cap, and gidx of the
    group is (index of the first, the oracle's mask); gidx is read at no other group
 g. under overflow a. to d. and f. hold for what fits
"""
import numpy as np

from oracle import oracle

RESP_MIN = 15            # RESPONSE_MIN_THRESHOLD: hot = response > 15
GARBAGE = 0xDEADBEEF     # what pack_raster leaves in the gidx pairs nobody may read


class ProductError(AssertionError):
    """A clause of the contract does not hold; .clause is its letter."""

    def __init__(self, clause, msg):
        super().__init__(f"clause {clause}: {msg}")
        self.clause = clause


def _require(ok, clause, msg):
    if not ok:
        raise ProductError(clause, msg() if callable(msg) else msg)


def expected_of(frame, level):
    """-> (level image or None at level 0, clamped response) of the oracle."""
    img = np.ascontiguousarray(frame) if level == 0 else oracle.decimate(frame, level)
    return (None if level == 0 else img), np.maximum(oracle.chess_response_5(img, fill=0), 0)


def clamp_supplied_response(resp):
    """What the response mode leaves of a caller's response: negatives 0, the 7-pixel frame 0 (cc.hip)."""
    out = np.zeros_like(resp)
    out[7:-7, 7:-7] = np.maximum(resp[7:-7, 7:-7], 0)
    return out


def hot_groups(resp):
    """-> (hot bool [h, w], mask u8 [h, gw]: bit i = pixel 8 * g + i of the row is hot)"""
    h, w = resp.shape
    gw = (w + 7) // 8
    hot = resp > RESP_MIN
    padded = np.zeros((h, gw * 8), bool)
    padded[:, :w] = hot
    return hot, np.packbits(padded.reshape(h, gw, 8), axis=2, bitorder="little")[:, :, 0]


_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int64)


def _slots(gidx, mask, ys, xs):
    """list index the map gives pixels (xs, ys), all hot: base + popcount(mask below x) -- with the ORACLE's mask"""
    g = xs >> 3
    below = mask[ys, g].astype(np.int64) & ((1 << (xs & 7)) - 1)
    return gidx[ys, g, 0].astype(np.int64) + _POPCOUNT[below]


def frame_products(products, f):
    """One frame of what Detector.pixel_products returns for a level."""
    p = {"hot_cnt": int(products["hot_cnt"][f]), "cap": int(products["cap"]), "hot_xy": products["hot_xy"][f],
         "gidx": products["gidx"][f], "response": products["response"][f]}
    if "image" in products:
        p["image"] = products["image"][f]
    return p


def check_products(p, image, resp):
    """The contract against an expected level image (None: the level has none) and clamped response."""
    h, w = resp.shape
    if image is not None:
        _require("image" in p, "a", "no level image among the products")
        _require(p["image"].shape == image.shape, "a", lambda: f"image shape {p['image'].shape} != {image.shape}")
        bad = np.argwhere(p["image"] != image)
        _require(len(bad) == 0, "a", lambda: f"{len(bad)} pixels differ, first (y, x) = {tuple(bad[0])}")
    _require(p["response"].shape == resp.shape, "b", lambda: f"response shape {p['response'].shape} != {resp.shape}")
    bad = np.argwhere(p["response"] != resp)
    _require(len(bad) == 0, "b", lambda: f"{len(bad)} responses differ, first (y, x) = {tuple(bad[0])}: "
             f"{p['response'][tuple(bad[0])]} != {resp[tuple(bad[0])]}")

    hot, mask = hot_groups(resp)
    n, cap = int(hot.sum()), p["cap"]
    _require(p["hot_cnt"] == n, "c", lambda: f"hot_cnt {p['hot_cnt']} != {n} hot pixels of the oracle (cap {cap})")

    stored = np.asarray(p["hot_xy"], np.uint32)
    _require(len(stored) == min(n, cap), "d", lambda: f"{len(stored)} entries stored, min(hot_cnt, cap) = {min(n, cap)}")
    _require(not (stored & 0x80000000).any(), "d", lambda: f"bit 31 set on entry {int(np.argmax(stored >> 31))}")
    sy, sx = (stored >> 16).astype(np.int64), (stored & 0xffff).astype(np.int64)
    inside = (sy < h) & (sx < w)
    _require(inside.all(), "d", lambda: f"entry {int(np.argmin(inside))} = {stored[np.argmin(inside)]:#x} lies outside the image")
    is_hot = hot[sy, sx]
    _require(is_hot.all(), "d", lambda: f"entry {int(np.argmin(is_hot))} = (x {sx[np.argmin(is_hot)]}, y {sy[np.argmin(is_hot)]}) is not hot")
    uniq, counts = np.unique(stored, return_counts=True)
    _require(len(uniq) == len(stored), "d", lambda: f"entry {uniq[np.argmax(counts)]:#x} is stored {counts.max()} times")

    ys, xs = np.nonzero(hot)                              # raster order: ascending x inside a group
    keys = (ys.astype(np.uint32) << 16) | xs.astype(np.uint32)
    if n <= cap:
        _require(np.array_equal(uniq, keys), "e", "the stored entries are not the oracle's hot pixels")

    gy, gx = np.nonzero(mask)                             # the groups with a hot pixel: the only pairs of gidx that are read
    gidx = p["gidx"]
    _require(gidx.shape == mask.shape + (2,), "f", lambda: f"gidx shape {gidx.shape}")
    got_mask = gidx[gy, gx, 1]
    bad = np.nonzero(got_mask != mask[gy, gx])[0]
    _require(len(bad) == 0, "f", lambda: f"group (x0 {8 * gx[bad[0]]}, y {gy[bad[0]]}): mask {got_mask[bad[0]]:#x} != {mask[gy, gx][bad[0]]:#x}")
    ends = gidx[gy, gx, 0].astype(np.int64) + _POPCOUNT[mask[gy, gx]]
    bad = np.nonzero(ends > n)[0]
    _require(len(bad) == 0, "f", lambda: f"group (x0 {8 * gx[bad[0]]}, y {gy[bad[0]]}): entries end at {ends[bad[0]]} > hot_cnt {n}")
    # every hot pixel whose slot lies below cap is stored in that slot ...
    k = _slots(gidx, mask, ys, xs)
    fits = k < cap
    bad = np.nonzero(stored[k[fits]] != keys[fits])[0]
    _require(len(bad) == 0, "f", lambda: f"pixel (x {xs[fits][bad[0]]}, y {ys[fits][bad[0]]}) belongs in entry {k[fits][bad[0]]}, "
             f"which holds {stored[k[fits][bad[0]]]:#x}")
    # ... and every stored entry sits in the slot the map gives its pixel
    at = _slots(gidx, mask, sy, sx)
    bad = np.nonzero(at != np.arange(len(stored)))[0]
    _require(len(bad) == 0, "f", lambda: f"entry {bad[0]} = (x {sx[bad[0]]}, y {sy[bad[0]]}): the map says index {at[bad[0]]}")
    return n


def check_level(products, frame, level, expected=None):
    """products: one frame's (frame_products); frame: the u8 source frame.  The expectations are the oracle's alone
    (`expected`: a cached expected_of(frame, level)).  -> the oracle's hot-pixel count."""
    image, resp = expected if expected is not None else expected_of(frame, level)
    return check_products(products, image, resp)


def pack_raster(image, resp, cap, order=None):
    """Products that satisfy the contract, built from the expectations: the hot pixels in raster order (`order`: a
    permutation of the GROUPS with a hot pixel, to lay the list out the way concurrent workgroups might), cut at cap."""
    h, w = resp.shape
    hot, mask = hot_groups(resp)
    gy, gx = np.nonzero(mask)
    if order is not None:
        gy, gx = gy[order], gx[order]
    counts = _POPCOUNT[mask[gy, gx]]
    base = np.concatenate([[0], np.cumsum(counts)])
    gidx = np.full(mask.shape + (2,), GARBAGE, np.uint32)
    gidx[gy, gx, 0] = base[:-1]
    gidx[gy, gx, 1] = mask[gy, gx]
    entries = []
    for y, g, m in zip(gy, gx, mask[gy, gx]):
        entries += [(int(y) << 16) | (8 * int(g) + i) for i in range(8) if m >> i & 1]
    n = int(hot.sum())
    p = {"response": resp.copy(), "hot_cnt": n, "cap": int(cap), "hot_xy": np.array(entries[:min(n, cap)], np.uint32), "gidx": gidx}
    if image is not None:
        p["image"] = image.copy()
    return p
