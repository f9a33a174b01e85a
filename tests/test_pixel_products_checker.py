"""CPU self-test of tests/pixel_products.py: products packed from the oracle pass the checker, and every way a kernel
could breach the hand-over contract without the end-to-end tests noticing is rejected, each by the clause it breaks.
This is what shows that tests/test_gpu_pixel_products.py would fail on a subtly wrong kernel."""
import copy

import numpy as np
import pytest

from tests import pixel_products as pp

W, H = 144, 80


def _frame():
    """Noise on the left (isolated hot pixels), a checkerboard of 3-pixel squares on the right (full groups)."""
    rng = np.random.default_rng(7)
    f = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    f[:, W // 2:] = ((((x // 3) + (y // 3)) & 1) * 255).astype(np.uint8)[:, W // 2:]
    return f


FRAME = _frame()
EXPECTED = {L: pp.expected_of(FRAME, L) for L in (0, 1)}


def _packed(level=0, cap=1 << 20, order=None):
    image, resp = EXPECTED[level]
    return pp.pack_raster(image, resp, cap, order)


def _hot(level=0):
    return pp.hot_groups(EXPECTED[level][1])


def _isolated_entry(p, level=0):
    """index of a stored entry whose pixel is the only hot one of its group"""
    _, mask = _hot(level)
    for i, e in enumerate(p["hot_xy"]):
        if pp._POPCOUNT[mask[e >> 16, (e & 0xffff) >> 3]] == 1:
            return i
    raise AssertionError("the frame has no isolated hot pixel")


def _group_of_two(p, level=0):
    """index of the first entry of a group with at least two hot pixels"""
    _, mask = _hot(level)
    for i, e in enumerate(p["hot_xy"]):
        if pp._POPCOUNT[mask[e >> 16, (e & 0xffff) >> 3]] >= 2:
            return i
    raise AssertionError("the frame has no group of two hot pixels")


def test_the_frame_has_what_the_mutations_need():
    hot, mask = _hot()
    counts = pp._POPCOUNT[mask]
    assert (counts == 1).sum() > 10 and (counts >= 4).sum() > 10 and hot.sum() > 500
    assert not hot[:7].any() and not hot[:, :7].any() and not hot[-7:].any() and not hot[:, -7:].any()


@pytest.mark.parametrize("level", [0, 1])
def test_raster_packing_is_accepted(level):
    p = _packed(level)
    assert pp.check_level(p, FRAME, level) == p["hot_cnt"] > 0          # (expectations straight from the oracle)
    assert pp.check_level(p, FRAME, level, EXPECTED[level]) == p["hot_cnt"]
    assert (p["gidx"] == pp.GARBAGE).any()                               # pairs nobody may read hold garbage


def test_any_order_of_the_groups_is_accepted():
    """Workgroups append concurrently: the contract fixes the order inside a group, not the order of the groups."""
    _, mask = _hot()
    perm = np.random.default_rng(1).permutation(int((mask != 0).sum()))
    pp.check_level(_packed(order=perm), FRAME, 0, EXPECTED[0])


def test_overflow_is_accepted_for_what_fits():
    n = _packed()["hot_cnt"]
    for cap in (n - 1, n // 2, 1):
        p = _packed(cap=cap)
        assert len(p["hot_xy"]) == cap and p["hot_cnt"] == n
        pp.check_level(p, FRAME, 0, EXPECTED[0])
    p = _packed(cap=n)                                                    # exactly full is no overflow
    pp.check_level(p, FRAME, 0, EXPECTED[0])


def _drop(p):
    p["hot_xy"] = np.delete(p["hot_xy"], _isolated_entry(p))


def _drop_and_count(p):
    _drop(p)
    p["hot_cnt"] -= 1


def _duplicate_isolated(p):
    i = _isolated_entry(p)
    p["hot_xy"][(i + 5) % len(p["hot_xy"])] = p["hot_xy"][i]


def _swap_in_group(p):
    i = _group_of_two(p)
    p["hot_xy"][[i, i + 1]] = p["hot_xy"][[i + 1, i]]


def _some_hot_group(p):
    gy, gx = np.nonzero(_hot()[1])
    return gy[len(gy) // 2], gx[len(gx) // 2]


def _base_off_by_one(p):
    y, g = _some_hot_group(p)
    p["gidx"][y, g, 0] += 1


def _mask_bit_missing(p):
    e = int(p["hot_xy"][_group_of_two(p)])
    y, g = e >> 16, (e & 0xffff) >> 3
    m = int(p["gidx"][y, g, 1])
    p["gidx"][y, g, 1] = m & (m - 1)


def _count_off_by_one(p):
    p["hot_cnt"] += 1


def _response_on_frame_row(p):
    p["response"][6, W // 2] = 5                                          # not hot: only the dense comparison can see it


def _bit31(p):
    p["hot_xy"][_isolated_entry(p)] |= 0x80000000


def _entry_not_hot(p):
    i = _isolated_entry(p)
    p["hot_xy"][i] = (3 << 16) | 3                                         # a pixel of the zero frame


MUTATIONS = [
    ("an entry dropped", _drop, "d"),
    ("an entry dropped, the count following it", _drop_and_count, "c"),
    ("an entry duplicated over an isolated pixel", _duplicate_isolated, "d"),
    ("two entries of a group swapped", _swap_in_group, "f"),
    ("a gidx base off by one", _base_off_by_one, "f"),
    ("a gidx mask with a bit missing", _mask_bit_missing, "f"),
    ("hot_cnt off by one", _count_off_by_one, "c"),
    ("one response value changed on a frame row", _response_on_frame_row, "b"),
    ("an entry with bit 31 set", _bit31, "d"),
    ("an entry that is not hot", _entry_not_hot, "d"),
]


@pytest.mark.parametrize("name,mutate,clause", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_each_mutation_is_rejected(name, mutate, clause):
    p = copy.deepcopy(_packed())
    mutate(p)
    with pytest.raises(pp.ProductError) as e:
        pp.check_level(p, FRAME, 0, EXPECTED[0])
    assert e.value.clause == clause, str(e.value)


def test_level_image_byte_in_the_outermost_column_is_rejected():
    """ChESS never reads the outer two pixels of a level image: only the comparison with oracle.decimate sees them."""
    for x in (0, -1):
        p = _packed(1)
        p["image"][H // 4, x] ^= 1
        with pytest.raises(pp.ProductError) as e:
            pp.check_level(p, FRAME, 1, EXPECTED[1])
        assert e.value.clause == "a"
    p = _packed(1)
    del p["image"]
    with pytest.raises(pp.ProductError):
        pp.check_level(p, FRAME, 1, EXPECTED[1])


def test_mutations_are_rejected_under_overflow_too():
    """Clause g: what fits below cap is held to d. and f.; hot_cnt to c."""
    n = _packed()["hot_cnt"]
    cap = n // 2
    for mutate, clause in ((_duplicate_isolated, "d"), (_swap_in_group, "f"), (_count_off_by_one, "c"), (_bit31, "d")):
        p = _packed(cap=cap)
        mutate(p)
        with pytest.raises(pp.ProductError) as e:
            pp.check_level(p, FRAME, 0, EXPECTED[0])
        assert e.value.clause == clause
    # a group whose map points below cap while its pixels were never stored there
    p = _packed(cap=cap)
    _, mask = _hot()
    gy, gx = np.nonzero(mask)
    p["gidx"][gy[-1], gx[-1], 0] = 0                                        # the last group's entries lie beyond cap
    with pytest.raises(pp.ProductError) as e:
        pp.check_level(p, FRAME, 0, EXPECTED[0])
    assert e.value.clause == "f"


def test_supplied_response_is_clamped_like_the_response_mode():
    r = np.full((20, 24), -3, np.int16)
    r[7, 7] = 40
    r[6, 7] = 99
    r[12, 16] = 17
    out = pp.clamp_supplied_response(r)
    assert out[7, 7] == 40 and out[12, 16] == 17 and out.sum() == 57
