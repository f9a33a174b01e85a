"""What tests/test_find_grids_model.py (CPU) and tests/test_gpu_find_grids.py (GPU) share: the corpus of
tests/grid_cases.py as batches of candidate lists, one batch per gridn, in the layout of mrgingham_amd_find_grids_batch
(xy int32 [nlists, CAPACITY, 2] with poison behind every list's count, counts int32 [nlists]); the lattices that sit on
the sequence walk's thresholds; the layout cases."""
import numpy as np

from tests import grid_cases as gc

CAPACITY = 512
POISON = 0x7F7F7F7F          # behind a list's count: far outside the coordinate range, never read

# the families in which no list may be declined for any reason (907 sets), and those in which -2 is allowed
NEVER_DECLINED = ("clean_", "ambiguous_", "jitter", "ratio_", "angle_", "cand_")
RING_DECLINES_ALLOWED = ("exact_", "cocircular_", "dup_", "empty_", "one_", "two_", "line_", "tiny_", "outlier")


def pack(lists, capacity=CAPACITY):
    """Candidate lists (int (n, 2) arrays) -> (xy, counts) with poison behind every count."""
    xy = np.full((len(lists), capacity, 2), POISON, dtype=np.int32)
    counts = np.zeros((len(lists),), dtype=np.int32)
    for i, p in enumerate(lists):
        p = np.asarray(p, dtype=np.int32).reshape(-1, 2)
        xy[i, :len(p)] = p
        counts[i] = len(p)
    return xy, counts


def corpus_batches(golden_dir=None):
    """{gridn: (names, lists, xy, counts)} over gc.all_cases(), in its order within a gridn."""
    by = {}
    for name, gridn, pts, _ in gc.all_cases(golden_dir):
        names, lists = by.setdefault(gridn, ([], []))
        names.append(name)
        lists.append(pts)
    return {g: (names, lists) + pack(lists) for g, (names, lists) in sorted(by.items())}


def threshold_lattices():
    """4 x 4 lattices whose last column gap is exactly 1.4 (0.7 walking back) or whose last column sits at 2.7: the
    length ratio of a step equals a limit of find_grid.cc:204-207 to the last bit, along the axes and along a 3-4-5
    direction (every length an integer)."""
    for u, v in (((50000, 0), (0, 50000)), ((30000, 40000), (-40000, 30000))):
        for columns in ([0, 1, 2, 3.4], [0, 1, 2, 2.7]):
            yield gc._lattice(4, u, v, columns=columns).astype(np.int32)


def garbage_lists(seed, n, capacity=CAPACITY):
    """n lists of random garbage: counts below 0, above the capacity and anywhere between; coordinates over the whole
    int32 range, in a tiny box (duplicates), on a line, on a lattice."""
    rng = np.random.RandomState(seed)
    xy = rng.randint(-2 ** 31, 2 ** 31 - 1, (n, capacity, 2)).astype(np.int32)
    counts = rng.randint(-3, capacity + 40, n).astype(np.int32)
    for i in range(n):
        kind = i % 5
        if kind == 1:
            xy[i] = rng.randint(0, 6, (capacity, 2)) * 1000
        elif kind == 2:
            t = rng.randint(0, 300, capacity)
            xy[i] = np.stack([t * 700, t * 300 + 5], 1)
        elif kind == 3:
            xy[i] = np.stack([rng.randint(0, 23, capacity) * 40000, rng.randint(0, 23, capacity) * 40000], 1)
        elif kind == 4:
            xy[i] = rng.randint(-(2 ** 24) + 1, 2 ** 24, (capacity, 2))
    return xy, counts
