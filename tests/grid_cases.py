"""Candidate sets for the grid-finder tests: the board generators of tests/test_grid.py, and the families on which
tests/test_oracle_grid.py holds mrgingham_amd/csrc/grid.cpp to upstream's own find_grid.cc.

A case is (name, gridn, points int32 (N,2) x1000, truth).  `truth` is the generating lattice in board order
(int64 (gridn*gridn, 2)) where the family has one -- a board that is reported must then equal it --, else None.
Everything is generated from seeds; tests/golden/grid_kat.npz records, per case, a hash of the input and upstream's
answer (tests/golden/make_grid_golden.py)."""
import hashlib
import os

import numpy as np


def _board(gridn, H, jitter=0.0, seed=0, outliers=0, shuffle=True, origin=(400.0, 300.0), pitch=60.0):
    """gridn x gridn corners through a homography (mild perspective + rotation), as x1000 ints."""
    rng = np.random.RandomState(seed)
    ii, jj = np.meshgrid(np.arange(gridn), np.arange(gridn), indexing="ij")       # ii = row, jj = column
    p = np.stack([jj.ravel() * pitch, ii.ravel() * pitch, np.ones(gridn * gridn)])
    q = H @ p
    xy = (q[:2] / q[2]).T + np.array(origin)
    xy = xy + rng.normal(0, jitter, xy.shape)
    truth = np.round(xy * 1000).astype(np.int64)
    pts = truth.copy()
    if outliers:
        lo, hi = truth.min(0) - 200000, truth.max(0) + 200000
        pts = np.concatenate([pts, np.stack([rng.randint(lo[0], hi[0], outliers), rng.randint(lo[1], hi[1], outliers)], 1)])
    if shuffle:
        pts = pts[rng.permutation(len(pts))]
    return pts.astype(np.int32), truth


def _rot(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


def _random_board(rng, trial, clean):
    gridn = int(rng.choice([4, 6, 10, 10, 14]))
    Hm = _rot(rng.uniform(-35, 35))
    Hm[2, 0], Hm[2, 1] = rng.uniform(-3e-4, 3e-4), rng.uniform(-3e-4, 3e-4)
    jitter = float(rng.choice([0.0, 0.2, 0.5, 1.0]))
    pts, truth = _board(gridn, Hm, jitter=jitter, seed=10000 + trial, outliers=int(rng.choice([0, 5, 30, 60])),
                        origin=(2000.0, 2000.0))
    # local pitch: distance to the nearest other lattice point
    d = np.sqrt(((truth[:, None, :] - truth[None, :, :]).astype(np.float64) ** 2).sum(-1))
    np.fill_diagonal(d, np.inf)
    pitch = d.min(1)
    is_truth = (pts[:, None, :] == truth[None, :, :]).all(-1).any(1)
    if clean:
        # keep only the outliers that are at least 1.5 local pitches away from every lattice point
        dist = np.sqrt(((pts[:, None, :] - truth[None, :, :]).astype(np.float64) ** 2).sum(-1))
        far = (dist > 1.5 * pitch[None, :]).all(1)
        pts = pts[is_truth | far]
        if trial % 3 == 1:                                     # exact duplicates of a few candidates
            pts = np.concatenate([pts, pts[:5]])
    else:
        kind = trial % 3
        if kind == 0:                                          # split blobs: a twin 3-8 % of the pitch away
            k = rng.randint(0, len(truth), 3)
            pts = np.concatenate([pts, (truth[k] + rng.randint(2000, 5000, (3, 2))).astype(np.int32)])
        elif kind == 1:                                        # near-duplicates a fraction of a pixel away
            pts = np.concatenate([pts, pts[:5] + rng.randint(-300, 300, (5, 2)).astype(np.int32)])
        # kind 2: the outliers inside the lattice are the ambiguity
    return gridn, jitter, pts.astype(np.int32), truth, pitch


# ---------------------------------------------------------------------------------------------
# The families of tests/test_oracle_grid.py
# ---------------------------------------------------------------------------------------------

def clean_sets():
    """The 500 sets of test_visiting_order_does_not_matter_on_clean_candidate_sets (same generator, same seeds)."""
    rng = np.random.RandomState(2024)
    for trial in range(500):
        gridn, _, pts, truth, _ = _random_board(rng, trial, clean=True)
        yield "clean_%03d" % trial, gridn, pts, truth


def ambiguous_sets():
    """The 300 sets of test_ambiguous_candidate_sets_are_order_dependent_but_never_wrong.  No truth: a corner of a
    reported board may be the twin of a split blob."""
    rng = np.random.RandomState(77)
    for trial in range(300):
        gridn, _, pts, _, _ = _random_board(rng, trial, clean=False)
        yield "ambiguous_%03d" % trial, gridn, pts, None


def _lattice(gridn, u, v, origin=(700000, 500000), columns=None):
    """origin + c_j * u + i * v in board order (row i, column j); columns = the c_j (default 0 .. gridn-1)."""
    c = np.arange(gridn, dtype=np.float64) if columns is None else np.asarray(columns, dtype=np.float64)
    ii, jj = np.meshgrid(np.arange(gridn), np.arange(gridn), indexing="ij")
    xy = np.array(origin)[None, :] + c[jj.ravel()][:, None] * np.array(u)[None, :] + ii.ravel()[:, None] * np.array(v)[None, :]
    return np.round(xy).astype(np.int64)


def _shuffled(truth, seed, extra=None):
    rng = np.random.RandomState(seed)
    pts = truth if extra is None else np.concatenate([truth, np.asarray(extra, dtype=np.int64).reshape(-1, 2)])
    return pts[rng.permutation(len(pts))].astype(np.int32)


def exact_lattice_cases():
    """Integer lattices without any noise.  Axis-aligned and sheared ones have exactly horizontal rows: ties in the
    "lowest y" top-edge logic (find_grid.cc:1105, :1118).  Squares along an integer vector and its quarter turn have
    every quad cocircular; those along (1, 1) also tie in the "more horizontal" choice (:1185)."""
    for gridn in (3, 4, 10, 14):
        t = _lattice(gridn, (60000, 0), (0, 60000))
        yield "exact_axis_g%d" % gridn, gridn, _shuffled(t, gridn), t
        t = _lattice(gridn, (60000, 0), (17000, 55000))
        yield "exact_shear_g%d" % gridn, gridn, _shuffled(t, 10 + gridn), t
        for k, (a, b) in enumerate([(48000, 14000), (56000, -33000), (40000, 9000)]):
            t = _lattice(gridn, (a, b), (-b, a))
            yield "exact_rotated%d_g%d" % (k, gridn), gridn, _shuffled(t, 20 + gridn + k), t
        # horizontal rows again, sheared the other way: the leftmost corner is a bottom corner, and the cycles start there
        t = _lattice(gridn, (60000, 0), (-17000, 55000))
        yield "exact_shearback_g%d" % gridn, gridn, _shuffled(t, 30 + gridn), t
        # squares standing on a corner: the two edges at the lowest vertex are equally horizontal, the slope tie of :1185
        for k, (a, b) in enumerate([(35000, 35000), (35000, -35000)]):
            t = _lattice(gridn, (a, b), (-b, a))
            yield "exact_diagonal%d_g%d" % (k, gridn), gridn, _shuffled(t, 40 + gridn + k), t


def jittered_axis_cases():
    """Axis-aligned lattices with every coordinate moved by a uniform integer in [-a, a] units (a unit is 1/1000 px):
    the horizontal-row ties of the exact lattice, broken at random."""
    for gridn in (10, 4):
        for amp in (1, 5, 50):
            for seed in range(12):
                rng = np.random.RandomState(1000 * amp + seed)
                t = _lattice(gridn, (60000, 0), (0, 60000)) + rng.randint(-amp, amp + 1, (gridn * gridn, 2))
                yield "jitter%d_g%d_s%02d" % (amp, gridn, seed), gridn, _shuffled(t, seed), t


def threshold_cases():
    """Boards that sit at the sequence tests' limits (find_grid.cc:204-207), gridn 4 so that the deviation test (more
    than two ratios seen) stays out of it.  ratio: the first column gap is r pitches wide -- walking towards it the
    last length ratio is r against the 1.4 limit, walking away from it 1/r against 0.7.  angle: the last column is
    moved along the columns' direction so that the rows' last step turns by the given angle, against acos(0.984) =
    10.263 degrees."""
    u, v = (48000, 14000), (-14000, 48000)                       # |u| = |v| = 50000, a quarter turn apart
    for r in (1.3, 1.39, 1.399, 1.401, 1.41, 1.425, 1.43, 1.45, 1.49, 1.51):
        t = _lattice(4, u, v, columns=[0, r, r + 1, r + 2])
        yield "ratio_%s" % str(r).replace(".", "p"), 4, _shuffled(t, int(r * 1000)), t
    for deg in (9.5, 10.2, 10.25, 10.27, 10.3, 10.8, 11.4, 11.6, 12.5):
        t = _lattice(4, u, v)
        d = np.tan(np.deg2rad(deg))
        t[3::4] += np.round(d * np.array(v)).astype(np.int64)[None, :]          # column 3 of every row
        yield "angle_%s" % str(deg).replace(".", "p"), 4, _shuffled(t, int(deg * 100)), t


def small_and_degenerate_cases():
    """Exact duplicates, sets of 0, 1 and 2 points, all-collinear sets, gridn 2, outliers around and inside a
    lattice of exact squares."""
    rot = _lattice(10, (48000, 14000), (-14000, 48000))
    Hm = _rot(6)
    Hm[2, 0] = 1.5e-4
    pts, truth = _board(10, Hm, jitter=0.2, seed=3)
    yield "dup_some", 10, np.concatenate([pts, pts[:7]]), truth
    yield "dup_all", 10, np.concatenate([pts, pts[::-1]]), truth
    yield "dup_exact_squares", 10, _shuffled(rot, 5, extra=rot[::3]), rot
    yield "dup_triple", 10, np.concatenate([pts, pts[:3], pts[:3]]), truth
    for gridn in (2, 3, 10):
        yield "empty_g%d" % gridn, gridn, np.zeros((0, 2), np.int32), None
        yield "one_g%d" % gridn, gridn, np.array([[123000, 456000]], np.int32), None
        yield "two_g%d" % gridn, gridn, np.array([[123000, 456000], [183000, 456000]], np.int32), None
    yield "two_same_g3", 3, np.array([[5000, 5000], [5000, 5000]], np.int32), None
    k = np.arange(120)
    yield "line_sloped", 10, np.stack([k * 10000, k * 5000], 1).astype(np.int32), None
    yield "line_horizontal", 10, _shuffled(np.stack([k * 7000, 0 * k + 90000], 1), 1), None
    yield "line_vertical", 4, _shuffled(np.stack([0 * k[:20] + 90000, k[:20] * 7000], 1), 2), None
    yield "line_with_duplicates", 3, np.stack([k[:12] // 2 * 3000, k[:12] // 2 * 9000], 1).astype(np.int32), None
    yield "line_uneven_g3", 3, np.array([[0, 0], [1000, 1000], [2000, 2000], [3500, 3500], [4000, 4000], [9000, 9000],
                                         [10000, 10000], [11000, 11000], [12000, 12000]], np.int32), None
    for gridn in (2, 3):                                           # gridn 2: no step to walk, no sequence, no board
        t = _lattice(gridn, (48000, 14000), (-14000, 48000))
        yield "tiny_g2_on_%dx%d" % (gridn, gridn), 2, _shuffled(t, gridn), None
    # outliers: well outside the lattice, on its own pitch just outside, and inside its cells
    rng = np.random.RandomState(9)
    lo, hi = rot.min(0), rot.max(0)
    far = np.stack([rng.randint(lo[0] - 400000, hi[0] + 400000, 60), rng.randint(lo[1] - 400000, hi[1] + 400000, 60)], 1)
    far = far[((far[:, None, :] - rot[None, :, :]).astype(np.float64) ** 2).sum(-1).min(1) > (1.6 * 50000) ** 2]
    yield "outliers_outside", 10, _shuffled(rot, 6, extra=far), rot
    ring = _lattice(12, (48000, 14000), (-14000, 48000), origin=(700000 - 48000 + 14000, 500000 - 14000 - 48000))
    on_pitch = ring[[0, 5, 11, 12 * 11, 12 * 6 + 11]]              # lattice positions one pitch outside the board
    yield "outliers_on_the_pitch", 10, _shuffled(rot, 7, extra=on_pitch), rot
    for n_in in (1, 3, 8):
        cells = rng.randint(0, 9, (n_in, 2))
        frac = rng.uniform(0.2, 0.8, (n_in, 2))
        inside = rot[0][None, :] + np.round((cells[:, :1] + frac[:, :1]) * np.array([48000, 14000])[None, :]
                                            + (cells[:, 1:] + frac[:, 1:]) * np.array([-14000, 48000])[None, :]).astype(np.int64)
        yield "outliers_inside_%d" % n_in, 10, _shuffled(rot, 8 + n_in, extra=inside), rot
    centre = (rot[0] + rot[11]) // 2                               # the centre of a cell: cocircular with its corners
    yield "outlier_at_a_cell_centre", 10, _shuffled(rot, 12, extra=[centre]), rot


def cocircular_cases():
    """Exact squares and 5:6 rectangles along random integer vectors -- every cell cocircular, every Voronoi vertex
    degenerate -- with a few outliers: at random around and inside the lattice, or exactly at cell centres (cocircular
    with the cell's corners: the lattice edge between two such cells has zero length in the Voronoi diagram and is no
    neighbourhood) and at the midpoints of lattice edges (collinear with their ends).  A triangulation has to put
    diagonals where the diagram has none; a finder that walks them answers differently from upstream here."""
    rng = np.random.RandomState(4)
    for it in range(200):
        gridn = int(rng.choice([3, 4, 5, 6, 10]))
        a, b = int(rng.randint(20, 70)) * 1000, int(rng.randint(-40, 40)) * 1000
        kind = it % 4
        u, v = ((a, b), (-b, a)) if kind != 3 else ((a, b), (-6 * b // 5, 6 * a // 5))
        t = _lattice(gridn, u, v, origin=(1500000, 1500000))
        extra = None
        if kind == 1:
            lo, hi = t.min(0), t.max(0)
            k = int(rng.randint(1, 8))
            extra = np.stack([rng.randint(lo[0] - 100000, hi[0] + 100000, k), rng.randint(lo[1] - 100000, hi[1] + 100000, k)], 1)
        elif kind == 2:
            cells = rng.randint(0, gridn - 1, (int(rng.randint(1, 4)), 2))
            extra = np.array([(t[i * gridn + j] + t[(i + 1) * gridn + j + 1]) // 2 if rng.rand() < 0.5
                              else (t[i * gridn + j] + t[i * gridn + j + 1]) // 2 for i, j in cells])
        yield "cocircular_%03d" % it, gridn, _shuffled(t, it, extra), (t if kind in (0, 3) and 2 * abs(b) < a else None)      # (turned further, which edge is "top" is upstream's say)


def golden_candidate_cases(golden_dir=None):
    """The detector's candidate sets of the baseline-size synthetic frames (tests/golden/grid_candidates.npz)."""
    golden_dir = golden_dir or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    z = np.load(os.path.join(golden_dir, "grid_candidates.npz"))
    for key in sorted(z.files):
        gridn = int(key.split("_board")[1].split("_")[0])
        yield key, gridn, z[key].astype(np.int32), None


def degenerate_cases(golden_dir=None):
    for gen in (exact_lattice_cases(), jittered_axis_cases(), threshold_cases(), small_and_degenerate_cases(),
                cocircular_cases(), golden_candidate_cases(golden_dir)):
        for case in gen:
            yield case


def all_cases(golden_dir=None):
    for gen in (clean_sets(), ambiguous_sets(), degenerate_cases(golden_dir)):
        for case in gen:
            yield case


def input_hash(gridn, pts):
    """First 8 bytes of the SHA-256 of gridn and the points, as an integer: catches drift of the generators."""
    h = hashlib.sha256(np.int32(gridn).tobytes() + np.ascontiguousarray(pts, dtype="<i4").tobytes()).digest()
    return int.from_bytes(h[:8], "little")


def indices_of(board, pts):
    """A board (float64 corners = input points / 1000, find_grid.cc:353-354) as indices into `pts` (the first of
    equal points)."""
    first = {}
    for i, p in enumerate(np.asarray(pts).tolist()):
        first.setdefault(tuple(p), i)
    return np.array([first[tuple(p)] for p in np.round(board * 1000).astype(np.int64).tolist()], dtype=np.int32)


def board_of(indices, pts):
    """The inverse of indices_of, double for double."""
    return np.asarray(pts, dtype=np.int32)[indices].astype(np.float64) / 1000.0
