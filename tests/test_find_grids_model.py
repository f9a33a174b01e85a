"""The host model of the device grid finder (mrgingham_amd_find_grids_host: csrc/grid_phases.h run serially), CPU.

The model is the text the kernel runs (tests/test_gpu_find_grids.py holds the kernel to it, list for list), so what is
pinned here holds on the device: every list it ANSWERS equals the host finder at the canonical ring start, double for
double after / 1000.0, and upstream's recorded answer; it declines nothing in the families that matter, nothing
anywhere for the guard band's sake at the default band, and exactly the lists that sit on a threshold.  Integer
indices and exact doubles: every check is an equality."""
import collections
import os
import subprocess

import numpy as np
import pytest

import mrgingham_amd
from mrgingham_amd import api
from tests import find_grids_cases as fc
from tests import grid_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrgingham_amd", "csrc")


@pytest.fixture(scope="module")
def corpus(golden_dir):
    """{gridn: (names, lists, xy, counts, index, status, boards)}: the model at the default band, once."""
    out = {}
    for gridn, (names, lists, xy, counts) in fc.corpus_batches(golden_dir).items():
        index, status = mrgingham_amd.find_grids_host(xy, counts, gridn)
        out[gridn] = (names, lists, xy, counts, index, status, mrgingham_amd.boards_of_indices(xy, index, status))
    return out


@pytest.fixture(scope="module")
def host(corpus):
    """The host finder at the canonical ring start, once: {name: board or None}."""
    return {name: api.find_grid_from_points_perturbed(pts, gridn, canonical_start=True)
            for gridn, (names, lists, *_) in corpus.items() for name, pts in zip(names, lists)}


def _answers_equal(names, status, boards, want_of):
    """Every answered list: status 1 with the wanted board double for double, status 0 exactly where none is wanted."""
    for i, name in enumerate(names):
        want = want_of(name)
        if status[i] < 0:
            continue
        assert status[i] == (1 if want is not None else 0), (name, int(status[i]))
        if want is not None:
            assert np.array_equal(boards[i], want), name
        else:
            assert np.isnan(boards[i]).all(), name


def test_corpus_is_the_whole_of_grid_cases(corpus):
    assert sum(len(v[0]) for v in corpus.values()) == 1166
    assert max(int(v[3].max()) for v in corpus.values()) == 261 and set(corpus) == {2, 3, 4, 5, 6, 10, 14}


def test_answers_equal_the_host_finder_at_the_canonical_start(corpus, host):
    for gridn, (names, lists, xy, counts, index, status, boards) in corpus.items():
        _answers_equal(names, status, boards, host.get)
        for i in np.nonzero(status != 1)[0]:
            assert (index[i] == -1).all(), names[i]
        for i in np.nonzero(status == 1)[0]:
            assert ((index[i] >= 0) & (index[i] < counts[i])).all(), names[i]


def test_answers_equal_recorded_upstream(corpus, golden_dir):
    """Replayed against tests/golden/grid_kat.npz as tests/test_oracle_grid.py replays it."""
    z = np.load(os.path.join(golden_dir, "grid_kat.npz"))
    off, idx = z["offsets"], z["indices"].astype(np.int64)
    kat = {str(n): (int(g), int(h), bool(f), idx[off[i]:off[i + 1]])
           for i, (n, g, h, f) in enumerate(zip(z["names"], z["gridn"], z["hash"], z["found"]))}
    nfound = 0
    for gridn, (names, lists, xy, counts, index, status, boards) in corpus.items():
        pts_of = dict(zip(names, lists))
        for name in names:
            assert kat[name][:2] == (gridn, gc.input_hash(gridn, pts_of[name])), name
        _answers_equal(names, status, boards, lambda n: gc.board_of(kat[n][3], pts_of[n]) if kat[n][2] else None)
        nfound += int((status == 1).sum())
    assert nfound >= 700, nfound


def test_what_is_declined_and_where(corpus, capsys):
    """None of the sets of the families clean, ambiguous, jitter*, ratio_*, angle_* and the golden device candidates (500 +
    300 + 72 + 10 + 9 + 16 = 907) for any reason; nowhere in the corpus for the guard band's sake; for a degenerate neighbour structure only among
    the exact and cocircular lattices and the small and degenerate sets."""
    declined = collections.Counter()
    never = 0
    for gridn, (names, lists, xy, counts, index, status, boards) in corpus.items():
        for name, st in zip(names, status.tolist()):
            if name.startswith(fc.NEVER_DECLINED):
                never += 1
                assert st >= 0, (name, st)
            assert st != -3, name
            if st == -2:
                assert name.startswith(fc.RING_DECLINES_ALLOWED), name
            if st < 0:
                declined[(name.split("_")[0], st)] += 1
    assert never == 907, never
    with capsys.disabled():
        print("\n  find_grids model: declined over the corpus: %d of 1166 %s" % (sum(declined.values()), dict(declined)))


def test_a_wide_guard_band_declines_and_changes_no_answer(corpus, host):
    ndeclined = 0
    for gridn, (names, lists, xy, counts, index, status, boards) in corpus.items():
        index10, status10 = mrgingham_amd.find_grids_host(xy, counts, gridn, guard_bits=10)
        _answers_equal(names, status10, mrgingham_amd.boards_of_indices(xy, index10, status10), host.get)
        assert set(np.unique(status10[status10 < 0]).tolist()) <= {-3}
        same = status10 >= 0
        assert np.array_equal(status10[same], status[same]) and np.array_equal(index10[same], index[same])
        ndeclined += int((status10 == -3).sum())
    assert ndeclined > 0


def test_lattices_on_a_threshold_are_the_hosts():
    """A length ratio of exactly 1.4 or 0.7: distance 0 from the limit, inside any band.  (The host finds no board on
    them; the device does not say so.)"""
    lists = list(fc.threshold_lattices())
    assert len(lists) == 4
    for pts in lists:
        assert api.find_grid_from_points_perturbed(pts, 4, canonical_start=True) is None
    xy, counts = fc.pack(lists)
    for bits in (33, 45, 8):
        index, status = mrgingham_amd.find_grids_host(xy, counts, 4, guard_bits=bits)
        assert status.tolist() == [-3] * 4 and (index == -1).all(), (bits, status)


def test_layout_cases():
    Hm = gc._rot(4)
    board, truth = gc._board(4, Hm, jitter=0.1, seed=5)
    want = api.find_grid_from_points_perturbed(board, 4, canonical_start=True)
    assert want is not None
    # poison beyond the count, at several capacities, the list at several places of a batch; count 0; count < gridn^2
    for capacity in (16, 17, 512, 700):
        lists = [board, np.zeros((0, 2), np.int32), board[:15], board]
        xy, counts = fc.pack(lists, capacity)
        index, status = mrgingham_amd.find_grids_host(xy, counts, 4)
        assert status.tolist() == [1, 0, 0, 1], capacity
        boards = mrgingham_amd.boards_of_indices(xy, index, status)
        assert np.array_equal(boards[0], want) and np.array_equal(boards[3], want)
        assert np.isnan(boards[1]).all() and (index[1:3] == -1).all()
    # what lies behind the count does not matter
    xy, counts = fc.pack([board], 64)
    index0, _ = mrgingham_amd.find_grids_host(xy, counts, 4)
    xy[0, 16:] = board[:1]
    index1, status1 = mrgingham_amd.find_grids_host(xy, counts, 4)
    assert status1[0] == 1 and np.array_equal(index0, index1)
    # count above the capacity, above the cap, below 0
    geometry = mrgingham_amd.find_grids_geometry()
    assert geometry["max_candidates"] >= 512 and (geometry["min_gridn"], geometry["max_gridn"]) == (2, 16)
    xy, counts = fc.pack([board, board, board], 16)
    counts[:] = [17, -1, 16]
    assert mrgingham_amd.find_grids_host(xy, counts, 4)[1].tolist() == [-1, -1, 1]
    big = geometry["max_candidates"] + 1
    xy = np.zeros((1, big, 2), np.int32)
    xy[0, :, 0] = np.arange(big) * 1000
    xy[0, :, 1] = (np.arange(big) % 7) * 1000
    assert mrgingham_amd.find_grids_host(xy, np.array([big], np.int32), 4)[1].tolist() == [-1]
    assert mrgingham_amd.find_grids_host(xy, np.array([big - 1], np.int32), 4)[1][0] != -1
    # a coordinate of 2^24 (and of -2^24) is out of range, one below is not
    for value, st in ((1 << 24, -5), (-(1 << 24), -5), ((1 << 24) - 1, 1)):
        moved = board.astype(np.int64)
        moved += value - moved.max() if value > 0 else value - moved.min()
        assert (np.abs(moved) <= 1 << 24).all()
        xy, counts = fc.pack([moved.astype(np.int32)], 32)
        assert mrgingham_amd.find_grids_host(xy, counts, 4)[1].tolist() == [st], value
    # gridn 2: no step to walk, no sequence, no board -- as on the host
    square = gc._lattice(2, (48000, 14000), (-14000, 48000)).astype(np.int32)
    assert api.find_grid_from_points_perturbed(square, 2, canonical_start=True) is None
    xy, counts = fc.pack([square, board])
    assert mrgingham_amd.find_grids_host(xy, counts, 2)[1].tolist() == [0, 0]
    # arguments
    for gridn, bits in ((1, 33), (17, 33), (4, 7), (4, 46)):
        with pytest.raises(ValueError):
            mrgingham_amd.find_grids_host(xy, counts, gridn, guard_bits=bits)


def test_model_under_address_and_undefined_sanitizers(corpus, tmp_path):
    """tests/boundary/grid_model_main.cpp: the corpus and 300 lists of random garbage -- counts below 0 and above the
    capacity, coordinates over all of int32, in a tiny box (duplicates), on a line, on a lattice -- one call per list over
    heap blocks of exactly its candidates and its indices; ends clean, and every status is the library's."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        flags = []  # (the sanitizer runtime of g++ is not installed: the program's own checks still run)
        print("\n  find_grids model: g++ has no sanitizer runtime here, the stand-alone program runs UNSANITIZED")
    exe = str(tmp_path / "grid_model")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, "-I", CSRC,
                        os.path.join(ROOT, "tests", "boundary", "grid_model_main.cpp"), os.path.join(CSRC, "grid_model.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    batches = [(gridn, 33, xy, counts, status) for gridn, (names, lists, xy, counts, index, status, boards) in corpus.items()]
    for k, gridn in enumerate((10, 4, 16)):
        xy, counts = fc.garbage_lists(100 + k, 100)
        batches.append((gridn, 33, xy, counts, mrgingham_amd.find_grids_host(xy, counts, gridn)[1]))
    assert sum(len(b[3]) for b in batches) == 1166 + 300
    path = tmp_path / "batches.bin"
    with open(path, "wb") as fp:
        for gridn, bits, xy, counts, _ in batches:
            fp.write(np.array([len(counts), xy.shape[1], gridn, bits], np.int32).tobytes())
            fp.write(counts.tobytes())
            fp.write(xy.tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(batches) + 1
    for line, (gridn, bits, xy, counts, status) in zip(lines, batches):
        assert [int(v) for v in line.split(":")[1].split()] == status.tolist(), line[:40]
    assert lines[-1].split()[:2] == ["lists", "1466"]
