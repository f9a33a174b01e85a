"""GPU: the device grid finder (Detector.find_grids, csrc/grid_find.hip) against its host model, and find_boards with
option "find_boards_grid".

The model (mrgingham_amd.find_grids_host) is the same text run serially; tests/test_find_grids_model.py holds it to the
host finder and to upstream's recorded answers.  Here the kernel must equal the model list for list -- indices,
statuses, decline reasons --, so everything pinned there holds on the device; and find_boards must report the same
boards, levels and refinement whichever side orders the candidates.  Integers and exact doubles: equalities only."""
import numpy as np
import pytest

import mrgingham_amd
from oracle import oracle
from tests import find_grids_cases as fc
from tests.test_gpu_grid_reference import _batches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus(golden_dir):
    """{gridn: (names, xy, counts, index, status)}: the corpus and the model's answers, once."""
    return {gridn: (names, xy, counts) + mrgingham_amd.find_grids_host(xy, counts, gridn)
            for gridn, (names, lists, xy, counts) in fc.corpus_batches(golden_dir).items()}


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector(0)
    yield d
    d.close()


def _device(det, xy, counts, gridn):
    import torch
    index, status = det.find_grids(torch.from_numpy(xy).cuda(), torch.from_numpy(counts).cuda(), gridn)
    return index.cpu().numpy(), status.cpu().numpy()


def test_kernel_equals_the_model_over_the_corpus(det, corpus):
    """One call per gridn, capacity 512, up to 485 lists: more lists than workgroups of a launch."""
    det.find_grids_stats()
    want = np.zeros(9)
    for gridn, (names, xy, counts, index, status) in corpus.items():
        got_index, got_status = _device(det, xy, counts, gridn)
        bad = np.nonzero(got_status != status)[0]
        assert len(bad) == 0, (gridn, [(names[i], int(got_status[i]), int(status[i])) for i in bad[:5]])
        bad = np.nonzero((got_index != index).any(1))[0]
        assert len(bad) == 0, (gridn, [names[i] for i in bad[:5]])
        want[0] += len(names)
        for st in status.tolist():
            want[2 - st] += 1
    assert max(len(v[0]) for v in corpus.values()) > mrgingham_amd.find_grids_geometry()["max_workgroups"]
    stats = det.find_grids_stats()
    assert [stats[k] for k in det.FIND_GRIDS_STATS] == want.tolist(), stats
    assert det.find_grids_stats()["lists"] == 0


def test_one_list_300_lists_and_garbage(det, corpus):
    names, xy, counts, index, status = corpus[10]
    assert len(names) >= 300
    for n in (1, 300):
        got_index, got_status = _device(det, xy[:n].copy(), counts[:n].copy(), 10)
        assert np.array_equal(got_status, status[:n]) and np.array_equal(got_index, index[:n]), n
    # the lists the model was run over under the sanitizers: every one ends as a status, the model's
    for k, gridn in enumerate((10, 4, 16)):
        gxy, gcounts = fc.garbage_lists(100 + k, 100)
        want_index, want_status = mrgingham_amd.find_grids_host(gxy, gcounts, gridn)
        got_index, got_status = _device(det, gxy, gcounts, gridn)
        assert np.array_equal(got_status, want_status) and np.array_equal(got_index, want_index), gridn
        assert (want_status < 0).any() and (want_status == 0).any()
    # out=, the lattices on a threshold, a wider band through the option, arguments
    import torch
    txy, tcounts = fc.pack(list(fc.threshold_lattices()))
    out = (torch.zeros((4, 16), dtype=torch.int32, device="cuda"), torch.zeros((4,), dtype=torch.int32, device="cuda"))
    assert det.find_grids(torch.from_numpy(txy).cuda(), torch.from_numpy(tcounts).cuda(), 4, out=out)[1] is out[1]
    assert out[1].cpu().tolist() == [-3] * 4 and (out[0].cpu().numpy() == -1).all()
    det.set_option("find_grids_guard_bits", 10)
    try:
        n4, xy4, counts4, _, _ = corpus[4]
        want_index, want_status = mrgingham_amd.find_grids_host(xy4, counts4, 4, guard_bits=10)
        got_index, got_status = _device(det, xy4, counts4, 4)
        assert np.array_equal(got_status, want_status) and np.array_equal(got_index, want_index)
    finally:
        det.set_option("find_grids_guard_bits", 33)
    for name, value in (("find_grids_guard_bits", 7), ("find_grids_guard_bits", 46), ("find_boards_grid", 2)):
        with pytest.raises(ValueError):
            det.set_option(name, value)
    with pytest.raises(RuntimeError):
        det.find_grids(torch.from_numpy(txy).cuda(), torch.from_numpy(tcounts).cuda(), 17)


def test_no_result_depends_on_what_scratch_held(corpus):
    """The hook of DESIGN.md section 3.3: scratch filled with 0x7F at its first use, then refilled with 0xFF at rest."""
    names, xy, counts, index, status = corpus[14]
    d = mrgingham_amd.Detector(0)
    try:
        d.set_option("scratch_fill", 0x7F)
        first = _device(d, xy, counts, 14)
        assert d.scratch_bytes() > 0
        d.set_option("scratch_fill_now", 0xFF)
        second = _device(d, xy, counts, 14)
        for got_index, got_status in (first, second):
            assert np.array_equal(got_status, status) and np.array_equal(got_index, index)
        assert d.find_grids_stats()["lists"] == 2 * len(names)      # (the counters are state: the fill leaves them)
    finally:
        d.close()


@pytest.fixture(scope="module")
def board_batches():
    import torch
    return [(name, gridn, torch.from_numpy(np.stack(imgs)).cuda(), has_board) for name, gridn, imgs, has_board in _batches()]


@pytest.fixture(scope="module")
def host_route(board_batches):
    """find_boards with the host grid finder (the default), once: {(name, refine): (boards, found, levels)}."""
    d = mrgingham_amd.Detector(0)
    try:
        return {(name, refine): d.find_boards(frames, gridn=gridn, refine=refine, levels=True)
                for name, gridn, frames, _ in board_batches for refine in (False, True)}
    finally:
        d.close()


def _same_boards(got, want, where):
    for g, w, what in zip(got, want, ("boards", "found", "levels")):
        assert np.array_equal(g, w, equal_nan=(what == "boards")), (where, what)


def test_find_boards_on_the_device_finder_equals_the_host_route(board_batches, host_route):
    d = mrgingham_amd.Detector(0)
    try:
        d.set_option("find_boards_grid", 1)
        for name, gridn, frames, has_board in board_batches:
            for refine in (False, True):
                got = d.find_boards(frames, gridn=gridn, refine=refine, levels=True)
                _same_boards(got, host_route[(name, refine)], (name, refine))
                assert ((got[1] >= 0) == np.array(has_board)).all(), name
        stats = d.find_grids_stats()
        assert stats["lists"] > 0 and stats["found"] > 0 and stats["none"] > 0, stats
        assert stats["declined_guard"] == 0 and stats["declined_ring"] == 0 and stats["declined_coordinate"] == 0, stats
    finally:
        d.close()


@pytest.mark.skipif(not oracle.have_reference_grid(), reason="oracle/_ref/libgrid_ref.so is not built")
def test_find_boards_on_the_device_finder_equals_upstream_on_the_devices_candidates(board_batches):
    d = mrgingham_amd.Detector(0)
    try:
        d.set_option("find_boards_grid", 1)
        for name, gridn, frames, has_board in board_batches:
            boards, found = d.find_boards(frames, gridn=gridn, refine=False)
            for f in range(frames.shape[0]):
                want, want_level = None, -1
                for L in (3, 2, 1, 0):
                    xy, counts = d.detect(frames[f:f + 1], L, capacity=8192)
                    want = oracle.ref_find_grid(xy[0, :int(counts[0])].cpu().numpy(), gridn)
                    if want is not None:
                        want_level = L
                        break
                assert found[f] == want_level, (name, f)
                assert np.array_equal(boards[f], want) if want is not None else np.isnan(boards[f]).all(), (name, f)
    finally:
        d.close()


def test_find_boards_falls_back_to_the_host_where_the_device_declines(board_batches, host_route):
    """A band of 2^-10 declines lists of these frames: the host finder answers them, and the boards stay."""
    d = mrgingham_amd.Detector(0)
    try:
        d.set_option("find_boards_grid", 1)
        d.set_option("find_grids_guard_bits", 10)
        for name, gridn, frames, _ in board_batches:
            for refine in (False, True):
                _same_boards(d.find_boards(frames, gridn=gridn, refine=refine, levels=True), host_route[(name, refine)], (name, refine))
        stats = d.find_grids_stats()
        assert stats["declined_guard"] > 0 and stats["host_fallbacks"] > 0, stats
    finally:
        d.close()


def test_find_boards_on_the_device_finder_with_three_jobs_in_flight(board_batches, host_route):
    d = mrgingham_amd.Detector(0)
    try:
        d.set_option("find_boards_grid", 1)
        d.set_option("scratch_sets", 3)
        name, gridn, frames, _ = board_batches[0]
        other_name, other_gridn, other, _ = board_batches[3]
        jobs = [d.find_boards_submit(frames, gridn=gridn, refine=True, levels=True),
                d.find_boards_submit(other, gridn=other_gridn, refine=True, levels=True),
                d.find_boards_submit(frames.flip(0).contiguous(), gridn=gridn, refine=True, levels=True)]
        got = [d.find_boards_collect(j) for j in jobs]
        _same_boards(got[0], host_route[(name, True)], name)
        _same_boards(got[1], host_route[(other_name, True)], other_name)
        _same_boards([a[::-1] for a in got[2]], host_route[(name, True)], name + " reversed")
        assert d.find_grids_stats()["lists"] == 3 * (2 * frames.shape[0] + other.shape[0])
    finally:
        d.close()
