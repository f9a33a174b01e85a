"""No result depends on what context scratch held before the call.

Every other GPU test starts on a fresh Detector, whose device memory reads as zero in practice, or repeats the same frames,
so that what a call left behind is the right data for the next one.  A kernel that reads scratch which nothing of its own
call has written passes all of them.  Here the library's fill hook (csrc/ctx.h, scratch_fill) makes that scratch loud:

  * first use: a fresh Detector with option "scratch_fill", so that every allocation is filled before anyone uses it;
  * reuse: the same calls on the same context after option "scratch_fill_now" has filled every buffer it owns;
  * leftovers of real calls: call A (noise and clutter, the full batch and size) on every scratch set, then call B (fewer
    or smaller frames; clean, all-zero and constant ones) on the same context, with and without a fill in between;
  * the contexts no caller holds: a child process with MRGINGHAM_AMD_SCRATCH_FILL in its environment.

The bytes are 0x7F (int16 30000-odd responses, counts of 2e9, doubles of 1e306) and 0xFF (-1 counts and indices, NaN doubles,
the largest sort key, and the hot list's "no pixel" word).  Every comparison is equality with the yardstick the entry
point's own test uses (tests/scratch_cases.py): the oracle, the array a file was written from, read_image, a fixture's luma
plane, and for the board finder the synchronous dense schedule of a context that was never filled."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scratch_cases as sc
from scratch_cases import FILL_BYTES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "scratch_child.py")


def _id(byte):
    return f"fill{byte:02X}"


fill = pytest.mark.parametrize("byte", FILL_BYTES, ids=_id)


# ---- the hook itself -------------------------------------------------------------------------------------------------
def test_the_hook_fills_and_keeps_the_state_words():
    """scratch_fill_now is not vacuous (the context owns scratch, and a refused value is refused), it completes what is
    in flight, and the state it must leave alone -- the fallback counter, the status words -- survives it."""
    import mrgingham_amd
    s = sc.search()
    det = mrgingham_amd.Detector(0)
    try:
        assert det.scratch_bytes() == 0
        det.set_option("scratch_fill_now", 0x7F)                 # nothing to fill yet: not an error
        for bad in (("scratch_fill", 256), ("scratch_fill", -2), ("scratch_fill_now", -1), ("scratch_fill_now", 256)):
            with pytest.raises(ValueError):
                det.set_option(*bad)
        det.set_option("sparse_refine", 2)
        out = det.chain(sc.dev(s.frames), start_level=3, max_points=1024, sync=False)      # in flight when the fill comes
        det.set_option("scratch_fill_now", 0xFF)
        for f, (wp, wl) in enumerate(s.chain):                   # (the call completed first, its outputs are the caller's)
            assert int(out[2][f]) == len(wl) and np.array_equal(out[0][f, :len(wl)].cpu().numpy(), wp), f
        assert det.scratch_bytes() > 0
        assert 0 <= det.sparse_fallbacks() <= len(s.frames)      # (0xFF in the counter would read as -1, 0x7F as 2e9)
        det.sync()                                               # (a filled status word would fail the sync)
        det.set_option("scratch_fill", 0x7F)
        det.set_option("scratch_fill", -1)
    finally:
        det.close()


# ---- component search --------------------------------------------------------------------------------------------------
# (cc_lds, sparse_refine, sparse_subsets): the searches out of LDS and in global memory (the users of arena / parent / roots),
# the dense and the sparse schedule with one and with two workgroups per frame; each with the pixel stream's four launch plans
SEARCH = [(1, 0, 2), (1, 2, 1), (1, 2, 2), (0, 0, 2)]
PLANS = [(1, 1), (0, 0), (0, 1), (1, 0)]


@fill
@pytest.mark.parametrize("multi,fuse", PLANS, ids=[f"multi{m}_fuse{f}" for m, f in PLANS])
@pytest.mark.parametrize("lds,sparse,subsets", SEARCH, ids=[f"lds{a}_sparse{b}_subsets{c}" for a, b, c in SEARCH])
def test_component_search(byte, lds, sparse, subsets, multi, fuse):
    """detect at levels 0 and 2, chain from level 3, refine at level 0 and both entry points on a caller's response: a board,
    a cluttered board, smoothed noise and an all-zero frame, with a table entry for every pixel (lists compared exactly)."""
    s = sc.search()

    def run(det, what):
        what = (what, byte, lds, sparse, subsets, multi, fuse)
        sc.check_detect(det, s, 0, what)
        sc.check_detect(det, s, 2, what)
        sc.check_chain(det, s, what)
        sc.check_refine(det, s, what)
        sc.check_on_response(det, s, what)
        assert (det.chain_info()[1] == -1) == (sparse == 2)    # the schedule the case is about took the chain
    sc.first_use_then_reuse(byte, run, cc_lds=lds, hot_capacity_shift=0, sparse_refine=sparse, sparse_subsets=subsets,
                            multi_level_launch=multi, fuse_pyramid=fuse)


@fill
def test_component_search_with_the_default_tables(byte):
    """The same calls with the tables at their default fraction of the pixels (the capacity retry grows them where a frame
    asks: new allocations in the middle of a call sequence)."""
    s = sc.search()

    def run(det, what):
        sc.check_detect(det, s, 0, (what, byte))
        sc.check_chain(det, s, (what, byte))
        sc.check_refine(det, s, (what, byte))
    sc.first_use_then_reuse(byte, run)


# ---- ChESS response, preprocessing, blobs --------------------------------------------------------------------------------
@fill
def test_chess_response(byte):
    sc.first_use_then_reuse(byte, sc.check_chess)


@fill
@pytest.mark.parametrize("fused", [1, 0])
def test_preprocess_8_bit(byte, fused):
    sc.first_use_then_reuse(byte, sc.check_preprocess8, preprocess_fused=fused)


@fill
@pytest.mark.parametrize("fused", [1, 0])
def test_preprocess_16_bit(byte, fused):
    sc.first_use_then_reuse(byte, sc.check_preprocess16, preprocess_fused=fused)


@fill
@pytest.mark.parametrize("chunk", [0, 1])
def test_blobs(byte, chunk):
    sc.first_use_then_reuse(byte, sc.check_blobs, blob_chunk_frames=chunk)


# ---- boards ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def board_batches():
    """two mixed batches and what the synchronous dense schedule of a context that is never filled finds in them"""
    import mrgingham_amd
    batches = [sc.mixed_batch(10 * i) for i in range(2)]
    ref = mrgingham_amd.Detector(0)
    try:
        ref.set_option("find_boards_pipeline", 0)
        ref.set_option("sparse_refine", 0)
        want = [ref.find_boards(b, gridn=sc.GRIDN, nthreads=4) for b in batches]
    finally:
        ref.close()
    assert any((f >= 0).any() for _, f in want)
    return batches, want


def _same_boards(got, want, what):
    (gb, gf), (wb, wf) = got, want
    assert np.array_equal(gf, wf), (what, gf, wf)
    for f in range(len(wf)):
        if wf[f] >= 0:
            assert np.array_equal(gb[f], wb[f]), (what, f)


@fill
def test_find_boards(byte, board_batches):
    """find_boards, and submit / collect with two batches in flight, under the sparse refinement"""
    batches, want = board_batches

    def run(det, what):
        for i, b in enumerate(batches):
            _same_boards(det.find_boards(b, gridn=sc.GRIDN, nthreads=4), want[i], (what, byte, "find_boards", i))
        jobs = [det.find_boards_submit(b, gridn=sc.GRIDN, nthreads=4) for b in batches]
        for i, job in enumerate(jobs):
            _same_boards(det.find_boards_collect(job), want[i], (what, byte, "submit / collect", i))
    sc.first_use_then_reuse(byte, run, sparse_refine=2)


# ---- loaders -------------------------------------------------------------------------------------------------------------
LISTS = ["jpeg_host", "jpeg_device", "jpeg_device_memset", "jpeg_device_sync", "png8", "png16", "pgm16", "tiff_lzw", "tiff_deflate",
         "bmp", "pnm"]


@pytest.fixture(scope="module")
def lists(tmp_path_factory):
    return sc.file_lists(tmp_path_factory.mktemp("scratch_fill_lists"))


@fill
@pytest.mark.parametrize("name", LISTS)
def test_loaders(byte, name, lists):
    """Every loader with one chunk and with chunks of two files (a partial last chunk follows full ones in the same slot);
    each list holds an unreadable file, whose frame stays zero."""
    assert sorted(lists) == sorted(LISTS)

    def run(det, what):
        for chunk in (0, 2):
            sc.check_file_list(det, lists[name], chunk, (what, byte))
    sc.first_use_then_reuse(byte, run)


# ---- leftovers of real calls --------------------------------------------------------------------------------------------
between = pytest.mark.parametrize("fill_between", (None,) + FILL_BYTES, ids=lambda b: "no_fill" if b is None else _id(b))


@between
@pytest.mark.parametrize("sparse", [0, 2])
def test_leftovers_of_the_component_search(fill_between, sparse):
    """A: six frames of noise and clutter through detect (levels 0 and 2) and chain.  B: three clean frames of the same
    size, then three of half the size (the same buffers, another layout), against the oracle."""
    a, same, half = sc.leftover_search()

    def call_a(det):
        fa = sc.dev(a)
        det.detect(fa, 0, capacity=8192)
        det.detect(fa, 2, capacity=8192)
        det.chain(fa, start_level=3, max_points=1024)

    def check_b(det, what):
        for s in (same, half):
            sc.check_detect(det, s, 0, what)
            sc.check_detect(det, s, 2, what)
            sc.check_chain(det, s, what)
    sc.a_then_b(fill_between, call_a, check_b, sparse_refine=sparse)


@between
def test_leftovers_of_preprocessing(fill_between):
    a8, a16, b8, b16 = sc.leftover_preprocess()

    def call_a(det):
        det.preprocess(sc.dev(a8), clahe=True, blur_radius=1)
        det.preprocess(sc.dev(a8), clahe=True, blur_radius=2)
        det.preprocess(sc.dev16(a16), clahe=True, blur_radius=1)
        det.preprocess(sc.dev16(a16), clahe=True, blur_radius=2)
        det.torch.cuda.synchronize()

    def check_b(det, what):
        sc.check_preprocess8(det, what, b8)
        sc.check_preprocess16(det, what, b16)
    sc.a_then_b(fill_between, call_a, check_b)


@between
def test_leftovers_of_the_blob_detector(fill_between):
    a, b = sc.leftover_blobs()
    sc.a_then_b(fill_between, lambda det: det.blobs(sc.dev(a), nthreads=2), lambda det, what: sc.check_blobs(det, what, b))


@pytest.fixture(scope="module")
def leftover_lists(tmp_path_factory):
    return sc.leftover_file_lists(tmp_path_factory.mktemp("scratch_fill_leftovers"))


@between
@pytest.mark.parametrize("name", LISTS)
def test_leftovers_of_the_loaders(fill_between, name, leftover_lists):
    """A: the readable files of the list, each twice, in chunks of two (both slots full).  B: the head of the list, its
    unreadable file included, in chunks of two and as one chunk."""
    fl, a, b = leftover_lists[name]

    def call_a(det):
        for k, v in fl.options.items():
            det.set_option(k, v)
        det.set_option(fl.chunk_option, 2)
        frames, status = getattr(det, fl.method)(a, nthreads=2, **fl.kw)
        det.set_option(fl.chunk_option, 0)
        assert not status.any()

    def check_b(det, what):
        for chunk in (2, 0):
            sc.check_file_list(det, b, chunk, what)
    sc.a_then_b(fill_between, call_a, check_b)


# ---- the contexts no caller holds ----------------------------------------------------------------------------------------
def _run_child(tmp, job, byte):
    """scratch_child.py in a fresh interpreter, 300 s at the most, with the variable set to `byte` (None: unset)"""
    jpath, opath = os.path.join(tmp, "job.json"), os.path.join(tmp, "out_%s.npz" % ("plain" if byte is None else _id(byte)))
    with open(jpath, "w") as f:
        json.dump(job, f)
    env = {k: v for k, v in os.environ.items() if k != "MRGINGHAM_AMD_SCRATCH_FILL"}
    if byte is not None:
        env["MRGINGHAM_AMD_SCRATCH_FILL"] = "0x%02X" % byte
    r = subprocess.run([sys.executable, CHILD, jpath, opath], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(opath))


@pytest.fixture(scope="module")
def child_job(tmp_path_factory):
    """the job of the child processes, what an unset environment gives for it, and the CPU yardsticks"""
    from mrgingham_amd import synth
    from oracle import oracle
    from tests import bmp_cases as bc, files_cases, pnm_cases as pc, tiff_cases as tc
    tmp = str(tmp_path_factory.mktemp("scratch_fill_child"))
    image = synth.board_frame(sc.W, sc.H, sc.GRIDN, seed=0).numpy()
    dots = synth.dots_frame(320, 240, 5, seed=1).numpy()
    image16 = image.astype(np.uint16) * 16 + 300
    for name, a in (("image", image), ("dots", dots), ("image16", image16)):
        np.save(os.path.join(tmp, name + ".npy"), a)
    files = files_cases.write_all(tmp)
    board = files_cases.board_pixels()
    extra = {"board.tif": os.path.join(tmp, "board.tif"), "board.bmp": os.path.join(tmp, "board.bmp"), "board.pam": os.path.join(tmp, "board.pam")}
    tc.write(extra["board.tif"], board, compression=tc.LZW, predictor=2, rows_per_strip=8)
    with open(extra["board.bmp"], "wb") as f:
        f.write(bc.write(board, 8, bc.grey_ramp()))
    with open(extra["board.pam"], "wb") as f:
        f.write(pc.write(board[..., None], 7, 8, head=pc.pam_head(board.shape[1], board.shape[0], 1, 255, "GRAYSCALE")))
    names = files_cases.mixed_list(files) + list(extra.values())
    job = {"image": os.path.join(tmp, "image.npy"), "dots": os.path.join(tmp, "dots.npy"), "image16": os.path.join(tmp, "image16.npy"),
           "files": [files["board.pgm"], files["board.png"], files[files_cases.BOARD]] + list(extra.values()), "list": names}
    want = {"find_points_0": oracle.find_corners(image, 0), "find_points_2": oracle.find_corners(image, 2),
            "find_points_blobs": oracle.find_blobs(dots), "chess": oracle.chess_response_5(image, fill=0)}
    for blur in (0, 1):
        want[f"preprocess_{blur}"] = oracle.preprocess(image, clahe=True, blur_radius=blur)
        want[f"preprocess16_{blur}"] = oracle.preprocess16(image16, clahe=True, blur_radius=blur)
    return tmp, job, _run_child(tmp, job, None), want, board, names


def _check_child(out, plain, want, board, names, what):
    for key in ("find_points_0", "find_points_2", "find_points_blobs"):
        assert np.array_equal(np.round(out[key] * 1000).astype(np.int64), want[key].astype(np.int64)), (what, key)
    assert np.array_equal(out["find_points_0_again"], out["find_points_0"]), what
    for key in ("chess", "preprocess_0", "preprocess_1", "preprocess16_0", "preprocess16_1"):
        assert np.array_equal(out[key], want[key]), (what, key)
    for i in range(6):
        assert np.array_equal(out[f"read_image_{i}"], board), (what, "read_image", i)
    assert out["find_board"].shape == (sc.GRIDN * sc.GRIDN, 2) and out["find_board_level2"].shape == (sc.GRIDN * sc.GRIDN, 2), what
    for key in ("find_board", "find_board_level2", "files_levels", "files_found", "files_status", "files_device_loader"):
        assert np.array_equal(out[key], plain[key]), (what, key)
    assert np.array_equal(out["find_board_again"], out["find_board"]), what
    assert np.array_equal(out["files_boards"], plain["files_boards"], equal_nan=True), what
    # the same pixels through six loaders (PGM, PNG, JPEG decode to them; TIFF, BMP and PAM were written from them): one board
    same = [i for i, n in enumerate(names) if os.path.basename(n) in ("board.pgm", "board.png", "board.tif", "board.bmp", "board.pam")]
    assert len(same) >= 7 and out["files_found"][same[0]] >= 0
    for i in same[1:]:
        assert np.array_equal(out["files_boards"][i], out["files_boards"][same[0]]), (what, names[i])
    assert out["files_device_loader"] > 0 and (out["files_status"] == 0).sum() >= 20


def test_an_unset_environment_equals_the_cpu_yardsticks(child_job):
    tmp, job, plain, want, board, names = child_job
    _check_child(plain, plain, want, board, names, "unset")


@fill
def test_contexts_no_caller_holds(byte, child_job):
    """find_points, find_board, ChESS_response_5, preprocess / preprocess16, read_image and one find_boards_files over the
    mixed list with every device route on, in a process whose environment fills every context's allocations."""
    tmp, job, plain, want, board, names = child_job
    _check_child(_run_child(tmp, job, byte), plain, want, board, names, _id(byte))
