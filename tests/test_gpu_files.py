"""A list of image files to boards on the device (mrgingham_amd.find_boards_files, the tool's --batch mode,
mrgingham_amd_find_boards_submit_ex): per file exactly what the decoder followed by the one-image path gives -- status,
found level, the boards double for double, the corners' levels -- whatever the chunk size, the thread count, the entropy
route or the file's place in the list.  No tolerance anywhere.

Files: tests/files_cases.py (the committed JPEG fixtures, PGM / PNG / 16-bit copies of the 640x480 board, one missing
path; lists of at most 24 names).  Every call into find_boards_files runs in a fresh child process under a time limit
(tests/files_child.py): a pipeline that waits for ever fails its test.  The children are started once per module and
their results shared."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import files_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mrgingham_amd", "bin", "mrgingham-amd-from-image")
CHILD = os.path.join(ROOT, "tests", "files_child.py")
STATS = ("chunks", "files_device_loader", "files_host_decoded", "files_one_image", "files_unreadable",
         "ms_detector_waited_for_chunk", "ms_loader_waited_for_slot")


def run_child(tmp, job):
    """The job in a process of its own, 120 s at the most -> the arrays it left."""
    jpath, opath = os.path.join(tmp, "job.json"), os.path.join(tmp, "out.npz")
    with open(jpath, "w") as f:
        json.dump(job, f)
    r = subprocess.run([sys.executable, CHILD, jpath, opath], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(opath))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return files_cases.write_all(tmp_path_factory.mktemp("files"))


# ---- equality with the one-image path -----------------------------------------------------------------------------
MATRIX = [dict(clahe=c, image_pyramid_level=l, refine=r, entropy=e)
          for c, l, r, e in itertools.product((True, False), (-1, 2), (True, False), ("host", "device"))]
MATRIX.append(dict(clahe=False, blur_radius=0, entropy="host"))          # the preprocessing pass is skipped


def matrix_id(kw):
    return "_".join(f"{k[:5]}{v}" for k, v in kw.items()).replace("-", "m")


@pytest.fixture(scope="module")
def matrix(files, tmp_path_factory):
    paths = files_cases.mixed_list(files)
    runs = [{"id": matrix_id(kw), "paths": paths, "kw": dict(kw, batch=3, nthreads=4), "ref": True} for kw in MATRIX]
    return paths, run_child(str(tmp_path_factory.mktemp("matrix")), {"runs": runs})


def assert_equals_reference(out, rid, n):
    for what in ("status", "found", "levels"):
        assert np.array_equal(out[f"{rid}_{what}"], out[f"{rid}_ref_{what}"]), (rid, what)
    assert np.array_equal(out[f"{rid}_boards"], out[f"{rid}_ref_boards"], equal_nan=True), rid
    assert len(out[f"{rid}_status"]) == n


@pytest.mark.parametrize("kw", MATRIX, ids=matrix_id)
def test_equals_the_one_image_path(matrix, kw):
    """batch 3 over 24 names of two board sizes and three tiny ones: seams, partial last chunks, buckets taking turns."""
    paths, out = matrix
    rid = matrix_id(kw)
    assert_equals_reference(out, rid, len(paths))
    status, found = out[rid + "_status"], out[rid + "_found"]
    unreadable = [i for i, p in enumerate(paths) if "missing" in p or "progressive" in p]
    assert np.flatnonzero(status != 0).tolist() == unreadable
    assert (found[[i for i, p in enumerate(paths) if os.path.basename(p).startswith("board")]] >= 0).all()   # (the test sees boards)
    assert np.isnan(out[rid + "_boards"][found < 0]).all()
    if not kw.get("refine", True):
        hit = found >= 0
        assert (out[rid + "_levels"][hit] == found[hit, None]).all()        # without refinement: the found level


def test_the_reference_finds_boards_of_both_sizes(matrix):
    """(what makes the equality above worth something: boards of both sizes are found, their levels are levels)"""
    paths, out = matrix
    rid = matrix_id(MATRIX[0])
    found, levels = out[rid + "_ref_found"], out[rid + "_ref_levels"]
    print("found levels of the reference:", found.tolist())
    assert (found >= 0).sum() >= 10                              # the ten 640x480 boards at least
    hit = found >= 0
    assert (levels[hit] <= found[hit, None]).all() and (levels[hit] >= 0).all()
    assert (found[[i for i, p in enumerate(paths) if "320x240" in p]] >= 0).any()


# ---- shapes, progress, stats ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes(files, tmp_path_factory):
    mixed = files_cases.mixed_list(files)
    board = files[files_cases.BOARD]
    six = [board, files["blend_320x240_grey_q90"], files["board.pgm"], board, files["blend_320x240_420_q90"], files["board.png"]]
    lists = {"batch1": (mixed[:9], 1), "batch_large": (mixed, 100), "multiple": (six, 3), "multiple_plus_1": (six + [board], 3),
             "unreadable_only": ([files["missing"], files["progressive_48x64_420"], files["cmyk_16x16"]], 2), "one_file": ([board], 4),
             "one_thread": (mixed[:12], 2)}
    runs = [{"id": k, "paths": p, "kw": {"batch": b, "nthreads": 1 if k == "one_thread" else 4}, "ref": True}
            for k, (p, b) in lists.items()]
    runs.append({"id": "empty", "paths": [], "kw": {"batch": 4, "nthreads": 4}, "ref": True})
    return lists, run_child(str(tmp_path_factory.mktemp("shapes")), {"runs": runs})


@pytest.mark.parametrize("rid", ["batch1", "batch_large", "multiple", "multiple_plus_1", "unreadable_only", "one_file",
                                 "one_thread", "empty"])
def test_shapes(shapes, rid):
    lists, out = shapes
    n = len(lists[rid][0]) if rid in lists else 0
    assert_equals_reference(out, rid, n)
    # progress: non-decreasing, ends at n, and what it called final stayed as it was
    nfinal = out[rid + "_nfinal"]
    assert len(nfinal) >= 1 and (np.diff(nfinal) >= 0).all() and nfinal[-1] == n
    assert out[rid + "_snap_ok"].all()
    # stats: the file counts add up; the device loader took the readable JPEG names
    stats = dict(zip(STATS, out[rid + "_stats"]))
    assert stats["files_device_loader"] + stats["files_host_decoded"] + stats["files_one_image"] + stats["files_unreadable"] == n
    assert stats["files_unreadable"] == (out[rid + "_status"] != 0).sum()
    if rid in lists:
        paths = lists[rid][0]
        ok = out[rid + "_status"] == 0
        assert stats["files_device_loader"] == sum(1 for p, k in zip(paths, ok) if k and p.endswith(".jpg"))
        assert stats["files_one_image"] == sum(1 for p in paths if p.endswith("board16.pgm"))
        assert stats["files_host_decoded"] == sum(1 for p in paths if p.endswith(("board.pgm", "board.png")))
    if rid == "unreadable_only":
        assert stats["chunks"] == 0 and (out[rid + "_status"] == -1).all() and (out[rid + "_found"] == -1).all()
    if rid in ("multiple", "multiple_plus_1"):
        assert stats["chunks"] == 3          # 640x480: three files, then the rest after the 320x240 chunk in between
    assert stats["ms_detector_waited_for_chunk"] >= 0 and stats["ms_loader_waited_for_slot"] >= 0


def test_progress_reports_a_growing_prefix_while_chunks_complete(shapes):
    lists, out = shapes
    nfinal = out["batch1_nfinal"]
    assert len(set(nfinal.tolist())) >= 4          # several chunks: the prefix moved several times, not once at the end


# ---- find_boards_submit_ex ------------------------------------------------------------------------------------------
def test_submit_ex_gives_the_levels_of_the_one_image_path(files):
    import ctypes
    import torch
    import mrgingham_amd
    from mrgingham_amd import _lib
    L = _lib.lib()
    L.mrgingham_amd_process_image.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 8 + [ctypes.c_void_p] * 2
    img = mrgingham_amd.read_image(files[files_cases.BOARD])
    frames = torch.from_numpy(np.stack([img] * 4)).cuda()
    det = mrgingham_amd.Detector()
    try:
        for refine in (True, False):
            xy, lv = np.zeros((100, 2)), np.full(100, -9, np.int8)
            level = L.mrgingham_amd_process_image(img.ctypes.data, 640, 480, 640, 0, 0, 10, -1, int(refine), xy.ctypes.data, lv.ctypes.data)
            assert level >= 0
            boards, found, levels = det.find_boards(frames, gridn=10, refine=refine, levels=True)
            assert levels.dtype == np.int8 and levels.shape == (4, 100)
            for f in range(4):
                assert found[f] == level and np.array_equal(boards[f], xy) and np.array_equal(levels[f], lv)
            assert (lv <= level).all() and (lv >= 0).all()
            if not refine:
                assert (lv == level).all()
            # no levels asked for (h_levels NULL): what find_boards_submit gives
            b0, f0 = det.find_boards_collect(det.find_boards_submit(frames, gridn=10))
            b1, f1 = det.find_boards(frames, gridn=10, refine=True, levels=False)
            job = det.find_boards_submit(frames, gridn=10, refine=refine)
            assert len(job) == 4
            b2, f2 = det.find_boards_collect(job)
            assert np.array_equal(b0, b1) and np.array_equal(f0, f1) and np.array_equal(f2, found) and np.array_equal(b2, boards)
    finally:
        det.close()


# ---- the tool -------------------------------------------------------------------------------------------------------
def parse_vnlog(text):
    """-> ([file names in the order their records begin], {name: [record lines]}, [comment lines])"""
    order, records, comments = [], {}, []
    for line in text.splitlines():
        if line.startswith("#"):
            comments.append(line)
            continue
        name = line.split(" ", 1)[0]
        if not order or order[-1] != name:
            order.append(name)
        records.setdefault(name, []).append(line)
    return order, records, comments


def run_tool(*args):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)
    return r


@pytest.mark.parametrize("extra", [(), ("--no-refine",), ("--jpeg-entropy", "device")], ids=["default", "no_refine", "device_entropy"])
def test_tool_batch_equals_the_tool_without_batch(files, extra):
    # every name once (the tool's records are keyed by name), the unreadable ones left out first.  A name that does not
    # exist never reaches the tool's workers (its glob fails): a file cut off inside its header stands in for it
    cut = os.path.join(os.path.dirname(files["missing"]), "cut_off.jpg")
    with open(cut, "wb") as f:
        f.write(open(files[files_cases.BOARD], "rb").read()[:100])
    names = [cut if p == files["missing"] else p for p in dict.fromkeys(files_cases.mixed_list(files))]
    readable = [p for p in names if p != cut and "progressive" not in p]
    plain = run_tool("--jobs", "1", *[a for a in extra if a not in ("--jpeg-entropy", "device")], *readable)
    batch = run_tool("--jobs", "4", "--batch", "3", *extra, *readable)
    assert plain.returncode == 0 and batch.returncode == 0, plain.stderr + batch.stderr
    order_p, rec_p, _ = parse_vnlog(plain.stdout)
    order_b, rec_b, com_b = parse_vnlog(batch.stdout)
    assert order_b == readable                                   # list order
    assert rec_b == rec_p
    assert any(len(v) == 100 for v in rec_b.values()) and com_b[-1] == "# filename x y level"
    # with the unreadable names: two lines each, the files after them still processed, exit status 0
    r = run_tool("--jobs", "4", "--batch", "3", *extra, *names)
    assert r.returncode == 0, r.stderr
    order, rec, comments = parse_vnlog(r.stdout)
    assert order == names
    for p in names:
        if p in rec_p:
            assert rec[p] == rec_p[p]
        else:
            assert rec[p] == [f"{p} - - -"] and f"## Couldn't open image '{p}'" in comments
            assert f"Couldn't open image '{p}'" in r.stderr
    # ... and each "## Couldn't open" line stands right in front of its record
    lines = r.stdout.splitlines()
    for p in names:
        if p not in rec_p:
            assert lines[lines.index(f"## Couldn't open image '{p}'") + 1] == f"{p} - - -"


# ---- independence ---------------------------------------------------------------------------------------------------
def test_a_detector_with_a_job_in_flight_is_left_alone(files, tmp_path):
    paths = [files[files_cases.BOARD], files["blend_320x240_grey_q90"], files["board.pgm"], files["board16.pgm"], files[files_cases.BOARD]]
    out = run_child(str(tmp_path), {"independence": {"paths": paths}})
    assert_equals_reference(out, "between", len(paths))
    assert (out["ind_want_found"] >= 0).all()
    for k in ("got", "again"):
        assert np.array_equal(out[f"ind_{k}_found"], out["ind_want_found"])
        assert np.array_equal(out[f"ind_{k}_boards"], out["ind_want_boards"])
