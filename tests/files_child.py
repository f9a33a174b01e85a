"""Child process of tests/test_gpu_files.py: every call into mrgingham_amd.find_boards_files runs in a process of its
own under the caller's time limit, so that a pipeline that waits for ever fails a test instead of hanging the run.

    python tests/files_child.py job.json out.npz

job.json: {"runs": [{"id": str, "paths": [...], "kw": {find_boards_files keywords}, "ref": bool}, ...],
           "independence": {"paths": [...]} (optional)}.
out.npz, per run: <id>_boards / _levels / _found / _status / _stats (FILES_STATS order) / _nfinal (the progress values) /
_snap_ok (per progress call: did the arrays' entries [0, nfinal) at that moment equal the final ones); with "ref" the
same four arrays as <id>_ref_* from the loop of the decoder and mrgingham_amd_process_image_ex over the same names."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mrgingham_amd  # noqa: E402
from mrgingham_amd import _lib, api  # noqa: E402


class CliOptions(ctypes.Structure):
    """mrgingham_amd_cli_options"""
    _fields_ = [(n, ctypes.c_int) for n in ("do_clahe", "blur_radius", "gridn", "image_pyramid_level", "do_refine", "do_blobs",
                                            "debug", "debug_sequence_x", "debug_sequence_y")] + [("filename", ctypes.c_char_p)]


def decode(path):
    """The decoder's image as the tool hands it to the one-image path: uint8 or uint16 [H, W], or None."""
    probe = mrgingham_amd.probe_image(path)
    if probe is not None and probe[2] == 16 and probe[3] == mrgingham_amd.KIND_PGM:            # 16-bit PGM: the samples as they are
        data = open(path, "rb").read()
        h, w = probe[0], probe[1]
        return np.frombuffer(data[len(data) - 2 * h * w:], ">u2").reshape(h, w).astype(np.uint16)
    assert probe is None or probe[2] == 8, "the lists of these tests hold no 16-bit PNG"
    return mrgingham_amd.read_image(path)


_ref_cache = {}


def reference(paths, gridn=10, image_pyramid_level=-1, clahe=True, blur_radius=1, refine=True, **_):
    key = (tuple(paths), gridn, image_pyramid_level, clahe, blur_radius, refine)
    if key in _ref_cache:
        return _ref_cache[key]
    L = _lib.lib()
    L.mrgingham_amd_process_image_ex.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(CliOptions), ctypes.c_void_p, ctypes.c_void_p]
    n, N = len(paths), gridn * gridn
    boards = np.full((n, N, 2), np.nan)
    levels = np.zeros((n, N), np.int8)
    found = np.full(n, -1, np.int8)
    status = np.full(n, -1, np.int32)
    o = CliOptions(int(clahe), blur_radius, gridn, image_pyramid_level, int(refine), 0, 0, -1, -1, None)
    for i, p in enumerate(paths):
        img = decode(p)
        if img is None:
            continue
        status[i] = 0
        img = np.ascontiguousarray(img)
        xy = np.zeros((N, 2))
        lv = np.zeros(N, np.int8)
        level = L.mrgingham_amd_process_image_ex(img.ctypes.data, 16 if img.dtype == np.uint16 else 8, img.shape[1], img.shape[0],
                                                 img.shape[1], ctypes.byref(o), xy.ctypes.data, lv.ctypes.data)
        if level >= 0:
            found[i], boards[i], levels[i] = level, xy, lv
    _ref_cache[key] = (boards, levels, found, status)
    return _ref_cache[key]


def one_run(run, out):
    rid, paths, kw = run["id"], run["paths"], run.get("kw", {})
    nfinal, snaps = [], []

    def progress(k, boards, levels, found, status):
        nfinal.append(k)
        snaps.append((boards[:k].copy(), levels[:k].copy(), found[:k].copy(), status[:k].copy()))
    boards, levels, found, status, stats = mrgingham_amd.find_boards_files(paths, progress=progress, **kw)
    out[rid + "_boards"], out[rid + "_levels"], out[rid + "_found"], out[rid + "_status"] = boards, levels, found, status
    out[rid + "_stats"] = np.array([stats[k] for k in api.FILES_STATS])
    out[rid + "_nfinal"] = np.array(nfinal, np.int64)
    final = (boards, levels, found, status)
    out[rid + "_snap_ok"] = np.array([all(np.array_equal(s, f[:k], equal_nan=True) for s, f in zip(snap, final))
                                      for k, snap in zip(nfinal, snaps)], bool)
    if run.get("ref"):
        for name, a in zip(("boards", "levels", "found", "status"), reference(paths, **kw)):
            out[rid + "_ref_" + name] = a


def independence(job, out):
    """A Detector of THIS process with a find_boards job in flight, a find_boards_files call in between, the job collected
    afterwards: its boards are the ones a Detector gives that was left alone."""
    import torch
    paths = job["paths"]
    frames = torch.from_numpy(np.stack([mrgingham_amd.read_image(paths[0])] * 3)).cuda()
    det = mrgingham_amd.Detector()
    want_boards, want_found = det.find_boards(frames, gridn=10)
    ticket = det.find_boards_submit(frames, gridn=10)
    one_run({"id": "between", "paths": paths, "kw": {"batch": 2, "nthreads": 4}, "ref": True}, out)
    got_boards, got_found = det.find_boards_collect(ticket)
    again_boards, again_found = det.find_boards(frames, gridn=10)
    out["ind_want_boards"], out["ind_want_found"] = want_boards, want_found
    out["ind_got_boards"], out["ind_got_found"] = got_boards, got_found
    out["ind_again_boards"], out["ind_again_found"] = again_boards, again_found
    det.close()


def main():
    job = json.load(open(sys.argv[1]))
    out = {}
    for run in job.get("runs", []):
        one_run(run, out)
    if "independence" in job:
        independence(job["independence"], out)
    np.savez(sys.argv[2], **out)


if __name__ == "__main__":
    main()
