"""Child process of tests/test_gpu_scratch_fill.py: the entry points whose contexts no caller holds -- the per-thread
contexts behind the reference's own names, their single-frame context, the loader and detector contexts inside
find_boards_files -- in a fresh interpreter, so that MRGINGHAM_AMD_SCRATCH_FILL in its environment (or its absence) is
what every one of those contexts is created under.

    python tests/scratch_child.py job.json out.npz

job.json: {"image": .npy path (uint8 board frame), "dots": .npy path (uint8 circle grid), "image16": .npy path (uint16),
"files": [...] (read_image, one by one), "list": [...] (one find_boards_files call, every device route on)}.
out.npz: what each call returned (a missing result as an empty array)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mrgingham_amd  # noqa: E402
from mrgingham_amd import api  # noqa: E402


def _arr(x):
    return np.zeros((0,)) if x is None else np.asarray(x)


def main():
    job = json.load(open(sys.argv[1]))
    image, dots, image16 = np.load(job["image"]), np.load(job["dots"]), np.load(job["image16"])
    out = {}
    for level in (0, 2):
        out[f"find_points_{level}"] = mrgingham_amd.find_points(image, image_pyramid_level=level)
    out["find_points_blobs"] = mrgingham_amd.find_points(dots, image_pyramid_level=0, blobs=True)
    out["find_board"] = _arr(mrgingham_amd.find_board(image, gridn=10))
    out["find_board_level2"] = _arr(mrgingham_amd.find_board(image, image_pyramid_level=2, gridn=10))
    out["chess"] = mrgingham_amd.ChESS_response_5(image)
    for blur in (0, 1):
        out[f"preprocess_{blur}"] = mrgingham_amd.preprocess(image, clahe=True, blur_radius=blur)
        out[f"preprocess16_{blur}"] = api.preprocess16(image16, clahe=True, blur_radius=blur)
    for i, path in enumerate(job["files"]):
        out[f"read_image_{i}"] = _arr(mrgingham_amd.read_image(path))
    boards, levels, found, status, stats = mrgingham_amd.find_boards_files(
        job["list"], batch=4, nthreads=4, entropy="device", png="device", deep="chunks", tiff="device", tiff_deflate="device",
        bmp="device", pnm="device")
    out["files_boards"], out["files_levels"], out["files_found"], out["files_status"] = boards, levels, found, status
    out["files_device_loader"] = np.array(stats["files_device_loader"])
    # the same calls once more: the contexts are the same ones, their scratch as the calls above left it
    out["find_points_0_again"] = mrgingham_amd.find_points(image, image_pyramid_level=0)
    out["find_board_again"] = _arr(mrgingham_amd.find_board(image, gridn=10))
    np.savez(sys.argv[2], **out)


if __name__ == "__main__":
    main()
