"""What the PNG device route (png_recon.hip, mrgingham_amd_read_pngs_batch, find_boards_files(png="device")) costs and buys:

    python tools/png_bench.py --parent-tool PATH [--rounds 3] [--jobs 16] [--batch 64] [--frames 64] [--files 128]
                              [--out profiles/png_bench.json]

1. The kernel alone: `--frames` frames of 4096x3072 (synth.board_frame plus noise), grey 8 bit and RGB 8 bit, once with
   Paeth on every row and once with the rotating filter types, reconstructed by Detector.png_reconstruct between two
   device events (two warm-up launches, the median of ten); the output is checked against the source array.  Per case:
   us per launch, the bytes the algorithm moves per launch -- one read of (rowbytes + 1) * height and one write of
   width * height per frame --, and what fraction of the HBM peak (8.0 TB/s) that is: a description of a dependency
   chain, not a target.  Beside it the wall time `--jobs` host threads need to inflate the same `--frames` files (zlib
   level 6) with mrgingham_amd_png_scanlines, in the same process: the kernel hides behind the host while its time stays
   below that.
2. The loader: `--files` names over two 12 MP grey PNG files (Paeth on four rows of five, the other types taking turns on
   the fifth; zlib level 6) in a RAM-backed directory, through the tool with --batch: the tool of the PARENT commit
   (--parent-tool: the yardstick), this tool with --png-reconstruct host and with --png-reconstruct device, each leg a
   child process, alternating, `--rounds` times, by the difference method of tools/files_bench.py (a short run and a long
   one; images/s without process start), with the pipeline's two wait clocks.
One JSON document."""
import concurrent.futures
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import files_bench  # noqa: E402
from tests import png_cases  # noqa: E402

HBM_PEAK = 8.0e12
W, H = 4096, 3072
PAETH_HEAVY = [4, 4, 4, 4, 1, 4, 4, 4, 4, 2, 4, 4, 4, 4, 3, 4, 4, 4, 4, 0]


_frames = {}


def board(seed, color_type):
    from mrgingham_amd import synth
    rng = np.random.default_rng(seed)
    if seed not in _frames:
        _frames[seed] = synth.board_frame(W, H, 10, seed=seed).numpy().astype(np.int32)
    grey = _frames[seed]
    if color_type == 0:
        return np.clip(grey + rng.integers(-3, 4, grey.shape), 0, 255).astype(np.uint8)
    return np.stack([np.clip(grey + rng.integers(-3, 4, grey.shape) + 2 * k, 0, 255) for k in range(3)], axis=-1).astype(np.uint8)


def inflate_wall_ms(data, nfiles, jobs):
    """Wall ms for `jobs` threads to run mrgingham_amd_png_scanlines over nfiles copies of the file (ctypes drops the GIL)."""
    from mrgingham_amd import _lib, api
    L = _lib.lib()
    h, w, bits, ct = api.png_scanlines_size(data)
    need = (w * png_cases.bpp_of(ct, bits) + 1) * h
    bufs = [np.empty(need, np.uint8) for _ in range(jobs)]

    def work(k):
        ints = [ctypes.c_int() for _ in range(4)]
        for _ in range(k, nfiles, jobs):
            assert L.mrgingham_amd_png_scanlines(data, len(data), bufs[k].ctypes.data, need, *[ctypes.byref(v) for v in ints]) == 0
    walls = []
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        for _ in range(3):
            t0 = time.perf_counter()
            list(pool.map(work, range(jobs)))
            walls.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(walls), walls


def kernel_cases(frames, jobs):
    import torch
    import mrgingham_amd
    det = mrgingham_amd.Detector(0)
    out = {}
    for name, ct in (("grey8", 0), ("rgb8", 2)):
        img = board(1, ct)
        want = torch.from_numpy(png_cases.grey_of(img, ct)).cuda()
        for fname, filters in (("paeth", 4), ("rotate", "rotate")):
            data, scan = png_cases.encode(img, ct, 8, filters=filters, level=6)
            d_scan = torch.from_numpy(scan).cuda().unsqueeze(0).repeat(frames, 1, 1).contiguous()
            d_out = torch.empty((frames, H, W), dtype=torch.uint8, device="cuda")
            for _ in range(2):
                det.png_reconstruct(d_scan, H, W, 8, ct, out=d_out)
            torch.cuda.synchronize()
            assert torch.equal(d_out[0], want) and torch.equal(d_out[frames - 1], want), "the kernel's output differs from the source"
            us = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                det.png_reconstruct(d_scan, H, W, 8, ct, out=d_out)
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            moved = frames * (scan.size + W * H)
            t = statistics.median(us)
            host_ms, host_walls = inflate_wall_ms(data, frames, jobs)
            out[f"{name}_{fname}"] = {
                "us_per_launch": round(t, 1), "us_per_launch_min_max": [round(min(us), 1), round(max(us), 1)],
                "bytes_per_launch": moved, "bytes_per_s": round(moved / (t * 1e-6)), "fraction_of_hbm_peak": round(moved / (t * 1e-6) / HBM_PEAK, 4),
                "file_bytes": len(data), "host_inflate_wall_ms_per_chunk": round(host_ms, 1),
                "host_inflate_wall_ms_rounds": [round(v, 1) for v in host_walls],
                "kernel_hides_behind_host_inflate": bool(t * 1e-3 < host_ms)}
            print(f"kernel {name}_{fname}: {t:.0f} us per {frames} frames, host inflate {host_ms:.0f} ms", file=sys.stderr, flush=True)
            del d_scan, d_out
    det.close()
    return out


def main(args):
    import torch
    import mrgingham_amd
    parent = files_bench.opts(args, "--parent-tool")
    rounds, jobs, batch = int(files_bench.opts(args, "--rounds", "3")), files_bench.opts(args, "--jobs", "16"), files_bench.opts(args, "--batch", "64")
    frames, nfiles = int(files_bench.opts(args, "--frames", "64")), int(files_bench.opts(args, "--files", "128"))
    out_path = files_bench.opts(args, "--out", os.path.join(ROOT, "profiles", "png_bench.json"))
    if not parent or not os.access(parent, os.X_OK) or not os.access(files_bench.CLI, os.X_OK):
        raise SystemExit(__doc__)
    doc = {"device": torch.cuda.get_device_name(0), "jobs": int(jobs), "batch": int(batch), "rounds": rounds, "frames_per_launch": frames,
           "frame": [W, H], "hbm_peak_bytes_per_s": HBM_PEAK, "geometry_rows_segment": list(mrgingham_amd.png_reconstruct_geometry())}
    doc["kernel"] = kernel_cases(frames, int(jobs))
    scratch = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        pngs = []
        for seed in (1, 2):
            pngs.append(os.path.join(scratch, f"board{seed}.png"))
            png_cases.write(pngs[-1], board(seed, 0), 0, 8, filters=PAETH_HEAVY, level=6)
        legs = {"parent_batch": [parent, "--jobs", jobs, "--batch", batch],
                "batch_png_host": [files_bench.CLI, "--jobs", jobs, "--batch", batch, "--png-reconstruct", "host"],
                "batch_png_device": [files_bench.CLI, "--jobs", jobs, "--batch", batch, "--png-reconstruct", "device"]}
        res = files_bench.measure("png12mp", [pngs[i % 2] for i in range(nfiles)], legs, rounds, scratch)
        res["file_bytes"] = {os.path.basename(p): os.path.getsize(p) for p in pngs}
        host, device = res["legs"]["batch_png_host"]["images_per_s_rounds"], res["legs"]["batch_png_device"]["images_per_s_rounds"]
        res["host_route_spread_images_per_s"] = round(max(host) - min(host), 1)
        res["device_minus_host_images_per_s"] = round(statistics.median(device) - statistics.median(host), 1)
        res["device_over_host"] = round(statistics.median(device) / statistics.median(host), 2)
        res["device_faster_by_more_than_the_host_spread"] = bool(min(device) > max(host))
        doc["loader"] = res
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
