"""The device grid finder against the host route of find_boards, on one device, in one process, alternating option
"find_boards_grid" 0 and 1 over three rounds (DESIGN.md sections 4.25 and 9):
  * find_boards frames/s, three batches in flight, 64 frames of 4096x3072, 1920x1080 and 640x480;
  * the host's grid-finder CPU per batch (find_boards_stats: the threads' phase clocks, summed) and the wall time the
    caller waits for them;
  * the kernel alone: microseconds per launch (hipEvents) for 192 lists of 100 and of 196 candidates.
usage: python tools/find_grids_bench.py [out.json] [--quick] [--batches N]"""
import sys, os, time, json; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import mrgingham_amd
from mrgingham_amd import synth


def boards_rate(det, batches, grid, n, depth=3):
    det.set_option("find_boards_grid", grid)
    jobs = []
    def step(i):
        jobs.append(det.find_boards_submit(batches[i % len(batches)], gridn=10))
        if len(jobs) >= depth:
            det.find_boards_collect(jobs.pop(0))
    def drain():
        while jobs:
            det.find_boards_collect(jobs.pop(0))
    for i in range(6):
        step(i)
    drain()
    det.find_boards_stats()
    det.find_grids_stats()
    t0 = time.perf_counter()
    for i in range(n):
        step(i)
    drain()
    dt = (time.perf_counter() - t0) / n
    fb, fg = det.find_boards_stats(), det.find_grids_stats()
    B = batches[0].shape[0]
    cpu_us = fb["grid_us_graph"] + fb["grid_us_adjacency"] + fb["grid_us_sequences"] + fb["grid_us_cycles_rows"]
    return {"grid": grid, "ms_per_batch": dt * 1e3, "frames_per_s": B / dt, "host_grid_cpu_ms_per_batch": cpu_us / 1e3 / n,
            "host_grid_calls_per_frame": fb["grid_calls"] / n / B, "ms_grid_finder_joined_per_batch": fb["ms_grid_finder_joined"] / n,
            "device_lists_per_batch": fg["lists"] / n, "device_declined_per_batch": (fg["lists"] - fg["found"] - fg["none"]) / n,
            "host_fallbacks_per_batch": fg["host_fallbacks"] / n}


def kernel_us(det, ncand, nlists=192, reps=50):
    """nlists lists of the corners of a gridn x gridn board under a mild homography; gridn 10 -> 100, 14 -> 196 candidates"""
    gridn = {100: 10, 196: 14}[ncand]
    rng = np.random.RandomState(ncand)
    xy = np.zeros((nlists, 512, 2), np.int32)
    for l in range(nlists):
        a = np.deg2rad(rng.uniform(-30, 30))
        ii, jj = np.meshgrid(np.arange(gridn), np.arange(gridn), indexing="ij")
        p = np.stack([jj.ravel() * 60.0, ii.ravel() * 60.0], 1) @ np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
        p = p / (1 + 2e-4 * p[:, :1]) + 2000 + rng.normal(0, 0.3, p.shape)
        xy[l, :ncand] = np.round(p[rng.permutation(ncand)] * 1000)
    txy = torch.from_numpy(xy).cuda()
    counts = torch.full((nlists,), ncand, dtype=torch.int32, device="cuda")
    out = (torch.empty((nlists, gridn * gridn), dtype=torch.int32, device="cuda"), torch.empty((nlists,), dtype=torch.int32, device="cuda"))
    det.find_grids(txy, counts, gridn, out=out)
    assert (out[1] == 1).all(), out[1].cpu().tolist()
    times = []
    for _ in range(reps):
        det.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        det.after_stream()
        det.find_grids(txy, counts, gridn, out=out, sync=False)
        det.stream_wait()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    return {"candidates": ncand, "lists": nlists, "us_min": times[0], "us_median": times[len(times) // 2], "us_max": times[-1]}


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", nargs="?", help="write the results here as JSON")
    ap.add_argument("--quick", action="store_true", help="4096x3072 only, 40 batches per round")
    ap.add_argument("--batches", type=int, default=0, help="batches timed per round (default 150; 40 with --quick)")
    opt = ap.parse_args()
    quick, n, args = opt.quick, opt.batches or (40 if opt.quick else 150), [opt.out] if opt.out else []
    det = mrgingham_amd.Detector(0)
    res = {"kernel": [kernel_us(det, c) for c in (100, 196)], "find_boards": []}
    for k in res["kernel"]:
        print(f"find_grids kernel, {k['lists']} lists of {k['candidates']}: {k['us_median']:.0f} us per launch (min {k['us_min']:.0f}, max {k['us_max']:.0f}; "
              "hipEvents around the call's stream waits and its launch)", flush=True)
    for (W, H) in [(4096, 3072)] if quick else [(4096, 3072), (1920, 1080), (640, 480)]:
        batches = [synth.board_batch(64, W, H, 10, 100 * i, device="cuda") for i in range(2)]
        rounds = [boards_rate(det, batches, grid, n) for _ in range(3) for grid in (0, 1)]
        for grid in (0, 1):
            rs = [r for r in rounds if r["grid"] == grid]
            fps = sorted(r["frames_per_s"] for r in rs)
            cpu = sorted(r["host_grid_cpu_ms_per_batch"] for r in rs)
            print(f"{W}x{H} x64 find_boards_grid {grid}: {fps[1]:8.0f} frames/s (min {fps[0]:.0f}, max {fps[2]:.0f}); host grid finder "
                  f"{cpu[1]:.2f} ms CPU per batch (min {cpu[0]:.2f}, max {cpu[2]:.2f}), {rs[0]['host_grid_calls_per_frame']:.2f} calls per frame; "
                  f"device lists {rs[0]['device_lists_per_batch']:.0f}, declined {rs[0]['device_declined_per_batch']:.2f} per batch", flush=True)
        res["find_boards"].append({"W": W, "H": H, "B": 64, "rounds": rounds})
        del batches
    det.close()
    if args:
        json.dump(res, open(args[0], "w"), indent=1)
