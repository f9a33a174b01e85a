"""What the batch blob detector buys: python tools/blobs_batch_bench.py --parent-lib PATH [--rounds 3] [--cases a,b]
                                                                       [--frames-scale 1.0] [--chunk-frames 0]

Cases: 64 circle-grid frames (synth.dots_frame, seeds 0..63) of 4096x3072, 1920x1080 and 640x480, and 16 frames of
2048x1536 smoothed noise (synth.noise_frame(.., smooth=2)).  Three columns per case, milliseconds per frame:
  P   a loop of find_points(img, 0, blobs=True) over host copies made beforehand, on the PARENT commit's library
      (--parent-lib, loaded in the child through MRGINGHAM_AMD_LIB): what a caller without the batch call has, uploads
      included, the device-to-host copy such a caller would need left out;
  N1  the same loop on this tree's library: the one-frame entry is the batch of one;
  NB  Detector.blobs on the device batch, this tree's library; with the device milliseconds of the chunks' kernels
      (hipEvents, from a call of its own with kernel timing on), the host milliseconds of filters and grouping, chunks,
      nodes, contours and points downloaded.
`--rounds` rounds, the three columns alternating within a round, one child process at a time (it takes all cases),
warm-up calls first.  One JSON line per case, round and column as it is measured, then one summary line per case: median
and min / max per column and the two conditions -- NB below P in every round; median(N1) - median(P) within P's own
spread (max - min).  Every column also reports a checksum of its keypoints: they must agree."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {                       # name: (kind, W, H, frames, passes of the timed loop)
    "dots_4096x3072": ("dots", 4096, 3072, 64, 1),
    "dots_1920x1080": ("dots", 1920, 1080, 64, 2),
    "dots_640x480": ("dots", 640, 480, 64, 4),
    "noise_2048x1536": ("noise", 2048, 1536, 16, 1),
}


def child(column, cases, scale, chunk_frames):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import mrgingham_amd
    from mrgingham_amd import synth
    for name in cases:
        kind, W, H, B, passes = CASES[name]
        B = max(1, int(B * scale))
        if kind == "dots":
            frames = torch.stack([synth.dots_frame(W, H, 10, s, device="cuda") for s in range(B)])
        else:
            frames = torch.stack([synth.noise_frame(W, H, s, smooth=2, device="cuda") for s in range(B)])
        torch.cuda.synchronize()
        line = {"case": name, "column": column, "frames": B, "width": W, "height": H}
        if column in ("P", "N1"):
            host = [frames[f].cpu().numpy() for f in range(B)]
            del frames
            for f in range(min(B, 3)):
                mrgingham_amd.find_points(host[f], 0, blobs=True)
            t0 = time.perf_counter()
            for _ in range(passes):
                got = [mrgingham_amd.find_points(img, 0, blobs=True) for img in host]
            dt = time.perf_counter() - t0
            got = [np.round(g * 1000).astype(np.int64) for g in got]
        else:
            det = mrgingham_amd.Detector(0)
            det.set_option("blob_chunk_frames", chunk_frames)
            det.blobs(frames)
            det.blobs(frames)
            t0 = time.perf_counter()
            for _ in range(passes):
                got = det.blobs(frames)
            dt = time.perf_counter() - t0
            det.set_kernel_timing(1)
            det.blobs_stats()
            det.blobs(frames)
            st = det.blobs_stats()
            det.set_kernel_timing(0)
            line.update({"device_ms_per_frame": round(st["device_ms"] / B, 4), "host_ms_per_frame": round(st["host_ms"] / B, 4),
                         "chunks": int(st["chunks"]), "nodes": int(st["nodes"]), "contours": int(st["contours"]),
                         "points": int(st["points"]), "chunk_frames_option": chunk_frames})
            det.close()
        line["ms_per_frame"] = round(dt / (passes * B) * 1e3, 4)
        line["keypoints"] = int(sum(len(g) for g in got))
        line["checksum"] = int(sum(int(g.astype(np.int64).sum()) * (f + 1) for f, g in enumerate(got)))
        print(json.dumps(line), flush=True)


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return args[args.index(name) + 1] if name in args else default
    if args and args[0] == "child":
        return child(args[1], args[2].split(","), float(args[3]), int(args[4]))
    parent_lib = opt("--parent-lib", None)
    if not parent_lib or not os.path.exists(parent_lib):
        sys.exit("blobs_batch_bench.py: --parent-lib PATH (the parent commit's libmrgingham_amd.so) is required")
    rounds = int(opt("--rounds", "3"))
    cases = opt("--cases", ",".join(CASES)).split(",")
    scale, chunk_frames = opt("--frames-scale", "1.0"), opt("--chunk-frames", "0")
    acc = {c: {"P": [], "N1": [], "NB": []} for c in cases}
    sums = {c: set() for c in cases}
    last_nb = {}
    for rnd in range(rounds):
        for column in ("P", "N1", "NB"):
            env = dict(os.environ)
            env.pop("MRGINGHAM_AMD_LIB", None)
            if column == "P":
                env["MRGINGHAM_AMD_LIB"] = os.path.abspath(parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "child", column, ",".join(cases), scale, chunk_frames],
                                 env=env, stdout=subprocess.PIPE, text=True, timeout=900)
            if out.returncode != 0:
                sys.exit(f"blobs_batch_bench.py: the child of column {column} failed ({out.returncode})")
            for ln in out.stdout.splitlines():
                if not ln.startswith("{"):
                    continue
                d = json.loads(ln)
                d["round"] = rnd
                print(json.dumps(d), flush=True)
                acc[d["case"]][column].append(d["ms_per_frame"])
                sums[d["case"]].add((d["keypoints"], d["checksum"]))
                if column == "NB":
                    last_nb[d["case"]] = d
    for c in cases:
        a = acc[c]
        med = {k: statistics.median(v) for k, v in a.items()}
        spread_p = max(a["P"]) - min(a["P"])
        print(json.dumps({"case": c, "summary": True, "rounds": rounds,
                          **{f"{k}_ms_per_frame": {"median": round(med[k], 4), "min": min(v), "max": max(v)} for k, v in a.items()},
                          "NB_below_P_every_round": all(nb < p for nb, p in zip(a["NB"], a["P"])),
                          "N1_minus_P_median": round(med["N1"] - med["P"], 4), "P_spread": round(spread_p, 4),
                          "N1_within_P_spread": med["N1"] - med["P"] <= spread_p,
                          "results_agree": len(sums[c]) == 1,
                          "NB_device_ms_per_frame": last_nb[c]["device_ms_per_frame"],
                          "NB_host_ms_per_frame": last_nb[c]["host_ms_per_frame"], "NB_chunks": last_nb[c]["chunks"]}), flush=True)


if __name__ == "__main__":
    main()
