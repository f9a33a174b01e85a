"""What the tool's --batch mode (mrgingham_amd_find_boards_files) buys on a list of files:

    python tools/files_bench.py --make DIR                     (needs Pillow: writes nodri.jpg and nodri420.jpg into DIR)
    python tools/files_bench.py --jpeg DIR --parent-tool PATH [--rounds 3] [--jobs 16] [--batch 64]
                                [--out profiles/files_bench.json]

Sets (files made the way tools/jpeg_huff_bench.py makes its own):
  jpeg12mp   256 names of synth.board_frame(4096, 3072) at quality 90 without restart markers, in grey (nodri.jpg) and in
             4:2:0 (nodri420.jpg), alternating;
  pgm640     4096 names over 256 PGM files of 640x480 (synth.board_batch: the files of bench.py's configs.c1_tool), in a
             RAM-backed directory.
Legs, alternating in one process on one box, each a child process under its own time limit, `--rounds` times:
  parent         the tool of the PARENT commit (--parent-tool: built into a scratch directory) with --jobs N: the yardstick;
  per_image      this tool without --batch (the same path: has to stay within the run-to-run spread of `parent`);
  batch_host     --batch B --jobs N;
  batch_device   --batch B --jobs N --jpeg-entropy device.
Every leg is a short run (an eighth of the names) and a long one; images/s is the median over the rounds of
(names long - names short) / (wall long - wall short), i.e. without process start and HIP initialisation; the whole-process
rate of the long run is reported beside it.  The vnlog goes to a file in the RAM-backed directory.  The batch legs also
report the pipeline's stats (MRGINGHAM_AMD_CLI_TIMING=1) and which side waited.  A leg that fails or runs into its time
limit ends the script.  One JSON document."""
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "mrgingham_amd", "bin", "mrgingham-amd-from-image")
LEG_TIMEOUT_S = 300


def opts(args, name, default=None):
    v = [args[i + 1] for i, a in enumerate(args) if a == name]
    return v[0] if v else default


def make(out_dir):
    from PIL import Image
    from mrgingham_amd import synth
    os.makedirs(out_dir, exist_ok=True)
    img = Image.fromarray(synth.board_frame(4096, 3072).numpy())
    img.save(os.path.join(out_dir, "nodri.jpg"), "JPEG", quality=90)
    img.convert("RGB").save(os.path.join(out_dir, "nodri420.jpg"), "JPEG", quality=90, subsampling=2)
    for n in ("nodri.jpg", "nodri420.jpg"):
        print(n, os.path.getsize(os.path.join(out_dir, n)))


def run_leg(cmd, names, sink, batch_stats):
    env = dict(os.environ, MRGINGHAM_AMD_DEVICE="0")
    if batch_stats:
        env["MRGINGHAM_AMD_CLI_TIMING"] = "1"
    t0 = time.perf_counter()
    with open(sink, "wb") as out:
        r = subprocess.run(cmd + names, stdout=out, stderr=subprocess.PIPE, text=True, env=env, timeout=LEG_TIMEOUT_S)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"leg failed ({r.returncode}): {' '.join(cmd)}\n{r.stderr[-2000:]}")
    with open(sink, "rb") as f:
        found = sum(1 for ln in f if not ln.startswith(b"#") and not ln.rstrip().endswith(b"- - -"))
    stats = None
    m = re.search(r"batch: (\d+) chunks; files: (\d+) device loader, (\d+) host-decoded, (\d+) one at a time, (\d+) unreadable; "
                  r"detector waited ([\d.]+) ms for chunks, loader waited ([\d.]+) ms for ring slots", r.stderr)
    if m:
        keys = ("chunks", "files_device_loader", "files_host_decoded", "files_one_image", "files_unreadable",
                "ms_detector_waited_for_chunk", "ms_loader_waited_for_slot")
        stats = dict(zip(keys, (float(x) for x in m.groups())))
    return wall, found, stats


def measure(set_name, names, legs, rounds, scratch):
    short = names[:max(len(names) // 8, 1)]
    sink = os.path.join(scratch, "vnlog.out")
    walls = {k: {"short": [], "long": []} for k in legs}
    last = {}
    for _ in range(rounds):
        for k, cmd in legs.items():                      # alternating
            batch = "--batch" in cmd
            ws, _, _ = run_leg(cmd, short, sink, batch)
            wl, found, stats = run_leg(cmd, names, sink, batch)
            walls[k]["short"].append(ws)
            walls[k]["long"].append(wl)
            last[k] = (found, stats)
            print(f"{set_name} {k}: short {ws:.3f} s, long {wl:.3f} s", file=sys.stderr, flush=True)
    out = {}
    for k in legs:
        steady = [(len(names) - len(short)) / max(wl - ws, 1e-9) for ws, wl in zip(walls[k]["short"], walls[k]["long"])]
        found, stats = last[k]
        out[k] = {"images_per_s": round(statistics.median(steady), 1), "images_per_s_rounds": [round(v, 1) for v in steady],
                  "images_per_s_with_process_start": round(len(names) / statistics.median(walls[k]["long"]), 1),
                  "wall_s_long": [round(v, 3) for v in walls[k]["long"]], "wall_s_short": [round(v, 3) for v in walls[k]["short"]],
                  "corner_records": found}
        if stats:
            out[k]["stats_long_run"] = stats
            d, l = stats["ms_detector_waited_for_chunk"], stats["ms_loader_waited_for_slot"]
            out[k]["who_waited"] = "the detector for the loader" if d > l else "the loader for the detector"
    return {"names": len(names), "names_short_run": len(short), "legs": out}


def main(args):
    if "--make" in args:
        return make(opts(args, "--make"))
    import torch
    from mrgingham_amd import synth
    jpeg_dir, parent = opts(args, "--jpeg"), opts(args, "--parent-tool")
    rounds, jobs, batch = int(opts(args, "--rounds", "3")), opts(args, "--jobs", "16"), opts(args, "--batch", "64")
    out_path = opts(args, "--out", os.path.join(ROOT, "profiles", "files_bench.json"))
    if not jpeg_dir or not parent or not os.access(parent, os.X_OK) or not os.access(CLI, os.X_OK):
        raise SystemExit(__doc__)
    legs = {"parent": [parent, "--jobs", jobs], "per_image": [CLI, "--jobs", jobs],
            "batch_host": [CLI, "--jobs", jobs, "--batch", batch],
            "batch_device": [CLI, "--jobs", jobs, "--batch", batch, "--jpeg-entropy", "device"]}
    scratch = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    doc = {"device": torch.cuda.get_device_name(0), "jobs": int(jobs), "batch": int(batch), "rounds": rounds, "sets": {}}
    try:
        jpegs = []
        for n in ("nodri.jpg", "nodri420.jpg"):        # (into the RAM-backed directory, like the PGM files)
            shutil.copy(os.path.join(jpeg_dir, n), os.path.join(scratch, n))
            jpegs.append(os.path.join(scratch, n))
        doc["sets"]["jpeg12mp"] = measure("jpeg12mp", [jpegs[i % 2] for i in range(256)], legs, rounds, scratch)
        doc["sets"]["jpeg12mp"]["file_bytes"] = {os.path.basename(p): os.path.getsize(p) for p in jpegs}
        frames = synth.board_batch(256, 640, 480, 10, 0, device=torch.device("cuda", 0)).cpu().numpy()
        pgms = []
        for i in range(256):
            pgms.append(os.path.join(scratch, f"f{i:03d}.pgm"))
            with open(pgms[-1], "wb") as f:
                f.write(b"P5\n640 480\n255\n")
                f.write(frames[i].tobytes())
        doc["sets"]["pgm640"] = measure("pgm640", pgms * 16, legs, rounds, scratch)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
