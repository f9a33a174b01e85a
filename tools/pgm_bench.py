"""What the PGM unpack kernel and the 16-bit chunks of the tool's --batch mode (--deep-batch chunks) cost and buy:

    python tools/pgm_bench.py --kernel [--out profiles/pgm_unpack_bench.json]
    python tools/pgm_bench.py --route --parent-tool PATH [--rounds 3] [--jobs 16] [--batch 64] [--out profiles/pgm_route_bench.json]

--kernel: mrgingham_amd_pgm_unpack_batch over 64 payloads of 4096x3072 big-endian pairs (1.6 GB read, 1.6 GB written: no
  cache holds them), two warm-ups, then ten launches between device events: the median in us, bytes/s on the model of 4
  bytes per sample (2 read, 2 written) and that as a fraction of 8 TB/s.  Beside it, in the same process and between the
  same events, hipMemcpyAsync device-to-device of the same bytes (torch's copy_ of a contiguous tensor), and the kernel
  in place.  The output is compared with numpy on the first and the last frame.
--route: tools/files_bench.py's difference method (a short and a long run per leg, images/s from the difference) on 512
  names over two 12 MP 16-bit PGM files in a RAM-backed directory.  Legs, each a child process, alternating, `--rounds`
  times: chunks (--batch B --jobs N --deep-batch chunks), one (--batch B --jobs N --deep-batch one) and parent (the tool
  of the PARENT commit, --parent-tool, with --batch B --jobs N: 16-bit files one at a time).  One JSON document each."""
import json
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK = 8e12


def kernel(out_path):
    import numpy as np
    import torch
    import mrgingham_amd
    B, H, W = 64, 3072, 4096
    det = mrgingham_amd.Detector()
    rng = np.random.default_rng(0)
    one = rng.integers(0, 256, H * W * 2, dtype=np.uint8)
    payload = torch.from_numpy(one).cuda().repeat(B, 1)
    payload[-1] = torch.from_numpy(one[::-1].copy()).cuda()           # (the last frame differs from the first)
    out = torch.empty((B, H, W), dtype=torch.uint16, device="cuda")
    copy_dst = torch.empty_like(payload)

    def timed(fn, n=10, warm=2):
        for _ in range(warm):
            fn()
        us = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        return us
    unpack = timed(lambda: det.pgm_unpack(payload, H, W, 16, out=out))
    got = [out[0].cpu().numpy(), out[B - 1].cpu().numpy()]
    assert np.array_equal(got[0], np.frombuffer(one.tobytes(), ">u2").reshape(H, W)), "frame 0 differs from numpy"
    assert np.array_equal(got[1], np.frombuffer(one[::-1].tobytes(), ">u2").reshape(H, W)), "the last frame differs from numpy"
    copy = timed(lambda: copy_dst.copy_(payload))
    assert torch.equal(copy_dst[-1], payload[-1])
    view = payload.view(torch.uint16).view(B, H, W)
    in_place = timed(lambda: det.pgm_unpack(payload, H, W, 16, out=view))
    assert torch.equal(payload[-1].cpu(), torch.from_numpy(one[::-1].copy())), "twelve swaps in place did not give the bytes back"
    samples = B * H * W

    def row(us):
        med = statistics.median(us)
        rate = 4 * samples / (med * 1e-6)
        return {"us_median": round(med, 1), "us": [round(v, 1) for v in us], "bytes_per_s": round(rate, -9),
                "fraction_of_8TBps": round(rate / HBM_PEAK, 3)}
    doc = {"device": torch.cuda.get_device_name(0), "frames": B, "width": W, "height": H, "bits": 16, "bytes_model": "4 B per sample: 2 read, 2 written",
           "pgm_unpack_kernel_16": row(unpack), "memcpy_device_to_device": row(copy), "pgm_unpack_kernel_16_in_place": row(in_place)}
    doc["kernel_over_copy"] = round(statistics.median(copy) / statistics.median(unpack), 3)
    det.close()
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


def route(args, out_path):
    import numpy as np
    import torch
    import files_bench
    from mrgingham_amd import synth
    parent = files_bench.opts(args, "--parent-tool")
    rounds, jobs, batch = int(files_bench.opts(args, "--rounds", "3")), files_bench.opts(args, "--jobs", "16"), files_bench.opts(args, "--batch", "64")
    if not parent or not os.access(parent, os.X_OK) or not os.access(files_bench.CLI, os.X_OK):
        raise SystemExit(__doc__)
    legs = {"chunks": [files_bench.CLI, "--jobs", jobs, "--batch", batch, "--deep-batch", "chunks"],
            "one": [files_bench.CLI, "--jobs", jobs, "--batch", batch, "--deep-batch", "one"],
            "parent": [parent, "--jobs", jobs, "--batch", batch]}
    scratch = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    doc = {"device": torch.cuda.get_device_name(0), "jobs": int(jobs), "batch": int(batch), "rounds": rounds}
    try:
        files = []
        for i in range(2):
            img = synth.board_frame(4096, 3072, seed=i).numpy().astype(np.uint16) * 257
            files.append(os.path.join(scratch, f"deep{i}.pgm"))
            with open(files[-1], "wb") as f:
                f.write(b"P5\n4096 3072\n65535\n")
                f.write(img.astype(">u2").tobytes())
        doc["pgm16_12mp"] = files_bench.measure("pgm16_12mp", [files[i % 2] for i in range(512)], legs, rounds, scratch)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    lg = doc["pgm16_12mp"]["legs"]
    doc["slowest_chunks_round_over_fastest_parent_round"] = round(min(lg["chunks"]["images_per_s_rounds"]) / max(lg["parent"]["images_per_s_rounds"]), 3)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


def main(args):
    import files_bench
    if "--kernel" in args:
        return kernel(files_bench.opts(args, "--out", os.path.join(ROOT, "profiles", "pgm_unpack_bench.json")))
    if "--route" in args:
        return route(args, files_bench.opts(args, "--out", os.path.join(ROOT, "profiles", "pgm_route_bench.json")))
    raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
