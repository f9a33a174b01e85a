"""What reading JPEG through the device costs: python tools/jpeg_bench.py [--file board.jpg] [--frames 64] [--launches 30]
                                                                        [--out profiles/jpeg_bench.json]

One 12 MP baseline JPEG, read `--frames` times under different paths.  Where Pillow is importable the file is
synth.board_frame(4096, 3072) encoded at quality 90; otherwise give it with --file.  Three legs, in one process on one box:
  idct     mrgingham_amd_jpeg_idct_batch alone on a device batch of the file's coefficients: microseconds per launch
           (hipEvents around each launch, median / min / max of --launches launches after three warm-up ones), the bytes
           it moves per pixel (2 read + 1 written) as a fraction of the 8 TB/s HBM peak;
  loader   Detector.read_jpegs over the files at 1, 4 and 16 host threads: frames per second (wall clock around the
           synchronous call, best and median of three calls after a warm-up one);
  host     the path without the device transform at 16 threads: read_image (entropy decode + inverse DCT on the host) into
           one page-locked batch, then ONE upload of 1 B/px -- frames per second the same way.
The engine clock reported beside them is the one the context's probe measures on a level-0 response launch over the same
frames right after the legs (Detector.sclk_mhz): the transform kernel itself carries no probe.  One JSON document."""
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12


def opt(args, name, default):
    return args[args.index(name) + 1] if name in args else default


def the_file(args, tmp):
    given = opt(args, "--file", None)
    if given:
        return given
    try:
        from PIL import Image
    except ImportError:
        sys.exit("jpeg_bench.py: Pillow is not importable here: give the 12 MP JPEG with --file")
    from mrgingham_amd import synth
    path = os.path.join(tmp, "board_4096x3072_q90.jpg")
    Image.fromarray(synth.board_frame(4096, 3072).numpy()).save(path, "JPEG", quality=90)
    return path


def rate(fn, frames, calls=3):
    fn()
    dts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        dts.append(time.perf_counter() - t0)
    return {"frames_per_s_best": round(frames / min(dts), 1), "frames_per_s_median": round(frames / statistics.median(dts), 1)}


def main():
    args = sys.argv[1:]
    import numpy as np
    import torch
    import mrgingham_amd
    from mrgingham_amd import api
    B, launches = int(opt(args, "--frames", "64")), max(20, int(opt(args, "--launches", "30")))
    out_path = opt(args, "--out", os.path.join(ROOT, "profiles", "jpeg_bench.json"))
    with tempfile.TemporaryDirectory() as tmp:
        path = the_file(args, tmp)
        data = open(path, "rb").read()
        coef, quant, (H, W) = mrgingham_amd.jpeg_coefficients(data)
        want = mrgingham_amd.read_image(path)
        det = mrgingham_amd.Detector(0)
        doc = {"file_bytes": len(data), "width": W, "height": H, "frames": B, "device": torch.cuda.get_device_name(0)}

        # leg 1: the kernel alone
        d_coef = torch.from_numpy(coef).to(det.device)[None].expand(B, -1, -1, -1).contiguous()
        d_quant = torch.from_numpy(quant.view(np.int16)).to(det.device)[None].expand(B, -1).contiguous()
        out = torch.empty((B, H, W), dtype=torch.uint8, device=det.device)
        for _ in range(3):
            det.jpeg_idct(d_coef, d_quant, H, W, out=out)
        torch.cuda.synchronize()
        us = []
        for _ in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            det.jpeg_idct(d_coef, d_quant, H, W, out=out)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        med = statistics.median(us)
        doc["idct"] = {"launches": launches, "us_per_batch_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                       "model_B_per_px": 3, "hbm_fraction": round(3.0 * B * W * H / (med * 1e-6) / HBM_PEAK, 3),
                       "equals_host_decoder": bool((out[0].cpu().numpy() == want).all() and (out[B - 1].cpu().numpy() == want).all())}
        del d_coef

        # leg 2: the loader
        files = [path] * B
        doc["loader"] = {}
        for n in (1, 4, 16):
            doc["loader"][f"threads_{n}"] = rate(lambda: det.read_jpegs(files, nthreads=n), B, calls=1 if n == 1 else 3)
        frames, status = det.read_jpegs(files, nthreads=16)
        doc["loader"]["equals_host_decoder"] = bool((status == 0).all() and (frames[B // 2].cpu().numpy() == want).all())
        doc["loader"]["scratch_bytes"] = det.scratch_bytes()

        # leg 3: the host path at 16 threads
        pinned = api.PinnedArray((B, H, W))
        pool = ThreadPoolExecutor(16)

        L, name = det.L, os.fsencode(path)

        def host_path():
            def one(f):                      # (one decode per file, straight into the page-locked batch)
                assert L.mrgingham_amd_read_image(name, 0, pinned.array[f].ctypes.data, H * W, None, None, None) == 0
            list(pool.map(one, range(B)))
            out.copy_(torch.from_numpy(pinned.array), non_blocking=True)
            torch.cuda.synchronize()
        doc["host_16_threads"] = rate(host_path, B)
        doc["host_16_threads"]["equals_host_decoder"] = bool((out[B // 2].cpu().numpy() == want).all())
        pool.shutdown()

        # the clock of the box, under a kernel that carries the probe
        det.set_kernel_timing(2)
        det.sclk_mhz()
        det.chess_response(out)
        doc["sclk_mhz_under_chess_level0"] = round(det.sclk_mhz(), 1)
        det.set_kernel_timing(0)
        a, b = doc["loader"]["threads_16"]["frames_per_s_median"], doc["host_16_threads"]["frames_per_s_median"]
        doc["device_path_over_host_path_at_16_threads"] = round(a / b, 3)
        det.close()
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
