"""What the Netpbm unpack kernel and the Netpbm batch loader cost:

    python tools/pnm_bench.py --kernel [--out profiles/pnm_unpack_bench.json]
    python tools/pnm_bench.py --loader [--rounds 3] [--jobs 16] [--files 64] [--out profiles/pnm_loader_bench.json]

--kernel: mrgingham_amd_pnm_unpack_batch over 64 rasters of 4096x3072 as P4 and as P7 of depth 3 at 8 and at 16 bits, depth 4
  at 8 bits and depth 1 at 8 bits: two warm-ups, then ten launches between device events; the median in us with min and max, bytes/s
  on the model of channels * bits / 8 + bits_out / 8 bytes per pixel (the raster read, the grey sample written) and that as
  a fraction of 8 TB/s.  The yardsticks run in the same process, between the same events, alternating with the launches
  inside every round: hipMemcpyAsync device-to-device of the same payload bytes (torch's copy_ of a contiguous tensor) and,
  for depth 1 at 8 bits, mrgingham_amd_pgm_unpack_batch over the same bytes.  Neither is code under test.  The output is
  compared with the host decoder's arithmetic (numpy) on rows of the first and the last frame.
--loader: mrgingham_amd_read_pnms_batch on `--files` names over two 12 MP P7 RGB files in a RAM-backed directory, option
  "pnm_unpack" 1 against 0 (every file decoded by the host threads inside the same call), `--rounds` alternating rounds
  after a warm-up round, wall time of the call: files/s per round.  One JSON document each."""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK = 8e12
GREY = (4899, 9617, 1868)  # R, G, B (csrc/png_filter.h)


def kernel(out_path):
    import numpy as np
    import torch
    import mrgingham_amd
    B, H, W = 64, 3072, 4096
    det = mrgingham_amd.Detector()
    rng = np.random.default_rng(0)
    doc = {"device": torch.cuda.get_device_name(0), "frames": B, "width": W, "height": H,
           "bytes_model": "channels * bits / 8 + bits_out / 8 B per pixel: the raster read, one grey sample written"}

    def event_us(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    def alternating(fns, n=10, warm=2):
        """the legs take turns inside every round -> {name: [us] * n}"""
        for _ in range(warm):
            for fn in fns.values():
                fn()
        us = {k: [] for k in fns}
        for _ in range(n):
            for k, fn in fns.items():
                us[k].append(event_us(fn))
        return us

    def row(us, bytes_moved):
        med = statistics.median(us)
        rate = bytes_moved / (med * 1e-6)
        return {"us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1), "us": [round(v, 1) for v in us],
                "bytes_per_s": round(rate, -9), "fraction_of_8TBps": round(rate / HBM_PEAK, 3)}

    def host_rows(raw, bits, ch):
        """rows of a raster (uint8 [rows, row_bytes]) -> grey [rows, W], the host decoder's arithmetic in numpy"""
        if bits == 1:
            return np.where(np.unpackbits(raw, axis=1)[:, :W] != 0, 0, 255).astype(np.uint8)
        px = (raw if bits == 8 else raw.view(">u2")).reshape(raw.shape[0], W, ch).astype(np.int64)
        g = px[..., 0] if ch <= 2 else (px[..., 0] * GREY[0] + px[..., 1] * GREY[1] + px[..., 2] * GREY[2] + 8192) >> 14
        return g.astype(np.uint16 if bits == 16 else np.uint8)

    px = H * W
    for name, bits, ch in (("p4", 1, 1), ("p7_depth3_8bit", 8, 3), ("p7_depth3_16bit", 16, 3), ("p7_depth4_8bit", 8, 4), ("p7_depth1_8bit", 8, 1)):
        rowb = (W + 7) // 8 if bits == 1 else W * ch * bits // 8
        es = 2 if bits == 16 else 1
        one = rng.integers(0, 256, H * rowb, dtype=np.uint8)
        payload = torch.from_numpy(one).cuda().repeat(B, 1)
        payload[-1] = torch.from_numpy(one[::-1].copy()).cuda()           # (the last frame differs from the first)
        out = torch.empty((B, H, W), dtype=torch.uint16 if es == 2 else torch.uint8, device="cuda")
        copy_dst = torch.empty_like(payload)
        legs = {"pnm_unpack": lambda: det.pnm_unpack(payload, H, W, bits, ch, out=out)}
        if bits == 8 and ch == 1:
            pgm_out = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
            legs["pgm_unpack_8"] = lambda: det.pgm_unpack(payload, H, W, 8, out=pgm_out)
        legs["memcpy_device_to_device"] = lambda: copy_dst.copy_(payload)
        us = alternating(legs)
        rows = [0, 1, H // 2, H - 1]
        for f, src in ((0, one), (B - 1, one[::-1])):
            raw = np.ascontiguousarray(src.reshape(H, rowb)[rows])
            got = out[f].cpu().numpy()[rows]
            assert np.array_equal(got, host_rows(raw, bits, ch)), f"{name}: frame {f} differs from the host arithmetic"
        r = {"bits": bits, "channels": ch, "row_bytes": rowb, "pnm_unpack": row(us["pnm_unpack"], B * (H * rowb + px * es)),
             "memcpy_device_to_device": row(us["memcpy_device_to_device"], 2 * B * H * rowb)}
        r["pnm_over_memcpy"] = round(statistics.median(us["pnm_unpack"]) / statistics.median(us["memcpy_device_to_device"]), 3)
        if "pgm_unpack_8" in us:
            r["pgm_unpack_8"] = row(us["pgm_unpack_8"], 2 * B * px)
            r["pnm_over_pgm_unpack"] = round(statistics.median(us["pnm_unpack"]) / statistics.median(us["pgm_unpack_8"]), 3)
            del pgm_out
        doc[name] = r
        del payload, copy_dst, out
        torch.cuda.empty_cache()
    det.close()
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


def loader(args, out_path):
    import numpy as np
    import torch
    import files_bench
    import mrgingham_amd
    from mrgingham_amd import synth
    from tests import pnm_cases
    rounds, jobs, nfiles = (int(files_bench.opts(args, k, d)) for k, d in (("--rounds", "3"), ("--jobs", "16"), ("--files", "64")))
    scratch = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    doc = {"device": torch.cuda.get_device_name(0), "jobs": jobs, "files": nfiles, "rounds": rounds, "width": 4096, "height": 3072,
           "format": "P7, depth 3, maxval 255"}
    det = mrgingham_amd.Detector()
    try:
        files = []
        for i in range(2):
            img = synth.board_frame(4096, 3072, seed=i).numpy()
            files.append(os.path.join(scratch, f"colour{i}.pam"))
            with open(files[-1], "wb") as f:
                f.write(pnm_cases.write(np.stack([img, img // 2, 255 - img], axis=-1), 7, 8))
        names = [files[i % 2] for i in range(nfiles)]
        want = [mrgingham_amd.read_image(p) for p in files]
        legs = {"device": [], "host": []}
        for r in range(rounds + 1):                                   # (round 0 warms the staging and the page cache up)
            for leg, unpack in (("device", 1), ("host", 0)):
                det.set_option("pnm_unpack", unpack)
                t0 = time.perf_counter()
                frames, status = det.read_pnms(names, nthreads=jobs)
                dt = time.perf_counter() - t0
                assert not status.any()
                assert np.array_equal(frames[1].cpu().numpy(), want[1]) and np.array_equal(frames[nfiles - 2].cpu().numpy(), want[nfiles % 2])
                if r:
                    legs[leg].append(round(nfiles / dt, 1))
                del frames
        doc["files_per_s_rounds"] = legs
        doc["slowest_device_round_over_fastest_host_round"] = round(min(legs["device"]) / max(legs["host"]), 3)
    finally:
        det.close()
        shutil.rmtree(scratch, ignore_errors=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


def main(args):
    import files_bench
    if "--kernel" in args:
        return kernel(files_bench.opts(args, "--out", os.path.join(ROOT, "profiles", "pnm_unpack_bench.json")))
    if "--loader" in args:
        return loader(args, files_bench.opts(args, "--out", os.path.join(ROOT, "profiles", "pnm_loader_bench.json")))
    raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
