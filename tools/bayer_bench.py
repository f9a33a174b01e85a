"""What taking Bayer mosaics to grey on the device costs, and what it saves a host-fed caller:

    python tools/bayer_bench.py --kernel   [--out profiles/bayer_grey_bench.json]
    python tools/bayer_bench.py --host-fed [--out profiles/bayer_grey_bench.json]

Both write into the same JSON document (each its own key; the other's stays).

--kernel: mrgingham_amd_bayer_grey_batch over 64 frames of 4096x3072, 8 bit RGGB and GRBG (a red-first and a green-first
  row) and 16 bit RGGB: two warm-ups, then ten launches between device events; the median in us with min and max,
  bytes/s on the model of 2 B per pixel at 8 bit and 4 at 16 (every sample read once, every grey written once) and that
  as a fraction of 8 TB/s.  The yardsticks run in the same process, between the same events, alternating with the
  launches inside every round: a device-to-device copy that moves the same byte count and, for the 8-bit cases,
  Detector.box_blur(radius=1) on the same frames -- box_blur3_kernel, the project's existing 3x3 stencil on the same byte
  model.  Neither is code under test.  Rows of the first and the last frame are compared with numpy
  (tests/bayer_cases.py).
--host-fed: 64 8-bit mosaics from page-locked memory to grey frames on the device, two legs, each fenced, three
  alternating rounds after a warm-up round, wall time:
    1. upload the mosaics, Detector.bayer_grey;
    2. 16 host threads run mrgingham_amd_bayer_grey_image on the same frames, then their output is uploaded: the route a
       caller has without the device call.
  The link bytes are equal.  The condition: the slowest round of leg 1 is faster than the fastest round of leg 2."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK = 8e12
B, H, W = 64, 3072, 4096


def _merge(out_path, key, value):
    doc = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            doc = json.load(f)
    doc[key] = value
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({key: value}, indent=1))


def _mosaics(np, rng, dtype):
    """[B,H,W] on the host: one random frame over and over, the last frame the first one upside down"""
    one = rng.integers(0, int(np.iinfo(dtype).max) + 1, (H, W), dtype=dtype)
    return one, np.ascontiguousarray(one[::-1])


def kernel(out_path):
    import numpy as np
    import torch
    import mrgingham_amd
    from tests import bayer_cases as bc
    bc.check_known()
    det = mrgingham_amd.Detector()
    rng = np.random.default_rng(0)
    doc = {"device": torch.cuda.get_device_name(0), "frames": B, "width": W, "height": H,
           "bytes_model": "2 B per pixel at 8 bit, 4 at 16: every sample read once, every grey written once",
           "kernel_geometry": dict(zip(("lanes_per_workgroup", "rows_per_slab", "max_workgroups_per_cu"), mrgingham_amd.bayer_grey_geometry()))}

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

    def rows_equal(got, src, pat):
        """the first, the middle and the last rows of a frame against numpy on slices that begin at even rows"""
        for a, b, keep in ((0, 4, slice(0, 3)), (H // 2 - 2, H // 2 + 2, slice(1, 3)), (H - 4, H, slice(1, 4))):
            if not np.array_equal(got[a:b][keep], bc.grey(src[a:b], pat)[keep]):
                return False
        return True

    for name, pat, dtype in (("rggb_8", "rggb", np.uint8), ("grbg_8", "grbg", np.uint8), ("rggb_16", "rggb", np.uint16)):
        es = np.dtype(dtype).itemsize
        first, last = _mosaics(np, rng, dtype)
        # (assembled as int16 where the samples are uint16: torch copies those everywhere)
        raw = torch.from_numpy(first.view(np.int16) if es == 2 else first).cuda().repeat(B, 1, 1)
        raw[-1] = torch.from_numpy(last.view(np.int16) if es == 2 else last).cuda()
        frames = raw.view(torch.uint16) if es == 2 else raw
        out = torch.empty((B, H, W), dtype=frames.dtype, device="cuda")
        moved = 2 * es * B * H * W
        copy_src = torch.empty((moved // 2,), dtype=torch.uint8, device="cuda")
        copy_dst = torch.empty_like(copy_src)
        legs = {"bayer_grey": lambda: det.bayer_grey(frames, pat, out=out),
                "memcpy_device_to_device": lambda: copy_dst.copy_(copy_src)}
        if es == 1:
            legs["box_blur3"] = lambda: det.box_blur(frames, radius=1)
        us = alternating(legs)
        for f, src in ((0, first), (B - 1, last)):
            got = out[f].view(torch.int16).cpu().numpy().view(np.uint16) if es == 2 else out[f].cpu().numpy()
            assert rows_equal(got, src, pat), f"{name}: frame {f} differs from numpy"
        r = {"bits": 8 * es, "pattern": pat, "bayer_grey": row(us["bayer_grey"], moved),
             "memcpy_device_to_device": row(us["memcpy_device_to_device"], moved)}
        r["bayer_over_memcpy"] = round(statistics.median(us["bayer_grey"]) / statistics.median(us["memcpy_device_to_device"]), 3)
        if es == 1:
            r["box_blur3"] = row(us["box_blur3"], moved)
            r["bayer_over_box_blur3"] = round(statistics.median(us["bayer_grey"]) / statistics.median(us["box_blur3"]), 3)
            r["bayer_minus_box_blur3_us"] = round(statistics.median(us["bayer_grey"]) - statistics.median(us["box_blur3"]), 1)
            r["box_blur3_spread_us"] = round(max(us["box_blur3"]) - min(us["box_blur3"]), 1)
        doc[name] = r
        del raw, frames, copy_src, copy_dst, out
        torch.cuda.empty_cache()
    det.close()
    _merge(out_path, "kernel", doc)


def host_fed(out_path):
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    import torch
    import mrgingham_amd
    from mrgingham_amd import _lib
    from tests import bayer_cases as bc
    bc.check_known()
    rounds, threads, pat = 3, 16, "rggb"
    det = mrgingham_amd.Detector()
    rng = np.random.default_rng(1)
    # page-locked: the mosaics as the grabber wrote them, and the grey frames a host that demosaiced them holds
    h_mosaic = torch.empty((B, H, W), dtype=torch.uint8, pin_memory=True)
    h_grey = torch.empty((B, H, W), dtype=torch.uint8, pin_memory=True)
    h_mosaic.numpy()[...] = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    d_mosaic = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    d_out = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    d_grey = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    L = _lib.lib()
    mosaic_np, grey_np = h_mosaic.numpy(), h_grey.numpy()

    def one(f):
        assert L.mrgingham_amd_bayer_grey_image(mosaic_np[f].ctypes.data, 8, W, H, W, mrgingham_amd.BAYER_PATTERNS[pat], grey_np[f].ctypes.data, W) == 0

    def leg_device(pool):
        d_mosaic.copy_(h_mosaic, non_blocking=True)
        det.bayer_grey(d_mosaic, pat, out=d_out)

    def leg_host(pool):
        list(pool.map(one, range(B)))
        d_grey.copy_(h_grey, non_blocking=True)

    ms = {"upload_and_bayer_grey": [], "host_threads_and_upload": []}
    with ThreadPoolExecutor(threads) as pool:
        for r in range(rounds + 1):                                   # (round 0 warms up)
            for name, leg in (("upload_and_bayer_grey", leg_device), ("host_threads_and_upload", leg_host)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg(pool)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if r:
                    ms[name].append(round(dt * 1e3, 3))
    assert torch.equal(d_out, d_grey), "the device's grey frames differ from the host's"
    assert np.array_equal(grey_np[B - 1][:3], bc.grey(mosaic_np[B - 1][:4], pat)[:3]) and np.array_equal(grey_np[0][-3:], bc.grey(mosaic_np[0][-4:], pat)[1:])
    dev, host = ms["upload_and_bayer_grey"], ms["host_threads_and_upload"]
    doc = {"device": torch.cuda.get_device_name(0), "frames": B, "width": W, "height": H, "bits": 8, "pattern": pat, "rounds": rounds,
           "link_bytes_each_leg": B * H * W, "host_threads": threads, "wall_ms_rounds": ms,
           "slowest_device_round_over_fastest_host_round": round(max(dev) / min(host), 3),
           "condition_met": max(dev) < min(host)}
    det.close()
    _merge(out_path, "host_fed", doc)


def main(args):
    import files_bench
    out = files_bench.opts(args, "--out", os.path.join(ROOT, "profiles", "bayer_grey_bench.json"))
    if "--kernel" in args:
        return kernel(out)
    if "--host-fed" in args:
        return host_fed(out)
    raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
