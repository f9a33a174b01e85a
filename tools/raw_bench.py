"""What unpacking packed camera frames on the device costs, and what it saves a host-fed caller:

    python tools/raw_bench.py --kernel   [--out profiles/raw_unpack_bench.json]
    python tools/raw_bench.py --host-fed [--out profiles/raw_unpack_bench.json]

Both write into the same JSON document (each its own key; the other's stays).

--kernel: mrgingham_amd_raw_unpack_batch over 64 frames of 4096x3072 per format: two warm-ups, then ten launches between
  device events; the median in us with min and max, bytes/s on the model of N/8 + 2 bytes per pixel (1.5 + 2 for the pixel
  pairs: the packed row read, the uint16 sample written) and that as a fraction of 8 TB/s.  The yardsticks run in the same
  process, between the same events, alternating with the launches inside every round: a device-to-device copy that moves
  the same byte count (a tensor of (payload + output) / 2 bytes: read once, written once) and
  mrgingham_amd_pgm_unpack_batch at 16 bits producing the same uint16 frames.  Neither is code under test.  The output is
  compared with numpy (tests/raw_cases.py) on rows of the first and the last frame.
--host-fed: the same 64 12-bit frames from page-locked memory to uint16 frames on the device, two legs, each fenced, three
  alternating rounds after a warm-up round, wall time:
    1. upload the P12 payload, Detector.raw_unpack;
    2. upload uint16 frames the host already holds (no widening counted).
  The condition: the slowest round of leg 1 is faster than the fastest round of leg 2.  Beside them, for the document
  only, the wall time of 16 host threads widening the frames with mrgingham_amd_raw_unpack_image: the route a caller
  without the device call has."""
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


def kernel(out_path):
    import numpy as np
    import torch
    import mrgingham_amd
    from tests import raw_cases as rc
    det = mrgingham_amd.Detector()
    rng = np.random.default_rng(0)
    doc = {"device": torch.cuda.get_device_name(0), "frames": B, "width": W, "height": H,
           "bytes_model": "N / 8 + 2 B per pixel (pixel pairs: 1.5 + 2): the packed row read, one uint16 sample written",
           "kernel_geometry": dict(zip(("lanes_per_workgroup", "max_workgroups_per_cu"), mrgingham_amd.raw_unpack_geometry()))}

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

    px = H * W
    # the yardstick kernel's input: big-endian pairs, the same for every format
    pgm_pay = torch.from_numpy(rng.integers(0, 256, 2 * px, dtype=np.uint8)).cuda().repeat(B, 1)
    pgm_out = torch.empty((B, H, W), dtype=torch.uint16, device="cuda")
    for fmt in rc.FORMATS:
        rowb = mrgingham_amd.raw_row_bytes(W, fmt)
        one = rng.integers(0, 256, H * rowb, dtype=np.uint8)
        payload = torch.from_numpy(one).cuda().repeat(B, 1)
        payload[-1] = torch.from_numpy(one[::-1].copy()).cuda()           # (the last frame differs from the first)
        out = torch.empty((B, H, W), dtype=torch.uint16, device="cuda")
        moved = B * (H * rowb + 2 * px)
        copy_src = torch.empty((moved // 2,), dtype=torch.uint8, device="cuda")
        copy_dst = torch.empty_like(copy_src)
        legs = {"raw_unpack": lambda: det.raw_unpack(payload, H, W, fmt, out=out),
                "memcpy_device_to_device": lambda: copy_dst.copy_(copy_src),
                "pgm_unpack_16": lambda: det.pgm_unpack(pgm_pay, H, W, 16, out=pgm_out)}
        us = alternating(legs)
        rows = [0, 1, H // 2, H - 1]
        for f, src in ((0, one), (B - 1, one[::-1])):
            raw = np.ascontiguousarray(src.reshape(H, rowb)[rows])
            got = out[f].cpu().numpy()[rows]
            assert np.array_equal(got, rc.unpack(raw, W, fmt)), f"{fmt}: frame {f} differs from numpy"
        r = {"bits": rc.BITS[fmt], "row_bytes": rowb, "raw_unpack": row(us["raw_unpack"], moved),
             "memcpy_device_to_device": row(us["memcpy_device_to_device"], moved),
             "pgm_unpack_16": row(us["pgm_unpack_16"], 4 * B * px)}
        r["raw_over_memcpy"] = round(statistics.median(us["raw_unpack"]) / statistics.median(us["memcpy_device_to_device"]), 3)
        r["raw_over_pgm_unpack_16"] = round(statistics.median(us["raw_unpack"]) / statistics.median(us["pgm_unpack_16"]), 3)
        doc[fmt] = r
        del payload, copy_src, copy_dst, out
        torch.cuda.empty_cache()
    det.close()
    _merge(out_path, "kernel", doc)


def pack_p12(a):
    """uint16 [..., W] (W even, values below 4096) -> uint8 [..., W * 3 / 2]: Mono12p, two samples in three bytes"""
    import numpy as np
    p0, p1 = a[..., 0::2], a[..., 1::2]
    out = np.empty(a.shape[:-1] + (a.shape[-1] // 2, 3), dtype=np.uint8)
    out[..., 0] = p0 & 0xFF
    out[..., 1] = (p0 >> 8) | ((p1 & 0xF) << 4)
    out[..., 2] = p1 >> 4
    return out.reshape(a.shape[:-1] + (a.shape[-1] * 3 // 2,))


def host_fed(out_path):
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    import torch
    import mrgingham_amd
    from mrgingham_amd import _lib
    from tests import raw_cases as rc
    rounds, threads = 3, 16
    det = mrgingham_amd.Detector()
    rng = np.random.default_rng(1)
    rowb = mrgingham_amd.raw_row_bytes(W, "p12")
    # page-locked: the packed payloads as the grabber wrote them, and the frames a host that widened them would hold
    h_pay = torch.empty((B, H * rowb), dtype=torch.uint8, pin_memory=True)
    h_16 = torch.empty((B, H, W), dtype=torch.int16, pin_memory=True)
    for f in range(B):
        a = rng.integers(0, 4096, (H, W), dtype=np.uint16)
        if f == 0:
            assert np.array_equal(pack_p12(a[:2]), rc.pack(a[:2], "p12"))
        h_16[f] = torch.from_numpy(a.view(np.int16))
        h_pay[f] = torch.from_numpy(pack_p12(a).reshape(-1))
    d_pay = torch.empty((B, H * rowb), dtype=torch.uint8, device="cuda")
    d_out = torch.empty((B, H, W), dtype=torch.uint16, device="cuda")
    d_16 = torch.empty((B, H, W), dtype=torch.int16, device="cuda")

    def leg_packed():
        d_pay.copy_(h_pay, non_blocking=True)
        det.raw_unpack(d_pay, H, W, "p12", out=d_out)

    def leg_wide():
        d_16.copy_(h_16, non_blocking=True)

    ms = {"upload_p12_and_raw_unpack": [], "upload_uint16": []}
    for r in range(rounds + 1):                                       # (round 0 warms up)
        for name, leg in (("upload_p12_and_raw_unpack", leg_packed), ("upload_uint16", leg_wide)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r:
                ms[name].append(round(dt * 1e3, 3))
    assert torch.equal(d_out.view(torch.int16), d_16), "the unpacked frames differ from the frames uploaded directly"

    # the route a caller has without the device call: 16 host threads widen the frames
    L = _lib.lib()
    pay_np, wide = h_pay.numpy(), np.empty((B, H, W), dtype=np.uint16)

    def widen(f):
        assert L.mrgingham_amd_raw_unpack_image(pay_np[f].ctypes.data, H * rowb, W, H, rowb, 1, wide[f].ctypes.data, W) == 0
    host_ms = []
    with ThreadPoolExecutor(threads) as pool:
        for r in range(rounds + 1):
            t0 = time.perf_counter()
            list(pool.map(widen, range(B)))
            if r:
                host_ms.append(round((time.perf_counter() - t0) * 1e3, 1))
    assert np.array_equal(wide.view(np.int16), h_16.numpy())
    doc = {"device": torch.cuda.get_device_name(0), "frames": B, "width": W, "height": H, "format": "p12", "rounds": rounds,
           "link_bytes": {"upload_p12_and_raw_unpack": B * H * rowb, "upload_uint16": 2 * B * H * W},
           "wall_ms_rounds": ms,
           "slowest_packed_round_over_fastest_uint16_round": round(max(ms["upload_p12_and_raw_unpack"]) / min(ms["upload_uint16"]), 3),
           "condition_met": max(ms["upload_p12_and_raw_unpack"]) < min(ms["upload_uint16"]),
           "link_GBps": {k: [round(bytes_ / (v * 1e-3) / 1e9, 1) for v in ms[k]]
                         for k, bytes_ in (("upload_p12_and_raw_unpack", B * H * rowb), ("upload_uint16", 2 * B * H * W))},
           "host_threads": threads, "host_widening_wall_ms_rounds": host_ms}
    det.close()
    _merge(out_path, "host_fed", doc)


def main(args):
    import files_bench
    out = files_bench.opts(args, "--out", os.path.join(ROOT, "profiles", "raw_unpack_bench.json"))
    if "--kernel" in args:
        return kernel(out)
    if "--host-fed" in args:
        return host_fed(out)
    raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
