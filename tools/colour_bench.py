"""What taking colour frames to grey on the device costs, against the routes a caller had before:

    python tools/colour_bench.py [--out profiles/colour_grey_bench.json] [--only rgb_8,rgba_16,...]

mrgingham_amd_colour_grey_batch over 64 frames of 4096x3072 for every format and sample width: two warm-up rounds, then
ten rounds between device events; the median in us with min and max, and bytes/s on the model of C*ES + ES bytes per
pixel (every source sample read once -- the ignored ones too: they share their cache lines -- and every grey written
once; C = 3, 4, 3 planar, 2 for 4:2:2).  No fraction of a peak is fixed in advance.  Inside every round each launch
alternates with
  (a) a device-to-device copy that moves the same byte count,
  (b) for contiguous rgb / rgba at 8 bit, Detector.pnm_unpack on the same bytes (the same work by the existing kernel),
  (c) the torch expression of the definition on the same frames, whose result must be torch.equal to the launch's.
None of the three is code under test.  Rows of the first and the last frame are compared with numpy
(tests/colour_cases.py).

The one condition (a caller already has route (b)): for contiguous 8-bit rgb, the median of colour_grey may exceed that of
pnm_unpack by at most pnm_unpack's own min-max spread in the same process; "rgb_8" carries "condition_met"."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
B, H, W = 64, 3072, 4096


def torch_grey(torch, frames, fmt, channels):
    """the definition as torch expressions: 64-bit intermediates, several passes"""
    wide = (frames.view(torch.int16).to(torch.int64) & 0xFFFF) if frames.dtype == torch.uint16 else frames.to(torch.int64)
    if channels == 2:
        g = wide[..., 1 if fmt == "uyvy" else 0]
    else:
        s = (wide[:, 0], wide[:, 1], wide[:, 2]) if channels == 0 else (wide[..., 0], wide[..., 1], wide[..., 2])
        r, gg, b = s[::-1] if fmt.startswith("bgr") else s
        g = (4899 * r + 9617 * gg + 1868 * b + 8192) >> 14
    if frames.dtype == torch.uint16:
        return g.to(torch.int16).view(torch.uint16)      # (the low 16 bits)
    return g.to(torch.uint8)


def run(out_path, only):
    import numpy as np
    import torch
    import mrgingham_amd
    from tests import colour_cases as cc
    cc.check_known()
    det = mrgingham_amd.Detector()
    rng = np.random.default_rng(0)
    doc = {"device": torch.cuda.get_device_name(0), "frames": B, "width": W, "height": H,
           "bytes_model": "C*ES + ES bytes per pixel: every source sample read once, every grey written once",
           "kernel_geometry": dict(zip(("lanes_per_workgroup", "max_workgroups_per_cu"), mrgingham_amd.colour_grey_geometry()))}
    if os.path.exists(out_path):                                        # (a run of some cases keeps the others)
        with open(out_path) as f:
            old = json.load(f)
        if old.get("device") == doc["device"]:
            doc.update({k: v for k, v in old.items() if k not in doc})

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
        return {"us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1), "us": [round(v, 1) for v in us],
                "bytes_per_s": round(bytes_moved / (med * 1e-6), -9)}

    def host(t):
        t = t.contiguous()
        return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.uint16 else t.cpu().numpy()

    for fmt, dtype in cc.cases():
        es = np.dtype(dtype).itemsize
        name = f"{fmt}_{8 * es}"
        if only and name not in only:
            continue
        C = cc.CHANNELS[fmt]
        per_pixel = (C or 3) * es + es
        # one random frame over and over, the last frame the first one upside down (assembled as int16 where the samples
        # are uint16: torch copies those everywhere)
        first = cc.random_frames(1, H, W, fmt, dtype, seed=int(rng.integers(1 << 30)))[0]
        last = np.ascontiguousarray(first[:, ::-1] if cc.planar(fmt) else first[::-1])
        as_torch = lambda a: torch.from_numpy(a.view(np.int16) if es == 2 else a).cuda()
        raw = as_torch(first).repeat(B, 1, 1, 1)
        raw[-1] = as_torch(last)
        frames = raw.view(torch.uint16) if es == 2 else raw
        out = torch.empty((B, H, W), dtype=frames.dtype, device="cuda")
        moved = per_pixel * B * H * W
        copy_src = torch.empty((moved // 2,), dtype=torch.uint8, device="cuda")
        copy_dst = torch.empty_like(copy_src)
        kept = {}

        def by_torch():
            kept["torch"] = torch_grey(torch, frames, fmt, C)
        legs = {"colour_grey": lambda: det.colour_grey(frames, fmt, out=out),
                "memcpy_device_to_device": lambda: copy_dst.copy_(copy_src)}
        if name in ("rgb_8", "rgba_8"):
            payload, old_out = frames.view(B, -1), torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
            legs["pnm_unpack"] = lambda: det.pnm_unpack(payload, H, W, 8, C, out=old_out)
        legs["torch_expression"] = by_torch
        us = alternating(legs)
        assert torch.equal(kept["torch"], out), f"{name}: the torch expression differs from the launch"
        if "pnm_unpack" in legs:
            assert torch.equal(old_out, out), f"{name}: pnm_unpack differs from the launch"
        for f, src in ((0, first), (B - 1, last)):
            got, want = host(out[f]), cc.grey(src[:, :4] if cc.planar(fmt) else src[:4], fmt)
            assert np.array_equal(got[:4], want), f"{name}: the first rows of frame {f} differ from numpy"
            want = cc.grey(src[:, -4:] if cc.planar(fmt) else src[-4:], fmt)
            assert np.array_equal(got[-4:], want), f"{name}: the last rows of frame {f} differ from numpy"
        med = {k: statistics.median(v) for k, v in us.items()}
        r = {"bits": 8 * es, "format": fmt, "bytes_per_pixel": per_pixel}
        r.update({k: row(v, moved) for k, v in us.items()})
        r["colour_over_memcpy"] = round(med["colour_grey"] / med["memcpy_device_to_device"], 3)
        r["colour_over_torch_expression"] = round(med["colour_grey"] / med["torch_expression"], 3)
        if "pnm_unpack" in legs:
            spread = max(us["pnm_unpack"]) - min(us["pnm_unpack"])
            r["colour_minus_pnm_unpack_us"] = round(med["colour_grey"] - med["pnm_unpack"], 1)
            r["pnm_unpack_spread_us"] = round(spread, 1)
            if name == "rgb_8":
                r["condition_met"] = bool(med["colour_grey"] - med["pnm_unpack"] <= spread)
        doc[name] = r
        print(json.dumps({name: {k: (v if not isinstance(v, dict) else {q: v[q] for q in ("us_median", "us_min", "us_max")}) for k, v in r.items()}}))
        sys.stdout.flush()
        del raw, frames, copy_src, copy_dst, out, kept, legs
        torch.cuda.empty_cache()
    det.close()
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def main(args):
    import files_bench
    out = files_bench.opts(args, "--out", os.path.join(ROOT, "profiles", "colour_grey_bench.json"))
    only = files_bench.opts(args, "--only", "")
    run(out, set(only.split(",")) if only else None)


if __name__ == "__main__":
    main(sys.argv[1:])
