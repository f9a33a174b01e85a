"""What the BMP unpack kernel and the BMP batch loader cost:

    python tools/bmp_bench.py --kernel [--out profiles/bmp_unpack_bench.json]
    python tools/bmp_bench.py --loader [--rounds 3] [--jobs 16] [--files 64] [--out profiles/bmp_loader_bench.json]

--kernel: mrgingham_amd_bmp_unpack_batch over 64 pixel arrays of 4096x3072 (bottom-up) at 8 bits with the identity table, 8
  bits with a palette, 24, 32 and 1 bit: two warm-ups, then ten launches between device events; the median in us with min and
  max, bytes/s on the model of bits/8 + 1 bytes per pixel (the pixel array read, the grey byte written) and that as a
  fraction of 8 TB/s.  The yardsticks run in the same process, between the same events, alternating with the BMP launches:
  at 8 bits mrgingham_amd_pgm_unpack_batch over the same bytes and hipMemcpyAsync device-to-device of the same bytes
  (torch's copy_ of a contiguous tensor); at the other depths the copy of the depth's own pixel arrays.  Neither is code
  under test.  The output is compared with the host decoder's text (numpy) on rows of the first and the last frame.
--loader: mrgingham_amd_read_bmps_batch on `--files` names over two 12 MP 8-bit grey-ramp files in a RAM-backed directory,
  option "bmp_unpack" 1 against 0 (every file decoded by the host threads inside the same call), `--rounds` alternating
  rounds, wall time of the call: files/s per round.  One JSON document each."""
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
           "bytes_model": "bits/8 + 1 B per pixel: the pixel array read, one grey byte written"}
    out = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")

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

    def host_rows(raw, bits, lut):
        """rows of a pixel array (uint8 [rows, row_bytes]) -> grey [rows, W], the host decoder's arithmetic in numpy"""
        if bits == 8:
            return raw if lut is None else lut[raw]
        if bits == 1:
            return lut[np.unpackbits(raw, axis=1)[:, :W]]
        px = raw.reshape(raw.shape[0], W, bits // 8).astype(np.int64)
        return ((px[..., 2] * GREY[0] + px[..., 1] * GREY[1] + px[..., 0] * GREY[2] + 8192) >> 14).astype(np.uint8)

    px = H * W
    for name, bits, identity in (("8bit_identity", 8, True), ("8bit_palette", 8, False), ("24bit", 24, False), ("32bit", 32, False),
                                 ("1bit", 1, False)):
        rowb = (W * bits + 31) // 32 * 4
        one = rng.integers(0, 256, H * rowb, dtype=np.uint8)
        payload = torch.from_numpy(one).cuda().repeat(B, 1)
        payload[-1] = torch.from_numpy(one[::-1].copy()).cuda()           # (the last frame differs from the first)
        lut_np = None if identity or bits > 8 else rng.integers(0, 256, 256, dtype=np.uint8)
        lut = None if lut_np is None else torch.from_numpy(lut_np).cuda().repeat(B, 1)
        copy_dst = torch.empty_like(payload)
        legs = {"bmp_unpack": lambda: det.bmp_unpack(payload, lut, H, W, bits, out=out)}
        if bits == 8:
            pgm_out = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
            legs["pgm_unpack_8"] = lambda: det.pgm_unpack(payload, H, W, 8, out=pgm_out)
        legs["memcpy_device_to_device"] = lambda: copy_dst.copy_(payload)
        us = alternating(legs)
        for f, src in ((0, one), (B - 1, one[::-1])):
            raw = src.reshape(H, rowb)[[0, 1, H // 2, H - 1]]
            got = out[f].cpu().numpy()[[H - 1, H - 2, H - 1 - H // 2, 0]]        # (bottom-up: array row r is frame row H - 1 - r)
            assert np.array_equal(got, host_rows(raw, bits, lut_np)), f"{name}: frame {f} differs from the host arithmetic"
        r = {"bits": bits, "row_bytes": rowb, "bmp_unpack": row(us["bmp_unpack"], B * (H * rowb + px)),
             "memcpy_device_to_device": row(us["memcpy_device_to_device"], 2 * B * H * rowb)}
        if bits == 8:
            r["pgm_unpack_8"] = row(us["pgm_unpack_8"], 2 * B * px)
            r["bmp_over_pgm_unpack"] = round(statistics.median(us["bmp_unpack"]) / statistics.median(us["pgm_unpack_8"]), 3)
            del pgm_out
        doc[name] = r
        del payload, copy_dst, lut
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
    from tests import bmp_cases
    rounds, jobs, nfiles = (int(files_bench.opts(args, k, d)) for k, d in (("--rounds", "3"), ("--jobs", "16"), ("--files", "64")))
    scratch = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    doc = {"device": torch.cuda.get_device_name(0), "jobs": jobs, "files": nfiles, "rounds": rounds, "width": 4096, "height": 3072, "bits": 8}
    det = mrgingham_amd.Detector()
    try:
        files = []
        for i in range(2):
            img = synth.board_frame(4096, 3072, seed=i).numpy()
            files.append(os.path.join(scratch, f"grey{i}.bmp"))
            with open(files[-1], "wb") as f:
                f.write(bmp_cases.write(img, 8, bmp_cases.grey_ramp()))
        names = [files[i % 2] for i in range(nfiles)]
        want = [mrgingham_amd.read_image(p) for p in files]
        legs = {"device": [], "host": []}
        for r in range(rounds + 1):                                   # (round 0 warms the staging and the page cache up)
            for leg, unpack in (("device", 1), ("host", 0)):
                det.set_option("bmp_unpack", unpack)
                t0 = time.perf_counter()
                frames, status = det.read_bmps(names, nthreads=jobs)
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
        return kernel(files_bench.opts(args, "--out", os.path.join(ROOT, "profiles", "bmp_unpack_bench.json")))
    if "--loader" in args:
        return loader(args, files_bench.opts(args, "--out", os.path.join(ROOT, "profiles", "bmp_loader_bench.json")))
    raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
