"""What decoding restart intervals on the device buys the JPEG loader:

    python tools/jpeg_huff_bench.py --make DIR                   (needs Pillow: writes the three files below into DIR)
    python tools/jpeg_huff_bench.py --file A.jpg [--file B.jpg ...] [--frames 64] [--launches 30]
                                    [--out profiles/jpeg_huff_bench.json]

The files are three encodings of the same pixels, synth.board_frame(4096, 3072) at quality 90: one restart interval per
MCU row (rows.jpg), 8 MCUs per interval (dri8.jpg) and no restart intervals (nodri.jpg).  Per file, read `--frames`
times, in one process on one box:
  kernel   jpeg_huff_kernel alone (files with restart intervals): hipEvents around the launches of one
           Detector.jpeg_entropy call over the batch (kernel timing on), median / min / max of --launches calls after three
           warm-up ones, for both block-filling variants (option "jpeg_entropy_memset"; the variant with the memset in
           front is charged the memset, timed by torch events around an equal one); Huffman symbols per second (counted
           from the host decoder's coefficients: one DC symbol per block, one per non-zero AC coefficient, ZRLs and EOBs)
           and compressed bytes per second;
  loader   Detector.read_jpegs at 1 / 4 / 16 host threads with entropy="host" and entropy="device", alternating: frames
           per second, best and median of three calls after a warm-up one of each;
  upload   bytes per frame that cross the link on either path (host: 2 B per coefficient of the padded block area + the
           table; device: the staging image -- records, tables, interval offsets, compressed bytes).
One JSON document.

    python tools/jpeg_huff_bench.py --sync --file nodri.jpg --file nodri420.jpg [--frames 64] [--launches 30]
                                    [--out profiles/jpeg_sync_bench.json]

The files WITHOUT restart intervals through the self-synchronising decoder (option "jpeg_sync"; --make writes the board
in grey, nodri.jpg, and in 4:2:0, nodri420.jpg).  Per file and per subsequence size S in 32, 64, 128:
  rounds   what mrgingham_amd.jpeg_sync_rounds counts, and the subsequences;
  kernels  hipEvents around round 0, the update rounds (cap + 1 launches), the scan and the write pass, each alone
           (option "jpeg_sync_time_phase") and around all of them, of one Detector.jpeg_entropy(sync=True) call over the
           batch: median of --launches calls after three warm-up ones;
  loader   Detector.read_jpegs at 1 / 4 / 16 host threads with entropy="host" and entropy="device", sync=True,
           alternating in one process: frames per second, best and median of three calls after a warm-up one of each;
  upload   bytes per frame that cross the link on either path.
One JSON document."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def opts(args, name):
    return [args[i + 1] for i, a in enumerate(args) if a == name]


def make(out_dir):
    from PIL import Image
    from mrgingham_amd import synth
    os.makedirs(out_dir, exist_ok=True)
    img = Image.fromarray(synth.board_frame(4096, 3072).numpy())
    img.save(os.path.join(out_dir, "rows.jpg"), "JPEG", quality=90, restart_marker_rows=1)
    img.save(os.path.join(out_dir, "dri8.jpg"), "JPEG", quality=90, restart_marker_blocks=8)
    img.save(os.path.join(out_dir, "nodri.jpg"), "JPEG", quality=90)
    img.convert("RGB").save(os.path.join(out_dir, "nodri420.jpg"), "JPEG", quality=90, subsampling=2)
    for n in ("rows.jpg", "dri8.jpg", "nodri.jpg", "nodri420.jpg"):
        print(n, os.path.getsize(os.path.join(out_dir, n)))


def symbols_of(coef):
    """Huffman symbols the luma blocks of a grey file decode to: DC + non-zero ACs + ZRLs + EOBs."""
    import numpy as np
    ac = coef.reshape(-1, 64)
    nat = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                    54, 47, 55, 62, 63])
    zz = ac[:, nat] != 0
    total = zz.shape[0] + int(zz[:, 1:].sum())                       # DC symbols + coded AC values
    last = np.where(zz[:, 1:].any(axis=1), 63 - np.argmax(zz[:, :0:-1], axis=1), 0)
    total += int((last < 63).sum())                                   # EOBs
    pos = np.where(zz[:, 1:], np.arange(1, 64)[None, :], 0)
    prev = np.maximum.accumulate(pos, axis=1)
    prev = np.concatenate([np.zeros((len(pos), 1), int), prev[:, :-1]], axis=1)
    runs = np.where(zz[:, 1:], np.arange(1, 64)[None, :] - prev - 1, 0)
    total += int((runs // 16).sum())                                  # ZRLs
    return total


def loader_legs(det, paths, B, ways):
    """ways: {name: read_jpegs keywords}, alternating -> {"threads_N": {name: {best, median}, ...}}"""
    out = {}
    for n in (1, 4, 16):
        legs = {w: [] for w in ways}
        for w, kw in ways.items():
            det.read_jpegs(paths, nthreads=n, **kw)          # warm-up
        for _ in range(1 if n == 1 else 3):
            for w, kw in ways.items():
                t0 = time.perf_counter()
                det.read_jpegs(paths, nthreads=n, **kw)
                legs[w].append(time.perf_counter() - t0)
        out[f"threads_{n}"] = {w: {"frames_per_s_best": round(B / min(v), 1), "frames_per_s_median": round(B / statistics.median(v), 1)}
                               for w, v in legs.items()}
    return out


def sync_main(args):
    import torch
    import mrgingham_amd
    files = opts(args, "--file")
    B = int((opts(args, "--frames") or ["64"])[0])
    launches = int((opts(args, "--launches") or ["30"])[0])
    out_path = (opts(args, "--out") or [os.path.join(ROOT, "profiles", "jpeg_sync_bench.json")])[0]
    det = mrgingham_amd.Detector(0)
    doc = {"frames": B, "device": torch.cuda.get_device_name(0), "files": {}}
    phases = ("all", "round0", "rounds", "scan", "write")
    for path in files:
        data = open(path, "rb").read()
        coef, quant, (H, W) = mrgingham_amd.jpeg_coefficients(data)
        want = mrgingham_amd.read_image(path)
        padded = lambda side: max(-(-side // (8 * h)) * h for h in (1, 2, 3, 4))      # noqa: E731
        sos = data.index(b"\xff\xda")
        stream = len(data) - 2 - (sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big"))
        ntables = 2 if b"\xff\xc0\x00\x0b" in data else 4                       # (SOF0 of one component: grey)
        host_upload = padded(H) * padded(W) * 64 * 2 + 128
        # the sync path's own image: record (80) + Huffman tables + the padded stream; the other image: record (64) + table (128)
        dev_upload = 80 + ntables * 1424 + ((stream + 3) & ~3) + 4 + 64 + 128
        entry = {"file_bytes": len(data), "width": W, "height": H, "entropy_bytes": stream,
                 "upload_bytes_per_frame": {"host": host_upload, "device": dev_upload, "host_over_device": round(host_upload / dev_upload, 2)},
                 "subsequence": {}}
        for S in (32, 64, 128):
            rounds, nsub = mrgingham_amd.jpeg_sync_rounds(data, S)
            leg = {"rounds": rounds, "subsequences": nsub, "cap": 8192 // S}
            det.set_option("jpeg_sync_subsequence", S)
            det.set_kernel_timing(1)
            det.chess_kernel_ms()
            for phase, name in enumerate(phases):
                det.set_option("jpeg_sync_time_phase", phase)
                us = []
                for k in range(3 + launches):
                    d_coef, d_quant, status = det.jpeg_entropy([data] * B, H, W, sync=True)
                    ms, n = det.chess_kernel_ms()
                    assert n == 1 and (status == 0).all(), (n, status)
                    if k >= 3:
                        us.append(ms * 1e3)
                leg[f"us_per_batch_{name}"] = {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)}
            det.set_option("jpeg_sync_time_phase", 0)
            det.set_kernel_timing(0)
            leg["equals_host_decoder"] = bool((d_coef[B - 1, :coef.shape[0], :coef.shape[1]].cpu().numpy() == coef).all())
            leg["compressed_bytes_per_s"] = round(stream * B / (leg["us_per_batch_all"]["median"] * 1e-6))
            del d_coef, d_quant
            paths = [path] * B
            leg["loader"] = loader_legs(det, paths, B, {"host": dict(entropy="host"), "sync": dict(entropy="device", sync=True)})
            for e in leg["loader"].values():
                e["sync_over_host_median"] = round(e["sync"]["frames_per_s_median"] / e["host"]["frames_per_s_median"], 3)
            frames, status = det.read_jpegs(paths, nthreads=16, entropy="device", sync=True)
            leg["loader"]["equals_host_decoder"] = bool((status == 0).all() and (frames[B // 2].cpu().numpy() == want).all()
                                                        and (frames[B - 1].cpu().numpy() == want).all())
            entry["subsequence"][str(S)] = leg
            print(os.path.basename(path), S, json.dumps(leg), flush=True)
        det.set_option("jpeg_sync_subsequence", 32)
        doc["files"][os.path.basename(path)] = entry
    det.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print("wrote", out_path)


def main():
    args = sys.argv[1:]
    if "--make" in args:
        return make(opts(args, "--make")[0])
    if "--sync" in args:
        return sync_main(args)
    import numpy as np
    import torch
    import mrgingham_amd
    files = opts(args, "--file")
    if not files:
        sys.exit("jpeg_huff_bench.py: give the files with --file (make them with --make DIR where Pillow is installed)")
    B = int((opts(args, "--frames") or ["64"])[0])
    launches = int((opts(args, "--launches") or ["30"])[0])
    out_path = (opts(args, "--out") or [os.path.join(ROOT, "profiles", "jpeg_huff_bench.json")])[0]
    det = mrgingham_amd.Detector(0)
    doc = {"frames": B, "device": torch.cuda.get_device_name(0), "files": {}}
    for path in files:
        data = open(path, "rb").read()
        coef, quant, (H, W) = mrgingham_amd.jpeg_coefficients(data)
        dri, offsets = mrgingham_amd.jpeg_restart_intervals(data)
        want = mrgingham_amd.read_image(path)
        entry = {"file_bytes": len(data), "width": W, "height": H, "restart_interval": dri, "intervals": len(offsets)}
        padded = lambda side: max(-(-side // (8 * h)) * h for h in (1, 2, 3, 4))      # noqa: E731
        host_upload = padded(H) * padded(W) * 64 * 2 + 128
        # records (64) + table (128) + Huffman tables (grey: 2 x 1424) + 8 per interval + the padded stream
        lo = int(offsets[0, 0]) if dri else 0
        stream = ((int(offsets[-1, 1]) - lo + 3) & ~3) + 4 if dri else 0
        dev_upload = 64 + 128 + 2 * 1424 + 8 * len(offsets) + stream if dri else host_upload + 192
        entry["upload_bytes_per_frame"] = {"host": host_upload, "device": dev_upload, "host_over_device": round(host_upload / dev_upload, 2)}

        if dri:     # the kernel alone
            symbols = symbols_of(coef)
            entry["symbols_per_frame"] = symbols
            zero_like = torch.empty((B, padded(H), padded(W), 64), dtype=torch.int16, device=det.device)
            for memset in (0, 1):
                det.set_option("jpeg_entropy_memset", memset)
                det.set_kernel_timing(1)
                det.chess_kernel_ms()
                us = []
                for k in range(3 + launches):
                    d_coef, d_quant, status = det.jpeg_entropy([data] * B, H, W)
                    ms, n = det.chess_kernel_ms()
                    assert n == 1 and (status == 0).all()
                    if k >= 3:
                        us.append(ms * 1e3)
                det.set_kernel_timing(0)
                ok = bool((d_coef[B - 1, :coef.shape[0], :coef.shape[1]].cpu().numpy() == coef).all())
                med = statistics.median(us)
                leg = {"launches": launches, "us_per_batch_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                       "equals_host_decoder": ok}
                if memset:
                    ms_ = []
                    for _ in range(10):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        zero_like.zero_()
                        e1.record()
                        e1.synchronize()
                        ms_.append(e0.elapsed_time(e1) * 1e3)
                    leg["memset_us_median"] = round(statistics.median(ms_), 1)
                    med += statistics.median(ms_)
                    leg["us_with_memset"] = round(med, 1)
                leg["symbols_per_s"] = round(symbols * B / (med * 1e-6))
                leg["compressed_bytes_per_s"] = round(stream * B / (med * 1e-6))
                entry["kernel_memset_front" if memset else "kernel_whole_blocks"] = leg
                del d_coef, d_quant
            det.set_option("jpeg_entropy_memset", 0)
            del zero_like

        # the loader, both ways, alternating
        paths = [path] * B
        entry["loader"] = {}
        for n in (1, 4, 16):
            legs = {"host": [], "device": []}
            for which in ("host", "device"):
                det.read_jpegs(paths, nthreads=n, entropy=which)          # warm-up
            for _ in range(1 if n == 1 else 3):
                for which in ("host", "device"):
                    t0 = time.perf_counter()
                    frames, status = det.read_jpegs(paths, nthreads=n, entropy=which)
                    legs[which].append(time.perf_counter() - t0)
            e = {}
            for which in ("host", "device"):
                e[which] = {"frames_per_s_best": round(B / min(legs[which]), 1), "frames_per_s_median": round(B / statistics.median(legs[which]), 1)}
            e["device_over_host_median"] = round(e["device"]["frames_per_s_median"] / e["host"]["frames_per_s_median"], 3)
            entry["loader"][f"threads_{n}"] = e
        frames, status = det.read_jpegs(paths, nthreads=16, entropy="device")
        entry["loader"]["equals_host_decoder"] = bool((status == 0).all() and (frames[B // 2].cpu().numpy() == want).all()
                                                      and (frames[B - 1].cpu().numpy() == want).all())
        doc["files"][os.path.basename(path)] = entry
        print(os.path.basename(path), json.dumps(entry), flush=True)
    det.close()
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
