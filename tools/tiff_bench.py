"""What the TIFF device route (tiff_decode.hip, mrgingham_amd_read_tiffs_batch) costs and buys at 12 MP:

    python tools/tiff_bench.py [--rounds 3] [--jobs 16] [--frames 64] [--codec lzw|deflate|both] [--out profiles/tiff_bench.json; --codec deflate: profiles/tiff_deflate_bench.json]

Files: two 4096x3072 frames (synth.board_frame plus noise), 8 bit and 16 bit, written by Pillow's libtiff into a RAM-backed
directory -- LZW with predictor 2 at 2, 16 and 256 rows per strip (8 KiB, 64 KiB and 1 MiB decoded per strip at 8 bit) and
uncompressed (--codec lzw, the default); with --codec deflate or both the same files as Deflate (Pillow's tiff_adobe_deflate) with predictor 2.
1. The launches alone: `--frames` files uploaded once, mrgingham_amd_tiff_decode_batch between two device events (two
   warm-up calls, the median of ten), its output checked against the source array.  On an LZW file that is the check
   kernel, the LZW kernel (one lane per strip) and the finish kernel; on the same pixels uncompressed it is the check and
   the finish kernel alone, so the difference prices the LZW launch.  For the finish kernel the bytes its algorithm moves
   -- one read of rowbytes x height and one write of width x height x bits / 8 per frame -- and the fraction of the HBM
   peak (8.0 TB/s) that is.  The three strip sizes are the sweep behind option "tiff_lzw_max_strip".
2. The loader: `--frames` names over the two files through Detector.read_tiffs with `--jobs` host threads, at every strip
   size of the sweep: the device route (option "tiff_lzw_max_strip" at its limit, 1 MiB, so that every file is taken)
   against the same call with every file forced to the host decoder (the option at 1), alternating, `--rounds` times in
   one process; frames per second of wall time.  These pairs are what the option's default is read from.  The Deflate
   legs: read_tiffs(deflate="device") with option "tiff_deflate_max_strip" at 1 MiB against read_tiffs(deflate="host"), which
   leaves every Deflate file to the host threads and zlib.
One JSON document.

    python tools/tiff_bench.py --tile 64x64,128x128,256x256,512x512 [--rounds 3] [--jobs 16] [--frames 64] [--out profiles/tiff_tiled_bench.json]

The same two measurements on TILED files of the same frames.  Pillow writes no tiles, so the files
come from a writer of this tool's own: little-endian, one IFD behind the tiles, every tile a stream of its own -- LZW (the
bytes of the tile, horizontal differences taken along each row of the tile, compressed by Pillow's libtiff as a one-strip
file whose strip is taken out), Deflate (zlib, level 6) or none; 4096 and 3072 are multiples of every tile side, so no
tile is padded.
1. The launches: mrgingham_amd_tiff_decode_batch_tiled on uncompressed tiles of every size (check kernel and
   tiff_finish_tiles_kernel alone) at 8 and 16 bit, beside mrgingham_amd_tiff_decode_batch on the same pixels in uncompressed
   strips (tiff_finish_kernel) in the same process, and on the LZW and Deflate tiles of every size.
2. The loader: LZW and Deflate with predictor 2 at every tile size at 8 bit, and at the 16-bit size (--tile16, default
   128x128), the device route against the same call on the host threads, alternating."""
import ctypes
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
W, H = 4096, 3072


def opts(args, name, default=None):
    return args[args.index(name) + 1] if name in args else default


def board(seed, bits):
    from mrgingham_amd import synth
    rng = np.random.default_rng(seed)
    grey = synth.board_frame(W, H, 10, seed=seed).numpy().astype(np.int32)
    img = np.clip(grey + rng.integers(-3, 4, grey.shape), 0, 255)
    return img.astype(np.uint8) if bits == 8 else (img * 257 + rng.integers(0, 64, grey.shape)).astype(np.uint16)


PILLOW_NAME = {"lzw": "tiff_lzw", "deflate": "tiff_adobe_deflate"}


def write_files(scratch, codecs):
    from PIL import Image
    files, source = {}, {}
    for bits in (8, 16):
        for seed in (1, 2):
            img = board(seed, bits)
            source[bits, seed] = img
            variants = [("none", dict(tiffinfo={278: 2}))]
            for codec in codecs:
                variants += [(f"{codec}_rows{rows}", dict(compression=PILLOW_NAME[codec], tiffinfo={317: 2, 278: rows})) for rows in (2, 16, 256)]
            for name, kw in variants:
                if bits == 16 and name.endswith(("_rows16", "_rows256")):
                    continue
                if bits == 16 and name.endswith("_rows2"):
                    kw = dict(kw, tiffinfo={317: 2, 278: 1})     # 8 KiB decoded per strip at 16 bit
                p = os.path.join(scratch, f"b{bits}_{name}_{seed}.tif")
                Image.fromarray(img).save(p, "TIFF", **kw)
                files[bits, name, seed] = p
    return files, source


def tile_stream(rows, codec):
    """One tile's bytes as they lie in the file.  rows: uint8 [tile length, bytes of a tile's row], differences taken."""
    import zlib
    if codec == "none":
        return rows.tobytes()
    if codec == "deflate":
        return zlib.compress(rows.tobytes(), 6)
    import mrgingham_amd
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rows).save(b, "TIFF", compression="tiff_lzw", tiffinfo={278: rows.shape[0]})
    d = b.getvalue()
    lay = mrgingham_amd.tiff_layout(d)
    assert lay is not None and lay.nstrips == 1 and lay.predictor == 1 and lay.width == rows.shape[1]
    return d[int(lay.strips["offset"][0]):int(lay.strips["offset"][0]) + int(lay.strips["nbytes"][0])]


def write_tiled(path, img, tw, tl, codec):
    """img uint8 / uint16 [H, W], H and W multiples of the tile's sides; predictor 2 with LZW and Deflate."""
    import struct
    h, w = img.shape
    assert h % tl == 0 and w % tw == 0
    bits = 8 * img.dtype.itemsize
    body, offsets, counts = bytearray(), [], []
    for y in range(0, h, tl):
        for x in range(0, w, tw):
            t = img[y:y + tl, x:x + tw]
            if codec != "none":
                t = np.concatenate([t[:, :1], t[:, 1:] - t[:, :-1]], axis=1)      # (wraps modulo 2^bits)
            stream = tile_stream(np.ascontiguousarray(t.astype("<u%d" % (bits // 8))).view(np.uint8).reshape(tl, -1), codec)
            offsets.append(8 + len(body))
            counts.append(len(stream))
            body += stream + (b"\0" if len(stream) % 2 else b"")
    n = len(offsets)
    entries = [(256, 4, [w]), (257, 4, [h]), (258, 3, [bits]), (259, 3, [{"none": 1, "lzw": 5, "deflate": 8}[codec]]), (262, 3, [1]),
               (277, 3, [1]), (284, 3, [1]), (317, 3, [1 if codec == "none" else 2]), (322, 3, [tw]), (323, 3, [tl]), (324, 4, offsets),
               (325, 4, counts)]
    extra, ifd = bytearray(), bytearray()
    base = 8 + len(body)
    for tag, typ, vals in entries:
        data = struct.pack("<%d%s" % (len(vals), "H" if typ == 3 else "I"), *vals)
        if len(data) <= 4:
            field = data.ljust(4, b"\0")
        else:
            field = struct.pack("<I", base + len(extra))
            extra += data
        ifd += struct.pack("<HHI", tag, typ, len(vals)) + field
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, base + len(extra)) + bytes(body) + bytes(extra) + struct.pack("<H", len(entries)) + bytes(ifd)
                + struct.pack("<I", 0))
    return n


def launch_ms(det, datas, want, frames, tiles=False):
    """decode_batch over `frames` copies of the files, uploaded once: median ms of ten calls.  tiles: through
    mrgingham_amd_tiff_layout_tiled and _tiff_decode_batch_tiled."""
    import torch
    import mrgingham_amd
    from mrgingham_amd import _lib, api
    lays = [mrgingham_amd.tiff_layout(d, deflate_max_strip=1 << 20, **({"tiles": True} if tiles else {})) for d in datas]
    assert all(l is not None and l.taken for l in lays) and len({l.key() for l in lays}) == 1
    lay, P = lays[0], max(l.nstrips for l in lays)
    pitch = (max(len(d) for d in datas) + 15) // 16 * 16
    h_files = np.zeros((frames, pitch), np.uint8)
    h_strips = np.zeros((frames, P), api.TIFF_STRIP)
    for i in range(frames):
        d, l = datas[i % len(datas)], lays[i % len(datas)]
        h_files[i, :len(d)] = np.frombuffer(d, np.uint8)
        h_strips[i, :l.nstrips] = l.strips
    d_files = torch.from_numpy(h_files).cuda()
    d_strips = torch.from_numpy(h_strips.view(np.uint8).reshape(frames, -1)).cuda()
    d_ns = torch.tensor([lays[i % len(datas)].nstrips for i in range(frames)], dtype=torch.int32, device="cuda")
    d_status = torch.zeros(frames, dtype=torch.int32, device="cuda")
    d_out = torch.empty((frames, H, W), dtype=torch.uint8 if lay.bits == 8 else torch.uint16, device="cuda")
    info = _lib.TiffInfo(*lay.key())
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        if tiles:
            assert det.L.mrgingham_amd_tiff_decode_batch_tiled(det.ctx, d_files.data_ptr(), pitch, d_strips.data_ptr(), P, d_ns.data_ptr(),
                                                               frames, ctypes.byref(info), lay.tile_width, lay.tile_length, d_out.data_ptr(),
                                                               H * W, W, d_status.data_ptr(), None, stream) == 0
            return
        assert det.L.mrgingham_amd_tiff_decode_batch(det.ctx, d_files.data_ptr(), pitch, d_strips.data_ptr(), P, d_ns.data_ptr(), frames,
                                                     ctypes.byref(info), d_out.data_ptr(), H * W, W, d_status.data_ptr(), None, stream) == 0
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    assert not d_status.any().item()
    for i in (0, 1, frames - 1):
        assert np.array_equal(d_out[i].cpu().numpy(), want[i % len(want)]), "the kernels' output differs from the source"
    ms = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    rowb = W * lay.samples * lay.bits // 8
    return {"ms_per_launch": round(statistics.median(ms), 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "strips_per_frame": P,
            "decoded_bytes_per_strip": int(lay.strips["rows"][0]) * (getattr(lay, "tile_width", 0) * lay.samples * lay.bits // 8 or rowb), "file_bytes": [len(d) for d in datas],
            "finish_bytes_per_launch": frames * (rowb * H + W * H * lay.bits // 8)}


def finish_rate(r):
    t = r["ms_per_launch"] * 1e-3
    r["finish_bytes_per_s"] = round(r["finish_bytes_per_launch"] / t)
    r["finish_fraction_of_hbm_peak"] = round(r["finish_bytes_per_launch"] / t / HBM_PEAK, 4)


def main_tiled(args):
    import torch
    import mrgingham_amd
    from mrgingham_amd import _lib
    from PIL import Image
    rounds, jobs, frames = int(opts(args, "--rounds", "3")), int(opts(args, "--jobs", "16")), int(opts(args, "--frames", "64"))
    sizes = [tuple(int(v) for v in t.split("x")) for t in opts(args, "--tile").split(",")]
    size16 = tuple(int(v) for v in opts(args, "--tile16", "128x128").split("x"))
    out_path = opts(args, "--out", os.path.join(ROOT, "profiles", "tiff_tiled_bench.json"))
    doc = {"device": torch.cuda.get_device_name(0), "jobs": jobs, "rounds": rounds, "frames": frames, "frame": [W, H],
           "hbm_peak_bytes_per_s": HBM_PEAK, "geometry_lanes_segment_step": list(mrgingham_amd.tiff_geometry()),
           "inflate_lanes": _lib.lib().mrgingham_amd_tiff_inflate_lanes(), "tiles": ["%dx%d" % t for t in sizes], "tile_16_bit": "%dx%d" % size16,
           "launches": {}, "loader": {}}
    scratch = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    det = mrgingham_amd.Detector(0)
    try:
        source = {(bits, seed): board(seed, bits) for bits in (8, 16) for seed in (1, 2)}

        def files_of(bits, tw, tl, codec):
            paths = []
            for seed in (1, 2):
                p = os.path.join(scratch, f"b{bits}_{codec}_{tw}x{tl}_{seed}.tif")
                if codec == "strip_none":
                    Image.fromarray(source[bits, seed]).save(p, "TIFF", tiffinfo={278: 2})
                else:
                    write_tiled(p, source[bits, seed], tw, tl, codec)
                paths.append(p)
            return paths

        for bits in (8, 16):      # the two finish kernels on the same pixels, uncompressed, in one process
            paths = files_of(bits, 0, 0, "strip_none")
            r = launch_ms(det, [open(p, "rb").read() for p in paths], [source[bits, 1], source[bits, 2]], frames)
            finish_rate(r)
            doc["launches"][f"b{bits}_strip_none"] = r
            print(f"launch b{bits}_strip_none: {r['ms_per_launch']} ms", file=sys.stderr, flush=True)
            for p in paths:
                os.remove(p)
            for tw, tl in sizes:
                paths = files_of(bits, tw, tl, "none")
                r = launch_ms(det, [open(p, "rb").read() for p in paths], [source[bits, 1], source[bits, 2]], frames, tiles=True)
                finish_rate(r)
                r["ratio_to_strip_finish"] = round(r["ms_per_launch"] / doc["launches"][f"b{bits}_strip_none"]["ms_per_launch"], 3)
                doc["launches"][f"b{bits}_none_{tw}x{tl}"] = r
                print(f"launch b{bits}_none_{tw}x{tl}: {r['ms_per_launch']} ms, {r['ratio_to_strip_finish']} x the strip launch", file=sys.stderr, flush=True)
                for p in paths:
                    os.remove(p)
        cases = [(8, tw, tl, c) for tw, tl in sizes for c in ("lzw", "deflate")] + [(16,) + size16 + (c,) for c in ("lzw", "deflate")]
        for bits, tw, tl, codec in cases:
            name = f"b{bits}_{codec}_{tw}x{tl}"
            two = files_of(bits, tw, tl, codec)
            r = launch_ms(det, [open(p, "rb").read() for p in two], [source[bits, 1], source[bits, 2]], frames, tiles=True)
            r[codec + "_launch_ms_by_difference"] = round(r["ms_per_launch"] - doc["launches"][f"b{bits}_none_{tw}x{tl}"]["ms_per_launch"], 3) \
                if f"b{bits}_none_{tw}x{tl}" in doc["launches"] else None
            doc["launches"][name] = r
            print(f"launch {name}: {r['ms_per_launch']} ms per {frames} frames", file=sys.stderr, flush=True)
            paths = [two[i % 2] for i in range(frames)]
            deflate = codec == "deflate"
            legs = {"device": 1 << 20, "host_forced": 1}
            walls = {leg: [] for leg in legs}
            det.set_option("tiff_deflate_max_strip", 1 << 20)
            for k in range(rounds + 1):               # (round 0 warms the staging up and is dropped)
                for leg, max_strip in legs.items():
                    if not deflate:
                        det.set_option("tiff_lzw_max_strip", max_strip)
                    t0 = time.perf_counter()
                    fr, status = det.read_tiffs(paths, nthreads=jobs, deflate="device" if deflate and leg == "device" else "host")
                    wall = time.perf_counter() - t0
                    assert not status.any() and np.array_equal(fr[1].cpu().numpy(), source[bits, 2])
                    del fr
                    if k:
                        walls[leg].append(wall)
            det.set_option("tiff_lzw_max_strip", 64 << 10)
            det.set_option("tiff_deflate_max_strip", 8 << 10)
            doc["loader"][name] = {leg: {"frames_per_s": round(frames / statistics.median(w), 1),
                                         "frames_per_s_rounds": [round(frames / v, 1) for v in w]} for leg, w in walls.items()}
            doc["loader"][name]["device_wins_every_round"] = min(walls["host_forced"]) > max(walls["device"])
            print(f"loader {name}: {doc['loader'][name]}", file=sys.stderr, flush=True)
            for p in two:
                os.remove(p)
    finally:
        det.close()
        shutil.rmtree(scratch, ignore_errors=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


def main(args):
    if "--tile" in args:
        return main_tiled(args)
    import torch
    import mrgingham_amd
    from mrgingham_amd import _lib
    rounds, jobs, frames = int(opts(args, "--rounds", "3")), int(opts(args, "--jobs", "16")), int(opts(args, "--frames", "64"))
    codecs = {"lzw": ["lzw"], "deflate": ["deflate"], "both": ["lzw", "deflate"]}[opts(args, "--codec", "lzw")]
    out_path = opts(args, "--out", os.path.join(ROOT, "profiles", "tiff_deflate_bench.json" if codecs == ["deflate"] else "tiff_bench.json"))
    cases = [(8, f"{c}_rows{r}") for c in codecs for r in (2, 16, 256)] + [(8, "none")] + [(16, f"{c}_rows2") for c in codecs] + [(16, "none")]
    doc = {"device": torch.cuda.get_device_name(0), "jobs": jobs, "rounds": rounds, "frames": frames, "frame": [W, H],
           "hbm_peak_bytes_per_s": HBM_PEAK, "geometry_lanes_segment_step": list(mrgingham_amd.tiff_geometry()), "codecs": codecs,
           "inflate_lanes": _lib.lib().mrgingham_amd_tiff_inflate_lanes()}
    scratch = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    det = mrgingham_amd.Detector(0)
    try:
        files, source = write_files(scratch, codecs)
        doc["launches"] = {}
        for bits, name in cases:
            datas = [open(files[bits, name, seed], "rb").read() for seed in (1, 2)]
            r = launch_ms(det, datas, [source[bits, 1], source[bits, 2]], frames)
            if name == "none":
                finish_rate(r)
            doc["launches"][f"b{bits}_{name}"] = r
            print(f"launch b{bits}_{name}: {r['ms_per_launch']} ms per {frames} frames", file=sys.stderr, flush=True)
        for bits, name in cases:      # the check and the finish kernel run on the uncompressed pixels too: the rest is the strip launch
            if name != "none":
                r, no = doc["launches"][f"b{bits}_{name}"], doc["launches"][f"b{bits}_none"]
                r[name.split("_")[0] + "_launch_ms_by_difference"] = round(r["ms_per_launch"] - no["ms_per_launch"], 3)
        doc["loader"] = {}
        for bits, name in cases:
            paths = [files[bits, name, 1 + i % 2] for i in range(frames)]
            deflate = name.startswith("deflate")
            legs = {"device": 1 << 20} if name == "none" else {"device": 1 << 20, "host_forced": 1}
            walls = {leg: [] for leg in legs}
            det.set_option("tiff_deflate_max_strip", 1 << 20)
            for r in range(rounds + 1):               # (round 0 warms the staging up and is dropped)
                for leg, max_strip in legs.items():
                    if not deflate:
                        det.set_option("tiff_lzw_max_strip", max_strip)
                    t0 = time.perf_counter()
                    fr, status = det.read_tiffs(paths, nthreads=jobs, deflate="device" if deflate and leg == "device" else "host")
                    wall = time.perf_counter() - t0
                    assert not status.any() and np.array_equal(fr[1].cpu().numpy(), source[bits, 2])
                    del fr
                    if r:
                        walls[leg].append(wall)
            det.set_option("tiff_lzw_max_strip", 64 << 10)
            det.set_option("tiff_deflate_max_strip", 8 << 10)
            doc["loader"][f"b{bits}_{name}"] = {leg: {"frames_per_s": round(frames / statistics.median(w), 1),
                                                      "frames_per_s_rounds": [round(frames / v, 1) for v in w]} for leg, w in walls.items()}
            print(f"loader b{bits}_{name}: {doc['loader'][f'b{bits}_{name}']}", file=sys.stderr, flush=True)
    finally:
        det.close()
        shutil.rmtree(scratch, ignore_errors=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
