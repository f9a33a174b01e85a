"""Windows Bitmap files into device frames (Detector.bmp_unpack, Detector.read_bmps) and through find_boards_files
(bmp="device", the tool's --bmp-unpack device).  The kernel runs the pixel text of the host decoder (csrc/bmp_pixels.h), so
the yardstick is read_image on the same file, byte for byte; for the route it is the PGM of the same board.  No tolerance
anywhere.

The shapes sit where the kernel can go wrong: a destination word begins at any byte phase, so a word's first pixel is no
multiple of 16 and, at 1 and 4 bits, lies inside a source byte; widths around 8, 16, 32 and 64 pixels; rows whose padded
length is no multiple of 16.  Nothing but the row-slot case is larger than 640 x 480."""
import os

import numpy as np
import pytest

import mrgingham_amd
from tests import bmp_cases as bc
from tests import files_cases
from tests.test_gpu_files import CLI, STATS, parse_vnlog, run_child, run_tool

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 7, 8, 15, 16, 17, 31, 33, 64, 65, 130)
HEIGHTS = (1, 2, 5)
# (bits, identity: the palette is the grey ramp and the launch takes no table)
VARIANTS = [(1, False), (4, False), (8, True), (8, False), (24, False), (32, False)]
VARIANT_IDS = ["1bit", "4bit", "8bit_identity", "8bit_palette", "24bit", "32bit"]


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector()
    yield d
    d.close()


def _case(B, h, w, bits, identity, top_down, seed, tmp_path=None):
    """B files of one kind -> (payload uint8 [B, P] with P beyond the pixel array, lut uint8 [B, 256] or None, the grey
    frames [B, h, w]); with tmp_path, frame 0 is what read_image gives for the file"""
    rowb = bc.row_bytes(w, bits)
    pitch = (rowb * h + 15) // 16 * 16 + 16
    pay = np.full((B, pitch), 0xEE, np.uint8)                      # (what lies behind a pixel array is never a sample)
    lut = np.zeros((B, 256), np.uint8)
    want = np.zeros((B, h, w), np.uint8)
    for f in range(B):
        pix = bc.random_pixels(w, h, bits, seed=seed + f)
        pal = None if bits > 8 else bc.grey_ramp() if identity else bc.random_palette(1 << bits, seed + f)
        rows = bc.pack_rows(pix, bits)
        pay[f, :rowb * h] = (rows if top_down else rows[::-1]).reshape(-1)
        want[f] = bc.expected(pix, bits, pal)
        if bits <= 8:
            lut[f, :len(pal)] = bc.grey(pal[:, 0], pal[:, 1], pal[:, 2])
        if f == 0 and tmp_path is not None:
            path = str(tmp_path / "case.bmp")
            data = bc.write(pix, bits, pal, top_down=top_down)
            with open(path, "wb") as fh:
                fh.write(data)
            lay = mrgingham_amd.bmp_layout(data)
            assert lay.taken and lay.lut_identity == int(identity) and (bits > 8 or np.array_equal(lay.lut, lut[0]))
            assert data[lay.payload_offset:lay.payload_offset + rowb * h] == pay[0, :rowb * h].tobytes()
            assert np.array_equal(mrgingham_amd.read_image(path), want[0])
    return pay, (None if identity or bits > 8 else lut), want


def _unpack(det, pay, lut, h, w, bits, top_down, out=None):
    import torch
    got = det.bmp_unpack(torch.from_numpy(pay).cuda(), None if lut is None else torch.from_numpy(lut).cuda(), h, w, bits,
                         top_down=top_down, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("top_down", [False, True], ids=["bottom_up", "top_down"])
@pytest.mark.parametrize("bits,identity", VARIANTS, ids=VARIANT_IDS)
def test_unpack_equals_the_host_decoder(det, tmp_path, bits, identity, top_down):
    """three frames per call, a payload pitch beyond the array and a stride beyond the width: the bytes between width and
    stride, and the rows behind every frame, keep their sentinel"""
    import torch
    for h in HEIGHTS:
        for w in WIDTHS:
            pay, lut, want = _case(3, h, w, bits, identity, top_down, seed=1000 * bits + 10 * w + h, tmp_path=tmp_path)
            big = torch.full((3, h + 1, w + 5), 0xA5, dtype=torch.uint8, device="cuda")
            got = _unpack(det, pay, lut, h, w, bits, top_down, out=big[:, :h, :])
            assert got.shape == (3, h, w) and np.array_equal(got, want), (w, h)
            back = big.cpu().numpy()
            assert np.array_equal(back[:, :h, :w], want) and (back[:, :h, w:] == 0xA5).all() and (back[:, h:, :] == 0xA5).all(), (w, h)
    # a dense output of the library's own
    pay, lut, want = _case(2, 5, 33, bits, identity, top_down, seed=bits)
    assert np.array_equal(_unpack(det, pay, lut, 5, 33, bits, top_down), want)


@pytest.mark.parametrize("bits,identity", VARIANTS, ids=VARIANT_IDS)
def test_every_destination_phase(det, bits, identity):
    """d_out at every byte phase of a 16-byte word, dense frames of odd width: the rows begin at every phase as well; a
    word's first pixel is 16k - phase, inside a source byte at 1 and 4 bits"""
    import torch
    for w in (17, 33):
        h = 5
        pay, lut, want = _case(3, h, w, bits, identity, False, seed=bits + w)
        d_pay = torch.from_numpy(pay).cuda()
        d_lut = None if lut is None else torch.from_numpy(lut).cuda()
        n = 3 * h * w
        for phase in range(16):
            flat = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            at = (phase - flat.data_ptr()) % 16 + 16
            out = flat[at:at + n].view(3, h, w)
            assert out.data_ptr() % 16 == phase
            det.bmp_unpack(d_pay, d_lut, h, w, bits, out=out)
            torch.cuda.synchronize()
            back = flat.cpu().numpy()
            assert np.array_equal(back[at:at + n].reshape(3, h, w), want), (w, phase)
            assert (back[:at] == 0x5A).all() and (back[at + n:] == 0x5A).all(), (w, phase)


def test_more_rows_than_the_launch_has_row_slots(det):
    """The grid is capped at max_workgroups_per_cu workgroups per CU and the kernel loops over the rows beyond: frames of
    1 x 32767 pixels, a row two lanes (one word, and one more where a row can begin inside a word), the smallest frame
    count above one trip."""
    import torch
    lanes, per_cu = mrgingham_amd.bmp_unpack_geometry()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slots = cus * per_cu * (lanes // 2)
    h = 32767
    B = slots // h + 1
    assert slots < B * h < 2 * slots and B * h * 4 < 16 << 20
    pay, lut, want = _case(B, h, 1, 8, False, False, seed=5)
    got = _unpack(det, pay, lut, h, 1, 8, False)
    assert got.shape == (B, h, 1) and np.array_equal(got, want)
    assert lut is not None and len(np.unique(want)) > 200


def _numpy_grey(raw, w, bits, lut):
    """rows of a pixel array, uint8 [rows, row_bytes] -> grey [rows, w]: the host decoder's arithmetic on whole arrays"""
    if bits == 8:
        return raw[:, :w] if lut is None else lut[raw[:, :w]]
    if bits == 1:
        return lut[np.unpackbits(raw, axis=1)[:, :w]]
    if bits == 4:
        return lut[np.stack([raw >> 4, raw & 15], axis=-1).reshape(len(raw), -1)[:, :w]]
    px = raw[:, :w * bits // 8].reshape(len(raw), w, bits // 8)
    return bc.grey(px[..., 2], px[..., 1], px[..., 0]).astype(np.uint8)


@pytest.mark.parametrize("bits,identity", VARIANTS, ids=VARIANT_IDS)
def test_full_width_rows_with_every_cu_full(det, bits, identity):
    """4096 pixels: a row takes the 256 lanes of a workgroup, a workgroup one row, and with more rows than the launch has
    workgroups every CU holds as many as it can and the kernel takes a second, ragged trip.  (The 8-bit launch without a
    table once gave wrong dwords at exactly this shape, and at no smaller one.)"""
    import torch
    lanes, per_cu = mrgingham_amd.bmp_unpack_geometry()
    w, h = 16 * lanes, torch.cuda.get_device_properties(0).multi_processor_count * per_cu + 37
    rowb = bc.row_bytes(w, bits)
    rng = np.random.default_rng(bits)
    raw = rng.integers(0, 256, (h, rowb), dtype=np.uint8)
    lut = None if identity or bits > 8 else rng.integers(0, 256, 256, dtype=np.uint8)
    want = _numpy_grey(raw, w, bits, lut)[::-1]
    got = _unpack(det, raw.reshape(1, -1), None if lut is None else lut.reshape(1, 256), h, w, bits, False)
    assert got.shape == (1, h, w) and np.array_equal(got[0], want)


def test_every_colour_channel_reaches_the_weights(det):
    """(a wrong byte order cannot hide: pure red, green and blue read 76, 150 and 29)"""
    pix = np.zeros((1, 16, 3), np.uint8)
    pix[0, 0::3, 0], pix[0, 1::3, 1], pix[0, 2::3, 2] = 255, 255, 255
    want = bc.expected(pix, 24)
    assert want[0, :3].tolist() == [76, 150, 29]
    for bits in (24, 32):
        px = pix if bits == 24 else np.concatenate([pix, np.full((1, 16, 1), 0xC3, np.uint8)], axis=-1)
        rows = bc.pack_rows(px, bits)
        pay = np.zeros((1, (rows.size + 15) // 16 * 16), np.uint8)
        pay[0, :rows.size] = rows.reshape(-1)
        assert np.array_equal(_unpack(det, pay, None, 1, 16, bits, False)[0], want)


def test_no_frames_and_bad_arguments_write_nothing(det):
    import torch
    h, w, bits = 5, 9, 4
    pay, lut, want = _case(1, h, w, bits, False, False, seed=3)
    d_pay, d_lut = torch.from_numpy(pay).cuda(), torch.from_numpy(lut).cuda()
    out = torch.full((h * w + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    pitch = pay.shape[1]
    assert tuple(det.bmp_unpack(d_pay[:0], d_lut[:0], h, w, bits).shape) == (0, h, w)

    def call(d_payload=None, payload_pitch=pitch, lut_ptr=-1, n=1, width=w, height=h, bits=bits, top_down=0, identity=0, d_out=None,
             frame_pitch=w * h, stride=w, ctx=-1):
        return det.L.mrgingham_amd_bmp_unpack_batch(det.ctx if ctx == -1 else ctx, d_pay.data_ptr() if d_payload is None else d_payload,
                                                    payload_pitch, d_lut.data_ptr() if lut_ptr == -1 else lut_ptr, n, width, height, bits,
                                                    top_down, identity, out.data_ptr() if d_out is None else d_out, frame_pitch, stride, None)
    need = bc.row_bytes(w, bits) * h
    bad = [dict(n=-1), dict(width=-1), dict(height=-1), dict(stride=w - 1), dict(frame_pitch=-1), dict(payload_pitch=-16),
           dict(payload_pitch=need // 16 * 16 - 16), dict(payload_pitch=pitch + 8), dict(bits=0), dict(bits=2), dict(bits=12), dict(bits=16),
           dict(bits=64), dict(d_payload=d_pay.data_ptr() + 4), dict(d_payload=d_pay.data_ptr() + 8), dict(d_payload=0), dict(d_out=0),
           dict(lut_ptr=None), dict(lut_ptr=None, identity=1), dict(bits=8, lut_ptr=None, payload_pitch=1 << 20),
           dict(width=32768, stride=32768, payload_pitch=1 << 40), dict(height=32768, payload_pitch=1 << 40), dict(ctx=None)]
    assert need < pitch and need // 16 * 16 - 16 < need
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(n=0) == 0 and call(width=0, stride=0) == 0 and call(height=0) == 0               # nothing to do is not an error
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A).all()
    assert call() == 0
    torch.cuda.synchronize()
    back = out.cpu().numpy()
    assert np.array_equal(back[:h * w].reshape(h, w), want[0]) and (back[h * w:] == 0x5A).all()


# ---- read_bmps --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bmp_list(tmp_path_factory):
    """(names, statuses): files of 65 x 7 of every depth and both row orders, and in between one file of every way to fail"""
    d = str(tmp_path_factory.mktemp("bmps"))
    w, h = 65, 7

    def put(name, data):
        path = os.path.join(d, name)
        with open(path, "wb") as f:
            f.write(data)
        return path
    pal256 = bc.random_palette(256, seed=1)
    grey8 = put("grey8.bmp", bc.write(bc.random_pixels(w, h, 8, seed=2), 8, bc.grey_ramp()))
    grey8_td = put("grey8_td.bmp", bc.write(bc.random_pixels(w, h, 8, seed=3), 8, bc.grey_ramp(), top_down=True))
    pal8 = put("pal8.bmp", bc.write(bc.random_pixels(w, h, 8, seed=4), 8, pal256, header=108))
    pal8_short = put("pal8_short.bmp", bc.write(bc.random_pixels(w, h, 8, seed=5), 8, bc.random_palette(100, seed=6), gap=5))
    rgb = put("rgb.bmp", bc.write(bc.random_pixels(w, h, 24, seed=7), 24))
    rgb_td = put("rgb_td.bmp", bc.write(bc.random_pixels(w, h, 24, seed=8), 24, top_down=True, header=124))
    rgbx = put("rgbx.bmp", bc.write(bc.random_pixels(w, h, 32, seed=9), 32, bitfields=True))
    one = put("one.bmp", bc.write(bc.random_pixels(w, h, 1, seed=10), 1, bc.random_palette(2, seed=11)))
    four_td = put("four_td.bmp", bc.write(bc.random_pixels(w, h, 4, seed=12), 4, bc.random_palette(16, seed=13), top_down=True))
    rle = put("rle8.bmp", bc.write_rle8(w, h, bc.rle8_encode(bc.random_pixels(w, h, 8, seed=14, top=3)), pal256))
    small = put("small.bmp", bc.write(bc.random_pixels(33, h, 8, seed=15), 8, bc.grey_ramp()))
    short = put("short.bmp", open(rgb, "rb").read()[:-1])
    rle_cut = put("rle8_cut.bmp", bc.write_rle8(w, h, bc.rle8_encode(bc.random_pixels(w, h, 8, seed=16))[:40], pal256))
    pgm = os.path.join(d, "grey.pgm")
    files_cases.write_pgm(pgm, bc.random_pixels(w, h, 8, seed=17))
    missing = os.path.join(d, "missing.bmp")
    names = [grey8, grey8, grey8_td, missing, pal8, pal8_short, small, rgb, rgb_td, short, rgbx, rle, one, one, pgm, four_td, rle_cut, grey8]
    status = [0, 0, 0, -1, 0, 0, -2, 0, 0, -1, 0, 0, 0, 0, -1, 0, -1, 0]
    return names, status


@pytest.mark.parametrize("chunk,unpack,nthreads", [(1, 1, 4), (2, 1, 0), (0, 1, 1), (0, 0, 4), (3, 0, 2)],
                         ids=["chunks_of_1", "chunks_of_2", "one_chunk", "host_decoded", "host_decoded_chunks_of_3"])
def test_read_bmps(det, bmp_list, chunk, unpack, nthreads):
    names, want_status = bmp_list
    det.set_option("bmp_chunk_frames", chunk)
    det.set_option("bmp_unpack", unpack)
    try:
        frames, status = det.read_bmps(names, nthreads=nthreads)
    finally:
        det.set_option("bmp_chunk_frames", 0)
        det.set_option("bmp_unpack", 1)
    assert status.tolist() == want_status
    got = frames.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (len(names), 7, 65)
    for f, name in enumerate(names):
        img = mrgingham_amd.read_image(name)
        if want_status[f] == 0:
            assert np.array_equal(got[f], img), name
        else:
            if name.endswith(".bmp"):                         # (-1: what read_image cannot read either; -2: what it can)
                assert (img is None) == (want_status[f] == -1), name
            assert not got[f].any(), name
    assert sum(1 for s in want_status if s == 0) == 13


def test_read_bmps_without_a_readable_header(det, bmp_list):
    names, _ = bmp_list
    frames, status = det.read_bmps([names[3], names[14]])
    assert tuple(frames.shape) == (2, 0, 0) and status.tolist() == [-1, -1]
    frames, status = det.read_bmps([])
    assert tuple(frames.shape) == (0, 0, 0) and len(status) == 0
    with pytest.raises(ValueError):
        det.set_option("bmp_unpack", 2)


# ---- find_boards_files(bmp=...) and the tool ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def board_files(tmp_path_factory):
    """the 640 x 480 board as PGM, 8-bit BMP (grey ramp; bottom-up and top-down), 24-bit BMP (r = g = b) and RLE8 BMP"""
    d = str(tmp_path_factory.mktemp("boards"))
    board = files_cases.board_pixels()
    f = {"board.pgm": os.path.join(d, "board.pgm")}
    files_cases.write_pgm(f["board.pgm"], board)
    datas = {"board8.bmp": bc.write(board, 8, bc.grey_ramp()), "board8_td.bmp": bc.write(board, 8, bc.grey_ramp(), top_down=True),
             "board24.bmp": bc.write(np.stack([board] * 3, axis=-1), 24),
             "board_rle8.bmp": bc.write_rle8(640, 480, bc.rle8_encode(board), bc.grey_ramp())}
    for name, data in datas.items():
        f[name] = os.path.join(d, name)
        with open(f[name], "wb") as fh:
            fh.write(data)
    f["missing"] = os.path.join(d, "missing.bmp")
    f["cut.bmp"] = os.path.join(d, "cut.bmp")
    with open(f["cut.bmp"], "wb") as fh:
        fh.write(datas["board24.bmp"][:-1])
    paths = [f["board.pgm"], f["board8.bmp"], f["board24.bmp"], f["board_rle8.bmp"], f["missing"], f["board8_td.bmp"], f["board8.bmp"],
             f["cut.bmp"], f["board24.bmp"]]
    return f, paths


RUNS = [(bmp, batch) for bmp in ("host", "device") for batch in (1, 4, 64)]


@pytest.fixture(scope="module")
def board_runs(board_files, tmp_path_factory):
    _, paths = board_files
    runs = [{"id": f"{bmp}_b{batch}", "paths": paths, "kw": {"batch": batch, "nthreads": 4, "bmp": bmp}, "ref": batch == 4} for bmp, batch in RUNS]
    return run_child(str(tmp_path_factory.mktemp("board_runs")), {"runs": runs})


@pytest.mark.parametrize("bmp,batch", RUNS, ids=[f"{b}_b{n}" for b, n in RUNS])
def test_files_give_the_boards_of_the_pgm(board_files, board_runs, bmp, batch):
    f, paths = board_files
    out, rid, n = board_runs, f"{bmp}_b{batch}", len(paths)
    status, found, boards, levels = (out[f"{rid}_{k}"] for k in ("status", "found", "boards", "levels"))
    bad = [paths.index(f["missing"]), paths.index(f["cut.bmp"])]
    assert len(status) == n and np.flatnonzero(status != 0).tolist() == bad
    assert found[0] >= 0 and not np.isnan(boards[0]).any()                       # (the PGM bears a board)
    for i in range(1, n):
        if i not in bad:                                                          # the PGM's numbers, double for double
            assert found[i] == found[0] and np.array_equal(boards[i], boards[0]) and np.array_equal(levels[i], levels[0]), paths[i]
    if batch == 4:
        for what in ("status", "found", "levels"):
            assert np.array_equal(out[f"{rid}_{what}"], out[f"{rid}_ref_{what}"]), what
        assert np.array_equal(boards, out[f"{rid}_ref_boards"], equal_nan=True)
    nfinal = out[rid + "_nfinal"]
    assert len(nfinal) >= 1 and (np.diff(nfinal) >= 0).all() and nfinal[-1] == n and out[rid + "_snap_ok"].all()
    stats = dict(zip(STATS, out[rid + "_stats"]))
    assert stats["files_device_loader"] + stats["files_host_decoded"] + stats["files_one_image"] + stats["files_unreadable"] == n
    assert stats["files_unreadable"] == 2 and stats["files_one_image"] == 0
    nbmp = sum(1 for i, p in enumerate(paths) if p.endswith(".bmp") and i not in bad)
    assert nbmp == 6
    assert stats["files_device_loader"] == (nbmp if bmp == "device" else 0)       # (the RLE8 file is a slot of a BMP run)
    assert stats["files_host_decoded"] == (1 if bmp == "device" else 1 + nbmp)


def test_tool_bmp_unpack_device_prints_the_same_vnlog(board_files):
    f, paths = board_files
    readable = [p for p in dict.fromkeys(paths) if "missing" not in p and "cut" not in p]
    plain = run_tool("--jobs", "2", *readable)
    host = run_tool("--jobs", "4", "--batch", "4", *readable)
    device = run_tool("--jobs", "4", "--batch", "4", "--bmp-unpack", "device", *readable)
    assert plain.returncode == 0 and host.returncode == 0 and device.returncode == 0, plain.stderr + host.stderr + device.stderr
    order, records, comments = parse_vnlog(device.stdout)
    assert (order, records) == parse_vnlog(host.stdout)[:2]          # (the comments name the command line)
    assert records == parse_vnlog(plain.stdout)[1]
    assert comments[-1] == "# filename x y level"
    assert order == readable and all(len(records[p]) == 100 for p in readable) and os.access(CLI, os.X_OK)
    want = [line.split(" ", 1)[1] for line in records[f["board.pgm"]]]
    for p in readable:
        assert [line.split(" ", 1)[1] for line in records[p]] == want, p
    r = run_tool("--bmp-unpack", "device", readable[0])
    assert r.returncode != 0 and "--bmp-unpack is only accepted with --batch" in r.stderr
    r = run_tool("--batch", "2", "--bmp-unpack", "both", readable[0])
    assert r.returncode != 0 and "--bmp-unpack takes 'host' or 'device', got 'both'" in r.stderr
    assert "--bmp-unpack host|device" in run_tool("--help").stdout
