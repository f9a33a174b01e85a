"""Binary PBM and PAM files into device frames (Detector.pnm_unpack, Detector.read_pnms) and through find_boards_files
(pnm="device", the tool's --pnm-unpack device).  The kernel runs the pixel text of the host decoder (csrc/pnm_pixels.h); the
yardstick is the array a file was written from through the grey weights (tests/pnm_cases.py) -- which is what read_image
gives, at 16 bits its high byte --, for the route the PGM of the same board.  np.array_equal everywhere, no tolerance.

The shapes sit where the kernel can go wrong: a Netpbm row begins at any byte of the raster and a destination word at any
byte phase, so a word's first pixel is no multiple of 16 and, at P4, lies inside a source byte.  Nothing but the row-slot
and the full-width cases is larger than 640 x 480."""
import os

import numpy as np
import pytest

import mrgingham_amd
from tests import files_cases
from tests import pnm_cases as pc
from tests.test_gpu_files import CLI, STATS, parse_vnlog, run_child, run_tool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector()
    yield d
    d.close()


def _case(B, h, w, layout, seed, tmp_path=None):
    """B rasters of one layout -> (payload uint8 [B, P] with P beyond the raster, the grey frames [B, h, w]); with tmp_path
    frame 0 is checked against read_image on the file"""
    _, magic, bits, ch, bw = layout
    need = pc.row_bytes(w, bits, ch) * h
    pitch = (need + 15) // 16 * 16 + 16
    pay = np.full((B, pitch), 0xEE, np.uint8)                      # (what lies behind a raster is never a sample)
    want = np.zeros((B, h, w), np.uint16 if bits == 16 else np.uint8)
    for f in range(B):
        s = pc.random_samples(w, h, bits, ch, bw, seed=seed + f)
        pay[f, :need] = np.frombuffer(pc.raster(s, bits), np.uint8)
        want[f] = pc.expected(s, bits, ch, bw)
        if f == 0 and tmp_path is not None:
            path = str(tmp_path / "case.pnm")
            data = pc.write(s, magic, bits, bw)
            with open(path, "wb") as fh:
                fh.write(data)
            head = mrgingham_amd.pnm_header(data)
            assert (head.bits, head.channels, head.black_and_white, head.row_bytes * h) == (bits, ch, int(bw), need)
            assert data[head.payload_offset:] == pay[0, :need].tobytes()
            assert np.array_equal(mrgingham_amd.read_image(path), want[0] if bits < 16 else (want[0] >> 8).astype(np.uint8))
    return pay, want


def _unpack(det, pay, h, w, layout, out=None):
    import torch
    _, _, bits, ch, bw = layout
    got = det.pnm_unpack(torch.from_numpy(pay).cuda(), h, w, bits, ch, black_and_white=bw, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("layout", pc.LAYOUTS, ids=pc.LAYOUT_IDS)
def test_unpack_equals_the_host_decoder(det, tmp_path, layout):
    """2 frames of 5 x 33, dense; then three frames per call at widths around the word sizes with a payload pitch beyond the
    raster and a stride beyond the width: the samples between width and stride, and the rows behind every frame, keep
    their sentinel"""
    import torch
    pay, want = _case(2, 5, 33, layout, seed=layout[2], tmp_path=tmp_path)
    got = _unpack(det, pay, 5, 33, layout)
    assert got.dtype == want.dtype and got.shape == (2, 5, 33) and np.array_equal(got, want)
    for h in (1, 2, 5):
        for w in (1, 3, 7, 8, 9, 15, 16, 17, 31, 33, 64, 65, 130):
            pay, want = _case(3, h, w, layout, seed=1000 * layout[2] + 10 * w + h)
            es = want.dtype.itemsize
            big = torch.full((3, h + 1, (w + 5) * es), 0xA5, dtype=torch.uint8, device="cuda")
            if es == 2:
                big = big.view(torch.uint16)
            guard = 0xA5 if es == 1 else 0xA5A5
            got = _unpack(det, pay, h, w, layout, out=big[:, :h, :])
            assert got.shape == (3, h, w) and np.array_equal(got, want), (w, h)
            back = big.cpu().numpy()
            assert np.array_equal(back[:, :h, :w], want) and (back[:, :h, w:] == guard).all() and (back[:, h:, :] == guard).all(), (w, h)


@pytest.mark.parametrize("layout", pc.LAYOUTS, ids=pc.LAYOUT_IDS)
def test_every_destination_phase(det, layout):
    """d_out at every byte phase of a 16-byte word (every even one at 16 bits), dense frames of odd width: the destination
    rows begin at every phase as well, and so do the source rows; guard bytes in front of and behind the frames stay"""
    import torch
    bits = layout[2]
    es = 2 if bits == 16 else 1
    for w in ((9, 17) if es == 2 else (17, 33)):
        h = 5
        pay, want = _case(3, h, w, layout, seed=bits + w)
        d_pay = torch.from_numpy(pay).cuda()
        n = 3 * h * w * es
        for phase in range(0, 16, es):
            flat = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            at = (phase - flat.data_ptr()) % 16 + 16
            out = flat[at:at + n]
            out = (out.view(torch.uint16) if es == 2 else out).view(3, h, w)
            assert out.data_ptr() % 16 == phase
            det.pnm_unpack(d_pay, h, w, bits, layout[3], black_and_white=layout[4], out=out)
            torch.cuda.synchronize()
            back = flat.cpu().numpy()
            assert np.array_equal(back[at:at + n].view(want.dtype).reshape(3, h, w), want), (w, phase)
            assert (back[:at] == 0x5A).all() and (back[at + n:] == 0x5A).all(), (w, phase)


@pytest.mark.parametrize("layout", pc.LAYOUTS, ids=pc.LAYOUT_IDS)
def test_more_rows_than_the_launch_has_row_slots(det, layout):
    """The grid is capped at max_workgroups_per_cu workgroups per CU and the kernel loops over the rows beyond: frames of
    1 x 32767 pixels, a row two lanes (one word, and one more where a row can begin inside a word), the smallest frame
    count above one trip."""
    import torch
    lanes, per_cu = mrgingham_amd.pnm_unpack_geometry()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slots = cus * per_cu * (lanes // 2)
    h = 32767
    B = slots // h + 1
    assert slots < B * h < 2 * slots and B * h * 8 < 16 << 20
    pay, want = _case(B, h, 1, layout, seed=5)
    got = _unpack(det, pay, h, 1, layout)
    assert got.shape == (B, h, 1) and np.array_equal(got, want) and len(np.unique(want)) >= 2


def _numpy_grey(raw, w, layout):
    """rows of a raster, uint8 [rows, row_bytes] -> grey [rows, w]: the host decoder's arithmetic on whole arrays"""
    _, _, bits, ch, bw = layout
    if bits == 1:
        return np.where(np.unpackbits(raw, axis=1)[:, :w] != 0, 0, 255).astype(np.uint8)
    s = raw.reshape(len(raw), w, ch) if bits == 8 else raw.view(">u2").reshape(len(raw), w, ch)
    return pc.expected(s, bits, ch, bw)


@pytest.mark.parametrize("layout", pc.LAYOUTS, ids=pc.LAYOUT_IDS)
def test_full_width_rows_with_every_cu_full(det, layout):
    """A row takes the 256 lanes of a workgroup, a workgroup one row, and with more rows than the launch has workgroups
    every CU holds as many as it can and the kernel takes a second, ragged trip.  (The BMP kernel's first form gave wrong
    dwords at exactly this shape, and at no smaller one.)"""
    import torch
    _, _, bits, ch, bw = layout
    lanes, per_cu = mrgingham_amd.pnm_unpack_geometry()
    w = (8 if bits == 16 else 16) * lanes
    h = torch.cuda.get_device_properties(0).multi_processor_count * per_cu + 37
    rowb = pc.row_bytes(w, bits, ch)
    raw = np.random.default_rng(bits + ch).integers(0, 256, (h, rowb), dtype=np.uint8)
    want = _numpy_grey(raw, w, layout)
    got = _unpack(det, raw.reshape(1, -1), h, w, layout)
    assert got.shape == (1, h, w) and got.dtype == want.dtype and np.array_equal(got[0], want)


def test_every_colour_channel_reaches_the_weights(det):
    """(a swapped channel order cannot hide: pure red, green and blue read 76, 150 and 29, and the formula's values at 16 bits)"""
    for bits, top in ((8, 255), (16, 65535)):
        s = np.zeros((1, 16, 3), np.uint16 if bits == 16 else np.uint8)
        s[0, 0::3, 0], s[0, 1::3, 1], s[0, 2::3, 2] = top, top, top
        want = pc.expected(s, bits, 3)
        assert want[0, :3].tolist() == ([76, 150, 29] if bits == 8 else [int(pc.grey(top, 0, 0)), int(pc.grey(0, top, 0)), int(pc.grey(0, 0, top))])
        assert bits == 8 or want[0, :3].tolist() == [19596, 38467, 7472]
        for ch in (3, 4):
            px = s if ch == 3 else np.concatenate([s, np.full((1, 16, 1), top - 60, s.dtype)], axis=-1)
            body = np.frombuffer(pc.raster(px, bits), np.uint8)
            pay = np.zeros((1, (body.size + 15) // 16 * 16), np.uint8)
            pay[0, :body.size] = body
            assert np.array_equal(_unpack(det, pay, 1, 16, ("", 7, bits, ch, False))[0], want), (bits, ch)


def test_no_frames_and_bad_arguments_write_nothing(det):
    import torch
    h, w = 5, 9
    layout = pc.LAYOUTS[3]                                      # P7 RGB, 8 bits
    assert layout[0] == "p7_rgb8"
    pay, want = _case(1, h, w, layout, seed=3)
    d_pay = torch.from_numpy(pay).cuda()
    out = torch.full((h * w + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    pitch = pay.shape[1]
    assert tuple(det.pnm_unpack(d_pay[:0], h, w, 8, 3).shape) == (0, h, w)

    def call(d_payload=None, payload_pitch=pitch, n=1, width=w, height=h, bits=8, channels=3, bw=0, d_out=None, frame_pitch=w * h, stride=w,
             ctx=-1):
        return det.L.mrgingham_amd_pnm_unpack_batch(det.ctx if ctx == -1 else ctx, d_pay.data_ptr() if d_payload is None else d_payload,
                                                    payload_pitch, n, width, height, bits, channels, bw,
                                                    out.data_ptr() if d_out is None else d_out, frame_pitch, stride, None)
    need = 3 * w * h
    bad = [dict(n=-1), dict(width=-1), dict(height=-1), dict(stride=w - 1), dict(frame_pitch=-1), dict(payload_pitch=-16),
           dict(payload_pitch=need // 16 * 16 - 16), dict(payload_pitch=pitch + 8), dict(bits=0), dict(bits=2), dict(bits=4), dict(bits=24),
           dict(bits=32), dict(channels=0), dict(channels=5), dict(channels=-1), dict(bits=1), dict(bits=1, channels=1, bw=1),
           dict(bw=1), dict(bits=16, channels=1, bw=1, payload_pitch=1 << 20), dict(channels=4), dict(bits=16),
           dict(bits=16, channels=1, d_out=out.data_ptr() + 1), dict(d_payload=d_pay.data_ptr() + 4), dict(d_payload=d_pay.data_ptr() + 8),
           dict(d_payload=0), dict(d_out=0), dict(width=32768, stride=32768, payload_pitch=1 << 40),
           dict(height=32768, payload_pitch=1 << 40), dict(ctx=None)]
    assert need < pitch and need // 16 * 16 - 16 < need and 4 * w * h > pitch and out.data_ptr() % 2 == 0
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(n=0) == 0 and call(width=0, stride=0) == 0 and call(height=0) == 0               # nothing to do is not an error
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A).all()
    assert call() == 0
    torch.cuda.synchronize()
    back = out.cpu().numpy()
    assert np.array_equal(back[:h * w].reshape(h, w), want[0]) and (back[h * w:] == 0x5A).all()
    for args in ((2, 1), (8, 5), (1, 3)):
        with pytest.raises(ValueError):
            det.pnm_unpack(d_pay, h, w, *args)
    with pytest.raises(ValueError):
        det.pnm_unpack(d_pay, h, w, 16, 1, black_and_white=True)


# ---- read_pnms --------------------------------------------------------------------------------------------------------
W, H = 65, 7
BY_NAME = {l[0]: l for l in pc.LAYOUTS}


@pytest.fixture(scope="module")
def pnm_list(tmp_path_factory):
    """(names, statuses, the frames they read to): 8-bit files of 65 x 7 of every layout and all four magics, and in between
    one file of every way to fail"""
    d = str(tmp_path_factory.mktemp("pnms"))
    frames = {}

    def put(name, data, want=None):
        path = os.path.join(d, name)
        with open(path, "wb") as f:
            f.write(data)
        frames[path] = want
        return path
    by_layout = {}
    for k, layout in enumerate(pc.LAYOUTS):
        if layout[2] != 16:
            data, want, _ = pc.write_layout(layout, W, H, seed=20 + k)
            by_layout[layout[0]] = put(layout[0] + ".pnm", data, want)
    grey = pc.random_samples(W, H, 8, 1, seed=40)
    pgm = put("grey.pgm", pc.write(grey, 5, 8, head=b"P5\n# a comment\n%d %d\n255\n" % (W, H)), grey[..., 0])
    long_head = pc.random_samples(W, H, 8, 3, seed=41)
    longp = put("long_head.pam", pc.write(long_head, 7, 8, head=pc.pam_head(W, H, 3, 255, "RGB", extra=[b"#" + b"c" * 6000])), pc.expected(long_head, 8, 3))
    small = put("small.pam", pc.write_layout(BY_NAME["p7_rgb8"], 33, H, seed=42)[0])
    deep = put("deep.pam", pc.write_layout(BY_NAME["p7_rgb16"], W, H, seed=43)[0])
    ppm = put("colour.ppm", pc.write(long_head, 6, 8))             # (P6 is not read)
    deep_pgm = put("deep.pgm", pc.write(pc.random_samples(W, H, 16, 1, seed=44), 5, 16, head=b"P5\n%d %d\n65535\n" % (W, H)))
    short = put("short.pam", open(by_layout["p7_rgb8"], "rb").read()[:-1])
    short_pgm = put("short.pgm", open(pgm, "rb").read()[:-1])
    ascii_ = put("ascii.pgm", b"P2\n2 2\n255\n1 2 3 4\n")
    png = os.path.join(d, "board.png")
    files_cases.write_png(png, grey[..., 0])
    frames[png] = None
    missing = os.path.join(d, "missing.ppm")
    frames[missing] = None
    p = by_layout
    names = [p["p7_rgb8"], p["p4"], pgm, missing, p["p7_grey8"], p["p7_grey_alpha8"], small, p["p7_rgb8"], p["p7_rgb_alpha8"], short, deep, p["p7_bw"],
             p["p7_bw_alpha"], p["p7_rgb8"], ppm, png, longp, ascii_, deep_pgm, short_pgm, p["p4"], pgm]
    status = [0, 0, 0, -1, 0, 0, -2, 0, 0, -1, -2, 0, 0, 0, -1, -1, 0, -1, -2, -1, 0, 0]
    return names, status, frames


@pytest.mark.parametrize("chunk,unpack,nthreads", [(1, 1, 4), (2, 1, 0), (3, 1, 2), (0, 1, 1), (0, 0, 4), (3, 0, 2)],
                         ids=["chunks_of_1", "chunks_of_2", "chunks_of_3", "one_chunk", "host_decoded", "host_decoded_chunks_of_3"])
def test_read_pnms(det, pnm_list, chunk, unpack, nthreads):
    names, want_status, frames_of = pnm_list
    det.set_option("pnm_chunk_frames", chunk)
    det.set_option("pnm_unpack", unpack)
    try:
        frames, status = det.read_pnms(names, nthreads=nthreads)
    finally:
        det.set_option("pnm_chunk_frames", 0)
        det.set_option("pnm_unpack", 1)
    assert status.tolist() == want_status
    got = frames.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (len(names), H, W)
    for f, name in enumerate(names):
        img = mrgingham_amd.read_image(name)
        if want_status[f] == 0:
            assert np.array_equal(got[f], img) and np.array_equal(got[f], frames_of[name]), name
        else:
            if want_status[f] == -2:                         # (what read_image can read; -1: what it cannot, or no Netpbm)
                assert img is not None, name
            elif not name.endswith(".png"):
                assert img is None, name
            assert not got[f].any(), name
    assert sum(1 for s in want_status if s == 0) == 13


def test_read_pnms_at_16_bits(det, tmp_path):
    """uint16 frames: P7 of every depth at 16 bits and a 16-bit P5, an 8-bit file among them is of another depth"""
    names, wants = [], []
    for k, layout in enumerate(l for l in pc.LAYOUTS if l[2] == 16):
        data, want, _ = pc.write_layout(layout, 33, 5, seed=60 + k, maxval=65535 if k % 2 else 4095)
        names.append(str(tmp_path / (layout[0] + ".pnm")))
        open(names[-1], "wb").write(data)
        wants.append(want)
    s = pc.random_samples(33, 5, 16, 1, seed=70)
    names.append(str(tmp_path / "deep.pgm"))
    open(names[-1], "wb").write(pc.write(s, 5, 16, head=b"P5 33 5 65535\n"))
    wants.append(s[..., 0])
    names.insert(2, str(tmp_path / "flat.pam"))
    open(names[2], "wb").write(pc.write_layout(BY_NAME["p7_rgb8"], 33, 5)[0])
    wants.insert(2, np.zeros((5, 33), np.uint16))
    for unpack, chunk in ((1, 0), (1, 2), (0, 0)):
        det.set_option("pnm_unpack", unpack)
        det.set_option("pnm_chunk_frames", chunk)
        try:
            frames, status = det.read_pnms(names, nthreads=3)
        finally:
            det.set_option("pnm_unpack", 1)
            det.set_option("pnm_chunk_frames", 0)
        assert status.tolist() == [0, 0, -2, 0, 0, 0]
        got = frames.cpu().numpy()
        assert got.dtype == np.uint16 and np.array_equal(got, np.stack(wants)), (unpack, chunk)


def test_read_pnms_without_a_readable_header(det, pnm_list):
    names, _, _ = pnm_list
    frames, status = det.read_pnms([names[3], names[15]])
    assert tuple(frames.shape) == (2, 0, 0) and status.tolist() == [-1, -1]
    frames, status = det.read_pnms([])
    assert tuple(frames.shape) == (0, 0, 0) and len(status) == 0
    with pytest.raises(ValueError):
        det.set_option("pnm_unpack", 2)
    with pytest.raises(ValueError):
        det.set_option("pnm_chunk_frames", -1)


# ---- find_boards_files(pnm=...) and the tool ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def board_files(tmp_path_factory):
    """the 640 x 480 board as PGM, as P7 RGB (grey in all three channels: it reads back exactly, the weights sum to 2^14), as
    P7 RGB_ALPHA and as P4 (thresholded: a file of the run that bears other numbers)"""
    d = str(tmp_path_factory.mktemp("boards"))
    board = files_cases.board_pixels()
    f = {"board.pgm": os.path.join(d, "board.pgm")}
    files_cases.write_pgm(f["board.pgm"], board)
    rgb = np.stack([board] * 3, axis=-1)
    datas = {"board_rgb.pam": pc.write(rgb, 7, 8), "board.ppm": pc.write(rgb, 6, 8), "board.pam": pc.write(np.concatenate([rgb, np.full(board.shape + (1,), 99, np.uint8)], axis=-1), 7, 8),
             "board.pbm": pc.write((board < 128).astype(np.uint8)[..., None], 4, 1)}
    for name, data in datas.items():
        f[name] = os.path.join(d, name)
        with open(f[name], "wb") as fh:
            fh.write(data)
    f["missing"] = os.path.join(d, "missing.pam")
    f["cut.pam"] = os.path.join(d, "cut.pam")
    with open(f["cut.pam"], "wb") as fh:
        fh.write(datas["board_rgb.pam"][:-1])
    paths = [f["board.pgm"], f["board_rgb.pam"], f["board.pam"], f["missing"], f["board_rgb.pam"], f["board.pbm"], f["cut.pam"], f["board.pam"],
             f["board.pgm"], f["board.ppm"]]                                          # (the P6 file is not read)
    assert mrgingham_amd.read_image(f["board.ppm"]) is None
    for name in ("board_rgb.pam", "board.pam"):
        assert np.array_equal(mrgingham_amd.read_image(f[name]), board)
    return f, paths


RUNS = [(pnm, batch) for pnm in ("host", "device") for batch in (1, 3, 64)]


@pytest.fixture(scope="module")
def board_runs(board_files, tmp_path_factory):
    _, paths = board_files
    runs = [{"id": f"{pnm}_b{batch}", "paths": paths, "kw": {"batch": batch, "nthreads": 4, "pnm": pnm}, "ref": batch == 3} for pnm, batch in RUNS]
    return run_child(str(tmp_path_factory.mktemp("board_runs")), {"runs": runs})


@pytest.mark.parametrize("pnm,batch", RUNS, ids=[f"{b}_b{n}" for b, n in RUNS])
def test_files_give_the_boards_of_the_pgm(board_files, board_runs, pnm, batch):
    f, paths = board_files
    out, rid, n = board_runs, f"{pnm}_b{batch}", len(paths)
    status, found, boards, levels = (out[f"{rid}_{k}"] for k in ("status", "found", "boards", "levels"))
    bad = [paths.index(f["missing"]), paths.index(f["cut.pam"]), paths.index(f["board.ppm"])]
    pbm = paths.index(f["board.pbm"])
    assert len(status) == n and np.flatnonzero(status != 0).tolist() == bad
    assert found[0] >= 0 and not np.isnan(boards[0]).any()                       # (the PGM bears a board)
    for i in range(1, n):
        if i not in bad and i != pbm:                                             # the PGM's numbers, double for double
            assert found[i] == found[0] and np.array_equal(boards[i], boards[0]) and np.array_equal(levels[i], levels[0]), paths[i]
    # every route gives every file the numbers of the first run
    first = f"{RUNS[0][0]}_b{RUNS[0][1]}"
    for what in ("status", "found", "levels"):
        assert np.array_equal(out[f"{rid}_{what}"], out[f"{first}_{what}"]), what
    assert np.array_equal(boards, out[f"{first}_boards"], equal_nan=True)
    if batch == 3:                                                                # ... which are read_image + process_image_ex's
        for what in ("status", "found", "levels"):
            assert np.array_equal(out[f"{rid}_{what}"], out[f"{rid}_ref_{what}"]), what
        assert np.array_equal(boards, out[f"{rid}_ref_boards"], equal_nan=True)
    nfinal = out[rid + "_nfinal"]
    assert len(nfinal) >= 1 and (np.diff(nfinal) >= 0).all() and nfinal[-1] == n and out[rid + "_snap_ok"].all()
    stats = dict(zip(STATS, out[rid + "_stats"]))
    assert stats["files_device_loader"] + stats["files_host_decoded"] + stats["files_one_image"] + stats["files_unreadable"] == n
    assert stats["files_unreadable"] == 3 and stats["files_one_image"] == 0
    npnm = sum(1 for i, p in enumerate(paths) if not p.endswith(".pgm") and i not in bad)
    assert npnm == 5
    assert stats["files_device_loader"] == (npnm if pnm == "device" else 0)       # (P5 files keep their route and counter)
    assert stats["files_host_decoded"] == (2 if pnm == "device" else 2 + npnm)


def test_tool_pnm_unpack_device_prints_the_same_vnlog(board_files):
    f, paths = board_files
    readable = [p for p in dict.fromkeys(paths) if "missing" not in p and "cut" not in p and not p.endswith((".pbm", ".ppm"))]
    plain = run_tool("--jobs", "2", *readable)
    host = run_tool("--jobs", "4", "--batch", "4", *readable)
    device = run_tool("--jobs", "4", "--batch", "4", "--pnm-unpack", "device", *readable)
    assert plain.returncode == 0 and host.returncode == 0 and device.returncode == 0, plain.stderr + host.stderr + device.stderr
    order, records, comments = parse_vnlog(device.stdout)
    assert (order, records) == parse_vnlog(host.stdout)[:2]          # (the comments name the command line)
    assert records == parse_vnlog(plain.stdout)[1]
    assert comments[-1] == "# filename x y level"
    assert order == readable and all(len(records[p]) == 100 for p in readable) and os.access(CLI, os.X_OK)
    want = [line.split(" ", 1)[1] for line in records[f["board.pgm"]]]
    for p in readable:
        assert [line.split(" ", 1)[1] for line in records[p]] == want, p
    r = run_tool("--pnm-unpack", "device", readable[0])
    assert r.returncode != 0 and "--pnm-unpack is only accepted with --batch" in r.stderr
    r = run_tool("--batch", "2", "--pnm-unpack", "both", readable[0])
    assert r.returncode != 0 and "--pnm-unpack takes 'host' or 'device', got 'both'" in r.stderr
    assert "--pnm-unpack host|device" in run_tool("--help").stdout
