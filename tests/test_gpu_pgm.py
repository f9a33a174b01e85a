"""Binary PGM files into device frames (Detector.pgm_unpack, Detector.read_pgms) and 16-bit files through the chunks of
find_boards_files (deep="chunks", the tool's --deep-batch chunks).  The unpack kernel moves bytes and swaps the two of a
16-bit sample: numpy's frombuffer(.., ">u2") is the yardstick; for files it is read_image (the samples' high bytes, or
the bytes) and the file's own bytes; for the route it is deep="one", the one-image path.  No tolerance anywhere.

The shapes sit where the kernel's 16-byte words meet the rows: sample counts that are odd, so that the rows of later
frames begin at every 2-byte phase of a word, and widths around 8 and 16 samples.  Nothing is larger than 640 x 480."""
import os

import numpy as np
import pytest

import mrgingham_amd
from tests import files_cases, png_cases
from tests.test_gpu_files import CLI, STATS, parse_vnlog, run_child, run_tool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector()
    yield d
    d.close()


def _payload(samples, bits):
    """[B, h, w] unsigned samples -> (the files' payloads uint8 [B, P], P the next multiple of 16; the frames numpy reads out of them)"""
    B = samples.shape[0]
    raw = samples.astype(">u2" if bits == 16 else np.uint8).reshape(B, -1).view(np.uint8)
    pay = np.zeros((B, (raw.shape[1] + 15) // 16 * 16), np.uint8)
    pay[:, :raw.shape[1]] = raw
    pay[:, raw.shape[1]:] = 0xEE                                   # (what lies behind a payload is never a sample)
    want = np.stack([np.frombuffer(pay[f, :raw.shape[1]].tobytes(), ">u2" if bits == 16 else np.uint8) for f in range(B)])
    return pay, want.reshape(samples.shape).astype(np.uint16 if bits == 16 else np.uint8)


def _random(B, h, w, bits, seed=0):
    return np.random.default_rng(seed).integers(0, 1 << bits, (B, h, w)).astype(np.uint16 if bits == 16 else np.uint8)


def _unpack(det, pay, h, w, bits, out=None):
    import torch
    got = det.pgm_unpack(torch.from_numpy(pay).cuda(), h, w, bits, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy()


# (the last three: more than one row per workgroup, one, and a row of more words than a workgroup has lanes, twice over)
SHAPES = [(1, 1), (5, 3), (9, 17)] + [(3, w) for w in (7, 8, 9, 15, 16, 17)] + [(70, 33), (2, 300), (2, 4200)]


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{w}x{h}" for h, w in SHAPES])
def test_unpack_equals_numpy(det, h, w, bits):
    """nine dense frames: with an odd sample count the frames, and their rows, begin at every 2-byte phase of a word"""
    samples = _random(9, h, w, bits, seed=h * 100 + w)
    pay, want = _payload(samples, bits)
    got = _unpack(det, pay, h, w, bits)
    assert got.dtype == want.dtype and got.shape == (9, h, w)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("rows_per_workgroup", [1, 256])
def test_unpack_takes_a_second_trip_over_the_rows(det, bits, rows_per_workgroup):
    """The grid is capped at eight workgroups per CU and the kernel loops over the rows beyond: every full-size call
    takes that loop, no other shape of this file does.  A row is taken by the power of two of lanes that covers its
    16-byte words, so a workgroup of 256 lanes holds one row of 2049 bytes or more (129 words and one more, the rows
    beginning inside a word), and 256 dense rows of 16 bytes.  The smallest row count above one trip, the last trip ragged."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows_per_trip = 8 * cus * rows_per_workgroup
    if rows_per_workgroup == 1:
        B, h, rowb = 1, rows_per_trip + 37, 2050
        assert (rowb + 15) // 16 + 1 > 128 and rowb % 16 != 0            # more words than 128 lanes cover; rows at every phase
    else:
        rowb = 16                                                        # dense and aligned: one word per row, one lane
        h = next(h for h in range(4099, 4200) if ((rows_per_trip // h + 1) * h - rows_per_trip) % 256)
        B = rows_per_trip // h + 1
    w, nrows = rowb * 8 // bits, B * h
    assert rows_per_trip < nrows < 2 * rows_per_trip                     # two trips
    assert (nrows - rows_per_trip) % rows_per_workgroup or rows_per_workgroup == 1   # ... whose last workgroup is not full
    samples = _random(B, h, w, bits, seed=bits + rows_per_workgroup)
    pay, want = _payload(samples, bits)
    got = _unpack(det, pay, h, w, bits)
    assert got.dtype == want.dtype and got.shape == (B, h, w)
    assert np.array_equal(got, want)


def test_every_16_bit_value_once(det):
    """(a wrong permute selector cannot hide: 0x0102 must come out as 0x0102 from the bytes 01 02)"""
    samples = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    pay, want = _payload(samples, 16)
    assert pay[0, 2 * 0x0102] == 0x01 and pay[0, 2 * 0x0102 + 1] == 0x02
    assert np.array_equal(_unpack(det, pay, 256, 256, 16), samples)
    samples8 = (np.arange(65536) % 256).astype(np.uint8).reshape(1, 256, 256)
    assert np.array_equal(_unpack(det, _payload(samples8, 8)[0], 256, 256, 8), samples8)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("h,w", [(9, 17), (3, 16), (4, 40)], ids=["17x9", "16x3", "40x4"])
def test_strided_output_leaves_everything_else_alone(det, h, w, bits):
    import torch
    stride, rows = w + 5, h + 2
    samples = _random(3, h, w, bits, seed=7)
    pay, want = _payload(samples, bits)
    dtype, sentinel = (torch.uint8, 0xA5) if bits == 8 else (torch.uint16, 0xA5A5)
    big = torch.full((3, rows, stride), sentinel, dtype=dtype, device="cuda")
    _unpack(det, pay, h, w, bits, out=big[:, :h, :])
    back = big.cpu().numpy()
    assert np.array_equal(back[:, :h, :w], want)
    assert (back[:, :h, w:] == sentinel).all() and (back[:, h:, :] == sentinel).all()


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("h,w", [(4, 8), (16, 24), (3, 16), (64, 100)], ids=["8x4", "24x16", "16x3", "100x64"])
def test_in_place(det, h, w, bits):
    """the layouts coincide (dense frames, a payload of whole words): the output is the payload buffer itself"""
    import torch
    samples = _random(3, h, w, bits, seed=11)
    pay, want = _payload(samples, bits)
    assert pay.shape[1] == h * w * bits // 8
    d_pay = torch.from_numpy(pay).cuda()
    out = (d_pay.view(torch.uint16) if bits == 16 else d_pay).view(3, h, w)
    got = det.pgm_unpack(d_pay, h, w, bits, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == d_pay.data_ptr()
    assert np.array_equal(got.cpu().numpy(), want)


def test_no_frames_and_bad_arguments_write_nothing(det):
    import torch
    h, w, bits = 5, 9, 16
    samples = _random(1, h, w, bits)
    pay, want = _payload(samples, bits)
    d_pay = torch.from_numpy(pay).cuda()
    out = torch.full((h * w + 8,), 0x5A5A, dtype=torch.uint16, device="cuda")
    pitch = pay.shape[1]
    assert tuple(det.pgm_unpack(d_pay[:0], h, w, bits).shape) == (0, h, w)

    def call(d_payload=None, payload_pitch=pitch, n=1, width=w, height=h, bits=bits, d_out=None, frame_pitch=w * h, stride=w, ctx=None):
        return det.L.mrgingham_amd_pgm_unpack_batch(det.ctx if ctx is None else ctx, d_pay.data_ptr() if d_payload is None else d_payload,
                                                    payload_pitch, n, width, height, bits, out.data_ptr() if d_out is None else d_out,
                                                    frame_pitch, stride, None)
    bad = [dict(n=-1), dict(width=-1), dict(height=-1), dict(stride=w - 1), dict(frame_pitch=-1), dict(payload_pitch=-16),
           dict(payload_pitch=pitch - 16), dict(payload_pitch=pitch + 8), dict(bits=12), dict(bits=4), dict(bits=32),
           dict(d_payload=d_pay.data_ptr() + 4), dict(d_payload=d_pay.data_ptr() + 8), dict(d_payload=0), dict(d_out=0),
           dict(d_out=out.data_ptr() + 1), dict(width=32768, stride=32768, payload_pitch=1 << 40), dict(height=32768, payload_pitch=1 << 40)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert det.L.mrgingham_amd_pgm_unpack_batch(None, d_pay.data_ptr(), pitch, 1, w, h, bits, out.data_ptr(), w * h, w, None) == -1
    assert call(n=0) == 0 and call(width=0, stride=0) == 0 and call(height=0) == 0               # nothing to do is not an error
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A).all()
    assert call() == 0
    torch.cuda.synchronize()
    back = out.cpu().numpy()
    assert np.array_equal(back[:h * w].reshape(h, w), want[0]) and (back[h * w:] == 0x5A5A).all()


# ---- read_pgms --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return files_cases.write_all(tmp_path_factory.mktemp("files"))


@pytest.fixture(scope="module")
def pgm_lists(files, tmp_path_factory):
    """per depth: (names, statuses) -- eight copies of the board and, in between, one file of every way to fail, and a
    header with comments that puts the samples at an odd offset"""
    d = str(tmp_path_factory.mktemp("pgms"))
    board = files_cases.board_pixels()
    out = {}
    for bits, stem, other in ((16, "board16.pgm", "board.pgm"), (8, "board.pgm", "board16.pgm")):
        good = open(files[stem], "rb").read()
        nbytes = 640 * 480 * bits // 8
        short = os.path.join(d, f"short{bits}.pgm")
        with open(short, "wb") as f:
            f.write(good[:-1])
        small = os.path.join(d, f"small{bits}.pgm")
        files_cases.write_pgm(small, board[:100, :200].astype(np.uint16) * (257 if bits == 16 else 1), maxval=65535 if bits == 16 else 255)
        odd = os.path.join(d, f"odd{bits}.pgm")
        head = b"P5 # one\n# two.\n640\t480 #three\n%d\r" % (65535 if bits == 16 else 255)
        assert len(head) % 2 == 1
        with open(odd, "wb") as f:
            f.write(head + good[-nbytes:][::-1])            # (other samples than the board's: the bytes reversed)
        names = [files[stem]] * 3 + [files["missing"], files[stem], files["board.png"], files[other], files[stem], small, short,
                                     odd, files[stem], files[stem], files[stem]]
        out[bits] = (names, [0, 0, 0, -1, 0, -1, -2, 0, -2, -1, 0, 0, 0, 0])
    return out


def _samples_of(path, bits):
    """the samples of a readable 640x480 PGM straight from its last bytes"""
    data = open(path, "rb").read()
    return np.frombuffer(data[len(data) - 640 * 480 * bits // 8:], ">u2" if bits == 16 else np.uint8).reshape(480, 640)


@pytest.mark.parametrize("bits,chunk,nthreads", [(16, 1, 4), (16, 3, 0), (16, 0, 1), (8, 3, 4)],
                         ids=["16bit_chunks_of_1", "16bit_chunks_of_3", "16bit_one_chunk", "8bit_chunks_of_3"])
def test_read_pgms(det, pgm_lists, bits, chunk, nthreads):
    names, want_status = pgm_lists[bits]
    det.set_option("pgm_chunk_frames", chunk)
    try:
        frames, status = det.read_pgms(names, nthreads=nthreads)
    finally:
        det.set_option("pgm_chunk_frames", 0)
    assert status.tolist() == want_status
    got = frames.cpu().numpy()
    assert got.dtype == (np.uint16 if bits == 16 else np.uint8) and got.shape == (len(names), 480, 640)
    for f, name in enumerate(names):
        if want_status[f] == 0:
            img = mrgingham_amd.read_image(name)              # (of a 16-bit file: the high bytes)
            assert np.array_equal(got[f] >> 8 if bits == 16 else got[f], img), name
            assert np.array_equal(got[f], _samples_of(name, bits)), name
        else:
            if name.endswith(".pgm"):                         # (-1: what read_image cannot read either; -2: what it can)
                assert (mrgingham_amd.read_image(name) is None) == (want_status[f] == -1), name
            assert not got[f].any(), name
    assert sum(1 for s in want_status if s == 0) == 9


def test_read_pgms_without_a_readable_header(det, files):
    frames, status = det.read_pgms([files["missing"], files["board.png"]])
    assert tuple(frames.shape) == (2, 0, 0) and status.tolist() == [-1, -1]
    frames, status = det.read_pgms([])
    assert tuple(frames.shape) == (0, 0, 0) and len(status) == 0


# ---- find_boards_files(deep="chunks") -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deep_files(files, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("deep"))
    board16 = files_cases.board_pixels().astype(np.uint16) * 257
    f = dict(files)
    f["grey16_a.png"] = os.path.join(d, "grey16_a.png")
    files_cases.write_png(f["grey16_a.png"], board16, bits=16)
    f["grey16_b.png"] = os.path.join(d, "grey16_b.png")
    png_cases.write(f["grey16_b.png"], board16, 0, 16, filters=("random", 2), nidat=2)
    f["rgb16.png"] = os.path.join(d, "rgb16.png")                 # r = g = b: its grey is the board
    png_cases.write(f["rgb16.png"], np.stack([board16] * 3, axis=-1), 2, 16, filters=("random", 3), nidat=3)
    f["tiny16.pgm"] = os.path.join(d, "tiny16.pgm")
    files_cases.write_pgm(f["tiny16.pgm"], (np.arange(16).reshape(4, 4) * 4000).astype(np.uint16), maxval=65535)
    b16 = f["board16.pgm"]
    paths = [b16, f["grey16_a.png"], f["board.pgm"], b16, f["rgb16.png"], f["tiny16.pgm"], f[files_cases.BOARD], b16, f["missing"],
             f["grey16_b.png"], b16, f["board.png"], b16]
    return f, paths


COMBOS = [(batch, clahe, blur, png) for png in ("host", "device") for clahe in (True, False) for blur in (0, 1) for batch in (1, 2, 64)]


def _rid(deep, batch, clahe, blur, png):
    return f"{deep}_b{batch}_c{int(clahe)}_r{blur}_{png}"


@pytest.fixture(scope="module")
def deep_runs(deep_files, tmp_path_factory):
    """every combination with deep="chunks", and deep="one" once per preprocessing: a child process per png route"""
    _, paths = deep_files
    out = {}
    for png in ("host", "device"):
        runs = [{"id": _rid("chunks", b, c, r, p), "paths": paths,
                 "kw": {"batch": b, "nthreads": 4, "clahe": c, "blur_radius": r, "png": p, "deep": "chunks"}} for b, c, r, p in COMBOS if p == png]
        runs += [{"id": _rid("one", 2, c, r, png), "paths": paths,
                  "kw": {"batch": 2, "nthreads": 4, "clahe": c, "blur_radius": r, "png": png, "deep": "one"}} for c in (True, False) for r in (0, 1)]
        out.update(run_child(str(tmp_path_factory.mktemp("deep_runs_" + png)), {"runs": runs}))
    return out


@pytest.mark.parametrize("batch,clahe,blur,png", COMBOS, ids=[_rid("chunks", *c) for c in COMBOS])
def test_chunks_equal_the_one_image_path(deep_files, deep_runs, batch, clahe, blur, png):
    f, paths = deep_files
    out, n = deep_runs, len(paths)
    got, want = _rid("chunks", batch, clahe, blur, png), _rid("one", 2, clahe, blur, png)
    for what in ("status", "found", "levels"):
        assert np.array_equal(out[f"{got}_{what}"], out[f"{want}_{what}"]), what
    assert np.array_equal(out[got + "_boards"], out[want + "_boards"], equal_nan=True)
    status, found = out[got + "_status"], out[got + "_found"]
    assert len(status) == n and np.flatnonzero(status != 0).tolist() == [paths.index(f["missing"])]
    assert (found[[i for i, p in enumerate(paths) if "tiny" not in p and "missing" not in p]] >= 0).all()   # (the files bear boards)
    # progress: non-decreasing, ends at n, and what it called final stayed as it was
    nfinal = out[got + "_nfinal"]
    assert len(nfinal) >= 1 and (np.diff(nfinal) >= 0).all() and nfinal[-1] == n and out[got + "_snap_ok"].all()
    # stats: only the 4x4 file, and only under CLAHE, is left to the one-image path
    stats = dict(zip(STATS, out[got + "_stats"]))
    one = dict(zip(STATS, out[want + "_stats"]))
    assert stats["files_one_image"] == (1 if clahe else 0)
    assert stats["files_device_loader"] + stats["files_host_decoded"] + stats["files_one_image"] + stats["files_unreadable"] == n
    assert stats["files_unreadable"] == 1
    pgm16 = sum(1 for p in paths if p.endswith("board16.pgm")) + (0 if clahe else 1)
    png16 = sum(1 for p in paths if p.endswith(("grey16_a.png", "grey16_b.png", "rgb16.png")))
    if png == "device":
        assert stats["files_device_loader"] == 1 + pgm16 + png16 + 1          # the JPEG, and board.png as well
        assert stats["files_host_decoded"] == 1                               # board.pgm
    else:
        assert stats["files_device_loader"] == 1 + pgm16
        assert stats["files_host_decoded"] == 2 + png16
    assert one["files_one_image"] == sum(1 for p in paths if p.endswith(("16.pgm", "16_a.png", "16_b.png", "rgb16.png")))


def test_tool_deep_batch_chunks_prints_the_same_vnlog(deep_files):
    f, paths = deep_files
    readable = [p for p in dict.fromkeys(paths) if "missing" not in p]
    one = run_tool("--jobs", "4", "--batch", "2", *readable)
    chunks = run_tool("--jobs", "4", "--batch", "2", "--deep-batch", "chunks", *readable)
    assert one.returncode == 0 and chunks.returncode == 0, one.stderr + chunks.stderr
    order, records, comments = parse_vnlog(chunks.stdout)
    assert (order, records) == parse_vnlog(one.stdout)[:2]          # (the comments name the command line)
    assert comments[-1] == "# filename x y level"
    assert order == readable and len(records[f["rgb16.png"]]) == 100 and len(records[f["board16.pgm"]]) == 100 and os.access(CLI, os.X_OK)
    r = run_tool("--deep-batch", "chunks", readable[0])
    assert r.returncode != 0 and "--deep-batch is only accepted with --batch" in r.stderr
    r = run_tool("--batch", "2", "--deep-batch", "both", readable[0])
    assert r.returncode != 0 and "--deep-batch takes 'one' or 'chunks', got 'both'" in r.stderr
