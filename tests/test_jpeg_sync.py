"""The host half of the self-synchronising Huffman decoder for files without restart intervals: the decoder text the
device kernels compile (csrc/jpeg_huff_sync.h) under the serial restatement of their schedule (csrc/jpeg.cpp jpeg_sync_*,
behind mrgingham_amd.jpeg_sync_rounds), run under the sanitizers by tests/boundary/jpeg_sync_main.cpp.  Fixtures:
tests/golden/jpeg_sync_golden.npz (make_jpeg_sync_golden.py) beside jpeg_golden.npz and jpeg_rst_golden.npz.  No GPU."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import mrgingham_amd
import test_jpeg_io
from test_jpeg_io import Case
from test_jpeg_scan import Lcg, entropy_range, rst_case, rst_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrgingham_amd", "csrc")
REALISTIC = ("blend_320x240_grey_q90", "blendopt_320x240_grey_q90", "blend_320x240_444_q95", "blend_320x240_422_q75",
             "blend_320x240_420_q90", "blend_320x240_420_q50", "plain_320x240_420_q90", "blend_640x480_420_q90")

_sync = None


def sync_cases():
    global _sync
    if _sync is None:
        g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_sync_golden.npz"))
        _sync = [Case(g, i) for i in range(len(g["name"]))]
    return _sync


def sync_case(prefix):
    return next(c for c in sync_cases() if c.name.startswith(prefix))


def nodri_cases():
    """Every readable fixture of the three golden files that has no restart intervals."""
    return [c for c in test_jpeg_io.cases() + rst_cases() + sync_cases()
            if c.readable and mrgingham_amd.jpeg_restart_intervals(c.data)[0] == 0]


def small_nodri_fixtures():
    """The files the corruptions are made from: every one of nodri_cases() but the boards (15 KB and more a copy) whose
    entropy-coded segment has at least 16 bytes."""
    out = []
    for c in nodri_cases():
        lo, hi = entropy_range(c.data)
        if not c.name.startswith(("board", "blend", "plain")) and hi - lo >= 16:
            out.append(c)
    return out


def sync_corruptions(c, per_kind=200):
    """[(kind, bytes)]: per_kind each of one bit flipped, one byte replaced, truncation, one byte removed -- all inside the
    entropy-coded segment, seeded by the fixture's name (the first four kinds of test_jpeg_scan.corruptions, which goes
    on to index restart offsets these files have not got)."""
    d = c.data
    lo, hi = entropy_range(d)
    rnd = Lcg(sum(c.name.encode()) * 7919 + len(d))
    out = []
    for _ in range(per_kind):
        at = lo + rnd(hi - lo)
        out.append(("flip", d[:at] + bytes([d[at] ^ (1 << rnd(8))]) + d[at + 1:]))
    for _ in range(per_kind):
        at = lo + rnd(hi - lo)
        out.append(("replace", d[:at] + bytes([(d[at] + 1 + rnd(255)) & 255]) + d[at + 1:]))
    for _ in range(per_kind):
        out.append(("truncate", d[:lo + rnd(hi - lo)]))
    for _ in range(per_kind):
        at = lo + rnd(hi - lo)
        out.append(("remove", d[:at] + d[at + 1:]))
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("jpeg_sync_program")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++", *flags, str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp / "probe")]).returncode != 0:
        pytest.skip("the sanitizer runtime of g++ is not installed")
    exe = str(tmp / "jpeg_sync")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "boundary", "jpeg_sync_main.cpp"),
                        os.path.join(CSRC, "jpeg.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_program(exe, tmp_path, items, sizes, cap=False, parts=1):
    """-> (accepted bool [n], rounds int [n, len(sizes)]; -1 where the file is not accepted).  parts: the corpus is cut
    into that many pieces, each walked by a process of its own."""
    procs = []
    for q in range(parts):
        mine = items[q * len(items) // parts:(q + 1) * len(items) // parts]
        blob, got = tmp_path / f"corpus{q}.bin", tmp_path / f"result{q}.txt"
        with open(blob, "wb") as f:
            f.write(struct.pack("<I", len(mine)))
            for data in mine:
                f.write(struct.pack("<I", len(data)) + data)
        procs.append((len(mine), got, subprocess.Popen([exe, str(blob), str(got), *(["cap"] if cap else []), *[str(s) for s in sizes]],
                                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    tables = []
    for count, got, p in procs:
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, (out, err[-4000:])
        table = np.loadtxt(got, dtype=np.int64, ndmin=2).reshape(count, 1 + len(sizes))
        assert out.split() == ["cases", str(count), "accepted", str(int(table[:, 0].sum()))], out
        tables.append(table)
    table = np.concatenate(tables)
    return table[:, 0].astype(bool), table[:, 1:]


def test_sync_fixture_set_is_what_the_other_tests_rely_on():
    names = [c.name for c in sync_cases()]
    assert names == list(REALISTIC) + ["noise_48x64_grey_q100"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_sync_golden.npz")) < 300 * 1024
    for c in sync_cases():
        assert b"\xff\xdd" not in c.data and mrgingham_amd.jpeg_restart_intervals(c.data)[0] == 0, c.name
        r = mrgingham_amd.jpeg_coefficients(c.data)
        assert r is not None and r[0].shape == (c.blocks_h, c.blocks_w, 64) and r[2] == (c.height, c.width), c.name
        if c.luma.size:
            assert np.array_equal(test_jpeg_io.plane_of(*r[:2], *r[2]), c.luma), c.name
    assert sync_case("blend_320x240_grey_q90").luma.size and sync_case("noise").luma.size
    for name in REALISTIC:                                           # half the default cap of 8192 bytes, at the least
        rounds, n = mrgingham_amd.jpeg_sync_rounds(sync_case(name).data, 32)
        assert rounds * 32 <= 4096 and n > 8 * rounds, (name, rounds, n)
    lo, hi = entropy_range(sync_case("blend_640x480").data)
    assert (hi - lo) // 8 >= 4 * 256                                 # many workgroups at 8-byte subsequences
    noise = sync_case("noise").data
    lo, hi = entropy_range(noise)
    assert noise[lo:hi].count(b"\xff\x00") >= 8
    rounds, n = mrgingham_amd.jpeg_sync_rounds(noise, 32)
    assert rounds > n // 2                                           # it hardly synchronises: rounds in proportion to its length


def test_schedule_equals_the_host_decoder_on_every_file_without_restart_intervals_under_sanitizers(program, tmp_path):
    """Intact files at S = 8, 32, 128 with as many rounds allowed as there are subsequences: int16 for int16 what
    jpeg_coefficients gives, the converged records a fixed point, jpeg_sync_decode not converged one round below its count
    (all checked inside the program), and the library's jpeg_sync_rounds equal to what the program counts."""
    cases = nodri_cases()
    assert len(cases) >= 21 + 9
    accepted, rounds = run_program(program, tmp_path, [c.data for c in cases], (8, 32, 128), cap=True)
    assert accepted.all()
    for c, row in zip(cases, rounds):
        for S, r in zip((8, 32, 128), row):
            lo, hi = entropy_range(c.data)
            got = mrgingham_amd.jpeg_sync_rounds(c.data, S)
            assert got is not None and got[0] == r and 0 <= r < max(got[1], 1), (c.name, S, got, r)
            assert abs(got[1] - -(-(hi - lo) // S)) <= 1, (c.name, S, got)       # (a file may lack its EOI: +- one piece)
    by_name = {c.name: row for c, row in zip(cases, rounds)}
    assert by_name["noise_48x64_444_q95_r0"][1] > 64 and by_name["nodri_48x64_420_q75_dri0"][1] > 16     # what the cap tests cut


def test_jpeg_sync_rounds_boundary():
    from mrgingham_amd import _lib
    L = _lib.lib()
    d = rst_case("nodri_48x64").data
    r, n = ctypes.c_int(-7), ctypes.c_size_t(77)
    assert L.mrgingham_amd_jpeg_sync_rounds(d, len(d), 32, ctypes.byref(r), ctypes.byref(n)) == 0 and r.value > 0 and n.value > r.value
    assert L.mrgingham_amd_jpeg_sync_rounds(d, len(d), 32, None, None) == 0
    dri = rst_case("noise_53x37_420").data
    assert L.mrgingham_amd_jpeg_sync_rounds(dri, len(dri), 32, ctypes.byref(r), ctypes.byref(n)) == -3 and (r.value, n.value) == (0, 0)
    prog = test_jpeg_io.case("progressive_48x64").data
    assert L.mrgingham_amd_jpeg_sync_rounds(prog, len(prog), 32, ctypes.byref(r), ctypes.byref(n)) == -1
    assert L.mrgingham_amd_jpeg_sync_rounds(None, 10, 32, None, None) == -1
    assert L.mrgingham_amd_jpeg_sync_rounds(d[:len(d) // 2], len(d) // 2, 32, None, None) == -1      # truncated: unreadable
    for bad in (0, 4, 6, 30, 1028, -8):
        assert L.mrgingham_amd_jpeg_sync_rounds(d, len(d), bad, None, None) == -1, bad
        with pytest.raises(ValueError):
            mrgingham_amd.jpeg_sync_rounds(d, bad)
    with pytest.raises(ValueError):
        mrgingham_amd.jpeg_sync_rounds(dri, 32)
    assert mrgingham_amd.jpeg_sync_rounds(prog) is None and mrgingham_amd.jpeg_sync_rounds(b"") is None
    assert "mrgingham_amd_jpeg_sync_rounds" in _lib.EXPORTS and L.mrgingham_amd_abi_version() == 4


def test_corrupted_files_are_accepted_exactly_when_the_host_accepts_under_sanitizers(program, tmp_path):
    """Seeded corruptions of the entropy-coded segment of every small file without restart intervals, at S = 8 and 32: the
    program fails on the first file that the schedule and jpeg_coefficients disagree about (acceptance, or a coefficient
    where both accept).  The corruptions must bite: the host decoder rejects between 30 % and 80 % of the flips and
    replacements, pooled, and every truncation."""
    fixtures = small_nodri_fixtures()
    assert len(fixtures) >= 16 + 1 and any(c.name.startswith("noise_48x64_grey_q100") for c in fixtures)
    kinds, items = [], []
    for c in fixtures:
        made = sync_corruptions(c)
        assert len(made) == 800, c.name
        kinds += [k for k, _ in made]
        items += [d for _, d in made]
    accepted, _ = run_program(program, tmp_path, items, (8, 32), parts=8)
    host = np.array([mrgingham_amd.jpeg_coefficients(d) is not None for d in items])
    assert np.array_equal(accepted, host)                                 # (the sanitized build and the library agree)
    kinds = np.array(kinds)
    pooled = ~host[(kinds == "flip") | (kinds == "replace")]
    print("rejected: flips + replacements %.1f %%, truncations %.1f %%, removals %.1f %%"
          % (100 * pooled.mean(), 100 * (~host[kinds == "truncate"]).mean(), 100 * (~host[kinds == "remove"]).mean()))
    assert 0.30 <= pooled.mean() <= 0.80
    assert not host[kinds == "truncate"].any()
