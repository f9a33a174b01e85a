"""The host half of the device entropy decoder: the marker scan that takes a baseline JPEG apart into its restart
intervals (csrc/jpeg.cpp jpeg_scan, behind mrgingham_amd.jpeg_restart_intervals) and the per-interval Huffman decoder
the device kernel compiles (csrc/jpeg_huff_lane.h), run on the host under the sanitizers by
tests/boundary/jpeg_lane_main.cpp.  Fixtures: tests/golden/jpeg_rst_golden.npz (make_jpeg_rst_golden.py) beside
jpeg_golden.npz.  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import mrgingham_amd
import test_jpeg_io
from test_jpeg_io import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrgingham_amd", "csrc")

_rst = None


def rst_cases():
    global _rst
    if _rst is None:
        g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_rst_golden.npz"))
        _rst = [Case(g, i) for i in range(len(g["name"]))]
    return _rst


def rst_case(prefix):
    return next(c for c in rst_cases() if c.name.startswith(prefix))


def dri_fixtures():
    """The files of the table the corruptions are made from: every DRI fixture but the 640x480 board (37 KB a copy)."""
    return [c for c in rst_cases() if not c.name.endswith("_dri0") and not c.name.startswith("board")]


def entropy_range(data):
    sos = data.index(b"\xff\xda")
    return sos + 2 + struct.unpack(">H", data[sos + 2:sos + 4])[0], len(data) - 2      # (up to the EOI marker)


class Lcg:
    def __init__(self, seed):
        self.x = seed & 0x7FFFFFFF

    def __call__(self, n):
        self.x = (self.x * 1103515245 + 12345) & 0x7FFFFFFF
        return (self.x >> 8) % n


def corruptions(c, per_kind=200):
    """[(kind, bytes)]: per_kind each of one bit flipped, one byte replaced, truncation, one byte removed -- all inside the
    entropy-coded segment, seeded by the fixture's name -- and up to three hand-made ones: an RST marker removed, two RST
    numbers exchanged, FF D9 planted in the middle of an interval."""
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
    _, offsets = mrgingham_amd.jpeg_restart_intervals(d)
    if len(offsets) >= 3:
        a, b = int(offsets[0, 1]), int(offsets[1, 1])                  # FF Dn behind the first and the second interval
        assert d[a] == 0xFF and d[a + 1] == 0xD0 and d[b] == 0xFF and d[b + 1] == 0xD1
        out.append(("rst_removed", d[:a] + d[a + 2:]))
        out.append(("rst_exchanged", d[:a + 1] + b"\xd1" + d[a + 2:b + 1] + b"\xd0" + d[b + 2:]))
    begin, end = (int(v) for v in offsets[len(offsets) // 2])
    if end - begin >= 4:
        mid = (begin + end) // 2
        out.append(("eoi_planted", d[:mid] + b"\xff\xd9" + d[mid + 2:]))
    return out


def test_rst_fixture_set_is_what_the_other_tests_rely_on():
    names = [c.name for c in rst_cases()]
    for part in ("noise_8x8_grey_q75_dri1", "noise_17x9_444_q75_dri1", "noise_31x33_420_q75_dri4", "noise_31x33_422_q75_dri1",
                 "noise_31x33_grey_q75_dri1", "noise_53x37_420_q75_dri5", "noise_48x64_grey_q75_dri1", "noise_136x136_grey_q75_dri1",
                 "noise_264x16_420_q75_dri7", "noise_48x64_444_q100_dri2", "noise_48x64_420_q30_dri3", "black_48x64_grey_q75_dri1",
                 "optimize_48x64_420_q75_dri2", "rows_48x64_420_q75_dri3", "nodri_48x64_420_q75_dri0", "board_640x480_grey_q90_dri80"):
        assert part in names, part
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_rst_golden.npz")) < 150 * 1024
    assert b"\xff\xd0" not in rst_case("noise_8x8").data                              # one interval: no RST marker
    wraps = rst_case("noise_48x64_grey").data
    assert wraps.count(b"\xff\xd7") >= 5 and len(mrgingham_amd.jpeg_restart_intervals(wraps)[1]) == 48
    lo, hi = entropy_range(rst_case("noise_48x64_444_q100").data)
    assert b"\xff\x00" in rst_case("noise_48x64_444_q100").data[lo:hi]
    assert len(mrgingham_amd.jpeg_restart_intervals(rst_case("noise_136x136").data)[1]) == 289
    sizes = np.diff(mrgingham_amd.jpeg_restart_intervals(rst_case("black_48x64").data)[1], axis=1)
    assert sizes.min() >= 1 and sizes.max() <= 3      # the shortest intervals there are (DC -64 after every reset: 3 bytes)


def test_host_decoder_reads_the_rst_fixtures(tmp_path):
    for c in rst_cases():
        r = mrgingham_amd.jpeg_coefficients(c.data)
        assert r is not None and r[0].shape == (c.blocks_h, c.blocks_w, 64) and r[2] == (c.height, c.width), c.name
        if c.luma.size:
            assert np.array_equal(test_jpeg_io.plane_of(*r[:2], *r[2]), c.luma), c.name


def test_scan_accepts_what_jpeg_coefficients_accepts_and_lists_disjoint_intervals():
    seen = 0
    for c in test_jpeg_io.cases() + rst_cases():
        host = mrgingham_amd.jpeg_coefficients(c.data)
        scan = mrgingham_amd.jpeg_restart_intervals(c.data)
        assert (scan is None) == (host is None) == (not c.readable), c.name
        if scan is None:
            continue
        dri, offsets = scan
        assert offsets.dtype == np.int64 and offsets.ndim == 2 and offsets.shape[1] == 2, c.name
        if dri == 0:
            assert len(offsets) == 0 and b"\xff\xdd" not in c.data, c.name
            continue
        seen += 1
        coef = host[0]
        H0 = V0 = 1
        if "_420" in c.name:
            H0 = V0 = 2
        elif "_422" in c.name:
            H0 = 2
        nmcu = (coef.shape[0] // V0) * (coef.shape[1] // H0)
        assert len(offsets) == -(-nmcu // dri), c.name
        lo, hi = entropy_range(c.data)
        assert offsets[0, 0] == lo and offsets[-1, 1] == hi, c.name
        assert (offsets[:, 0] <= offsets[:, 1]).all() and (offsets[1:, 0] > offsets[:-1, 1]).all(), c.name   # disjoint, ordered
        for i in range(len(offsets) - 1):                                  # what lies between two of them is one RST marker
            assert c.data[offsets[i, 1]:offsets[i + 1, 0]] == bytes([0xFF, 0xD0 + (i & 7)]), (c.name, i)
    assert seen >= 15 + 20                                                 # (two thirds of the older fixtures have a DRI)
    assert mrgingham_amd.jpeg_restart_intervals(b"") is None and mrgingham_amd.jpeg_restart_intervals(b"\xff\xd8\xff") is None


def test_scan_c_boundary():
    import ctypes
    from mrgingham_amd import _lib
    L = _lib.lib()
    d = rst_case("noise_53x37_420").data
    ri, n = ctypes.c_int(), ctypes.c_size_t()
    assert L.mrgingham_amd_jpeg_restart_intervals(d, len(d), ctypes.byref(ri), None, 0, ctypes.byref(n)) == 0
    assert (ri.value, n.value) == (5, 3)
    out = np.full((4, 2), -7, np.int64)
    assert L.mrgingham_amd_jpeg_restart_intervals(d, len(d), None, out.ctypes.data, 2, None) == -2 and (out == -7).all()
    assert L.mrgingham_amd_jpeg_restart_intervals(d, len(d), None, out.ctypes.data, 3, None) == 0
    assert (out[3] == -7).all() and (out[:3] > 0).all()
    assert L.mrgingham_amd_jpeg_restart_intervals(None, 10, None, None, 0, None) == -1
    first = d.index(b"\xff\xd0")
    bad = d[:first + 1] + b"\xd1" + d[first + 2:]
    assert L.mrgingham_amd_jpeg_restart_intervals(bad, len(bad), None, None, 0, None) == -1        # out of sequence


def _sanitized_lane_program(tmp_path, name="jpeg_lane"):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the sanitizer runtime of g++ is not installed")
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "boundary", name + "_main.cpp"),
                        os.path.join(CSRC, "jpeg.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run_lane_program(exe, tmp_path, items):
    blob = tmp_path / "corpus.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for data in items:
            f.write(struct.pack("<I", len(data)) + data)
    got = tmp_path / "accepted.bin"
    r = subprocess.run([exe, str(blob), str(got)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    accepted = np.frombuffer(got.read_bytes(), np.uint8)
    assert r.stdout.split() == ["cases", str(len(items)), "accepted", str(int(accepted.sum()))], r.stdout
    return accepted


def test_lanes_in_reverse_order_equal_the_host_decoder_under_sanitizers(tmp_path):
    """Every DRI fixture of both golden files, intact: decoded interval by interval, last interval first, int16 for int16
    what jpeg_coefficients gives."""
    exe = _sanitized_lane_program(tmp_path)
    items = [c.data for c in rst_cases() if not c.name.endswith("_dri0")]
    items += [c.data for c in test_jpeg_io.cases() if c.readable and mrgingham_amd.jpeg_restart_intervals(c.data)[0]]
    assert len(items) >= 15 + 20
    assert _run_lane_program(exe, tmp_path, items).all()


def test_corrupted_intervals_are_accepted_exactly_when_the_host_accepts_under_sanitizers(tmp_path):
    """Seeded corruptions of the entropy-coded segment of every DRI fixture: the program fails on the first file that the
    interval-wise decode and jpeg_coefficients disagree about (acceptance, or a coefficient where both accept).  The
    corruptions must bite: the host decoder rejects between 30 % and 80 % of the flips and replacements, pooled."""
    exe = _sanitized_lane_program(tmp_path)
    kinds, items = [], []
    for c in dri_fixtures():
        made = corruptions(c)
        assert len(made) >= 801, c.name
        kinds += [k for k, _ in made]
        items += [d for _, d in made]
    accepted = _run_lane_program(exe, tmp_path, items)
    host = np.array([mrgingham_amd.jpeg_coefficients(d) is not None for d in items])
    assert np.array_equal(accepted.astype(bool), host)                    # (the sanitized build and the library agree)
    kinds = np.array(kinds)
    pooled = ~host[(kinds == "flip") | (kinds == "replace")]
    print("rejected: flips + replacements %.1f %%, truncations %.1f %%, removals %.1f %%"
          % (100 * pooled.mean(), 100 * (~host[kinds == "truncate"]).mean(), 100 * (~host[kinds == "remove"]).mean()))
    assert 0.30 <= pooled.mean() <= 0.80
    assert not host[kinds == "rst_removed"].any() and not host[kinds == "rst_exchanged"].any()
    assert (kinds == "rst_removed").sum() >= 12 and (kinds == "eoi_planted").sum() >= 12


def test_staging_images_of_the_device_decoders_under_sanitizers(tmp_path):
    """csrc/jpeg_stage.h (plan, lay out, fill) over all 16 restart fixtures and every fixture without restart intervals,
    chunked by size, and one mixed chunk: tests/boundary/jpeg_stage_main.cpp lists what it requires of every chunk."""
    from test_jpeg_sync import nodri_cases
    exe = _sanitized_lane_program(tmp_path, "jpeg_stage")
    nodri = nodri_cases()
    assert len(rst_cases()) == 16 and len(nodri) >= 30
    mixed = [rst_case("rows_48x64_420"), rst_case("nodri_48x64"), test_jpeg_io.case("progressive_48x64"), test_jpeg_io.case("noise_16x16_444")]
    items = [c.data for c in rst_cases() + nodri + mixed]
    blob = tmp_path / "corpus.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for data in items:
            f.write(struct.pack("<I", len(data)) + data)
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[0] == "mixed 0 -3 -1 -2" and lines[1] == "mixed_off -3 -3 -1 -2", r.stdout
    with_dri = sum(not c.name.endswith("_dri0") for c in rst_cases())
    words = lines[2].split()
    assert words[:2] == ["cases", str(16 + len(nodri) + 4)] and words[2] == "chunks" and int(words[3]) >= 10, r.stdout
    assert words[4:] == ["intervals", str(with_dri), "sync", str(16 - with_dri + len(nodri))], r.stdout
