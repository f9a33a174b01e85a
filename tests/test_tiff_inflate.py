"""The Deflate strip decoder of csrc/tiff_inflate.h against zlib, without a GPU: the shared text through both table
arrangements in a stand-alone program under the address and undefined-behaviour sanitizers, over good, crafted, broken and
mutated streams (tests/tiff_inflate_cases.py: the lists the device tests use too); tiff_layout's Deflate limit; the loader
flag of find_boards_files_ex3; the tool's argument errors."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import mrgingham_amd
from tests import files_cases
from tests import tiff_cases as tc
from tests import tiff_inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrgingham_amd", "csrc")
CLI = os.path.join(ROOT, "mrgingham_amd", "bin", "mrgingham-amd-from-image")


def test_zlib_is_the_judge_of_the_crafted_lists(tmp_path):
    """read_image -- zlib's uncompress -- reads the file around every crafted accepted stream to the bytes it was made
    for, and gives None for the file around every broken one."""
    p = tmp_path / "case.tif"
    for name, (stream, data, shape) in ic.crafted_accepted().items():
        p.write_bytes(ic.craft_file(stream, shape))
        got = mrgingham_amd.read_image(str(p))
        assert got is not None and got.tobytes() == data, name
    broken = ic.broken_streams()
    assert len(broken) == 23 and len(ic.crafted_accepted()) == 10
    for name, stream in broken.items():
        p.write_bytes(ic.craft_file(stream))
        assert mrgingham_amd.read_image(str(p)) is None, name
        assert mrgingham_amd.probe_image(str(p)) is not None, name   # (the directory is fine: only decoding finds it)


def walked():
    """The walker over a part of the good streams (one raw stream per payload and kind of compressor) and the crafted ones."""
    infos = []
    for data in ic.payloads():
        for level, strategy in ((0, ic.STRATEGIES[0]), (6, ic.STRATEGIES[0]), (9, ic.STRATEGIES[0]), (6, ic.STRATEGIES[3]), (6, ic.STRATEGIES[4])):
            info = ic.walk(ic.deflate(data, level, strategy, raw=True), raw=True)
            assert info["out"] == data
            infos.append(info)
    for name, (stream, data, _) in ic.crafted_accepted().items():
        info = ic.walk(stream)
        assert info["out"] == data, name
        infos.append(info)
    return infos


def test_the_corpus_has_every_block_kind_and_the_long_and_far_matches():
    infos = walked()
    assert set().union(*(i["kinds"] for i in infos)) == {0, 1, 2}
    assert set().union(*(i["repeats"] for i in infos)) == {16, 17, 18}
    assert max(i["max_length"] for i in infos) == 258
    assert max(i["max_distance"] for i in infos) > 32000
    assert any(i["overlap"] for i in infos)


def test_both_table_arrangements_against_zlib_under_sanitizers(tmp_path):
    """tests/boundary/tiff_inflate_fuzz_main.cpp built with -fsanitize=address,undefined and run as a child process: per
    stream zlib's verdict, the shared text's with the host's table and with the kernel's strided one, stream and outputs in
    heap blocks of exactly their sizes.  The program fails on the first unequal verdict or byte; here: every good and
    crafted accepted stream is accepted, every broken one refused, and of the mutated ones zlib accepts at least a quarter
    and refuses at least a quarter (with seed 11: 983 and 1017 of 2000)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the sanitizer runtime of g++ is not installed")
    exe = str(tmp_path / "tiff_inflate_fuzz")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "boundary", "tiff_inflate_fuzz_main.cpp"),
                        "-lz", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    good = ic.good_streams()
    assert len(good) == 5 * 4 * 5 * 2
    accepted, broken = ic.crafted_accepted(), ic.broken_streams()
    mutated = ic.mutations([g for g in good if g[1]])
    ncraft = len(ic.craft_payload())
    items = [(s, raw, len(data)) for s, raw, data in good]
    items += [(s, False, len(data)) for s, data, _ in accepted.values()]
    items += [(s, False, ncraft) for s in broken.values()]
    items += [(s, raw, len(data)) for s, raw, data in mutated]
    blob = tmp_path / "corpus.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for s, raw, nout in items:
            f.write(struct.pack("<III", int(raw), nout, len(s)) + s)
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-200:], r.stderr[-4000:])
    v = r.stdout.strip()
    assert len(v) == len(items)
    a, b, c = len(good), len(good) + len(accepted), len(good) + len(accepted) + len(broken)
    assert v[:a] == "A" * len(good)
    assert v[a:b] == "A" * len(accepted), dict(zip(accepted, v[a:b]))
    assert v[b:c] == "R" * len(broken), dict(zip(broken, v[b:c]))
    took, refused = v[c:].count("A"), v[c:].count("R")
    print(f"mutated streams: zlib accepts {took}, refuses {refused} of {len(mutated)}")
    assert len(mutated) == 2000 and took + refused == 2000
    assert 4 * took >= len(mutated) and 4 * refused >= len(mutated)


def test_layout_takes_deflate_files_from_their_strip_size_on():
    img = ic.ramp_noise(11, 37)
    for comp in (tc.ADOBE_DEFLATE, tc.DEFLATE):
        data, strips = tc.encode(img, compression=comp, rows_per_strip=3, predictor=2)
        plain = mrgingham_amd.tiff_layout(data)
        assert plain is not None and plain.rc == mrgingham_amd.TIFF_NOT_TAKEN and not plain.taken
        zero = mrgingham_amd.tiff_layout(data, deflate_max_strip=0)
        assert zero.rc == plain.rc and zero.key() == plain.key() and np.array_equal(zero.strips, plain.strips)
        for limit, taken in ((3 * 37 - 1, False), (3 * 37, True), (3 * 37 + 1, True), (1 << 20, True), (1 << 30, True), (1, False)):
            lay = mrgingham_amd.tiff_layout(data, deflate_max_strip=limit)
            assert lay.taken == taken and lay.rc == (0 if taken else mrgingham_amd.TIFF_NOT_TAKEN), (comp, limit)
            assert lay.key() == plain.key() and lay.compression == comp
            assert [tuple(int(x) for x in s) for s in lay.strips] == strips
    # the Deflate limit changes nothing for the other schemes
    for comp, taken in ((tc.NONE, True), (tc.LZW, True), (tc.PACKBITS, False)):
        data, _ = tc.encode(img, compression=comp, rows_per_strip=3)
        assert mrgingham_amd.tiff_layout(data, deflate_max_strip=1 << 20).taken == taken
    # a strip above 1 MiB is never taken
    big = np.zeros((1025, 1024), np.uint8)
    data, _ = tc.encode(big, compression=tc.ADOBE_DEFLATE)
    assert not mrgingham_amd.tiff_layout(data, deflate_max_strip=1 << 30).taken
    assert mrgingham_amd.tiff_layout(tc.encode(big[:1024], compression=tc.ADOBE_DEFLATE)[0], deflate_max_strip=1 << 30).taken


def test_layout_leaves_a_strip_of_more_bytes_than_any_zlib_stream_needs_to_the_host(tmp_path):
    """A block need not give a byte, so a lane's work goes with the strip's bytes in the file: a strip that gives its rows and
    then runs through thousands of empty blocks is a stream zlib accepts -- read_image reads the file -- and the device
    route does not take it, whatever the Deflate limit; with a run that stays within the byte limit it does."""
    w, h = ic.CRAFT_SHAPE
    img = ic.ramp_noise(h, w)
    for blocks, taken in ((700, True), (6000, False)):
        stream = ic.with_empty_blocks(img.tobytes(), blocks)
        assert (len(stream) <= ic.max_bytes(w * h)) == taken
        data = ic.craft_file(stream)
        p = tmp_path / "blocks.tif"
        p.write_bytes(data)
        assert np.array_equal(mrgingham_amd.read_image(str(p)), img)
        for limit in (w * h, 1 << 20):
            lay = mrgingham_amd.tiff_layout(data, deflate_max_strip=limit)
            assert lay is not None and lay.taken == taken and lay.rc == (0 if taken else mrgingham_amd.TIFF_NOT_TAKEN), (blocks, limit)
    # the limit to the byte: decoded + decoded / 8 + 512
    good = ic.deflate(img.tobytes())
    for extra, taken in ((0, True), (1, False)):
        stream = good + bytes(ic.max_bytes(w * h) - len(good) + extra)
        assert mrgingham_amd.tiff_layout(ic.craft_file(stream), deflate_max_strip=1 << 20).taken == taken


def test_files_ex3_takes_the_deflate_flag_only_with_the_tiff_flag():
    """With no files the call returns before it needs a device."""
    from mrgingham_amd import _lib
    L = _lib.lib()
    o = _lib.FilesOptions(1, 1, 10, -1, 1, 0, 0, 0, -1)
    seen = []
    cb = _lib.PROGRESS_F(lambda n, cookie: seen.append(n))

    def ex3(flags):
        return L.mrgingham_amd_find_boards_files_ex3(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, flags)
    fine = list(range(8)) + [12, 13, 14, 15]
    for flags in fine:
        assert ex3(flags) == 0, flags
    assert seen == [0] * len(fine)
    for flags in (8, 9, 10, 11, 16):
        assert ex3(flags) == -1, flags
    assert L.mrgingham_amd_find_boards_files_ex2(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, 8) == -1
    assert L.mrgingham_amd_find_boards_files_ex2(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, 12) == -1
    lanes = L.mrgingham_amd_tiff_inflate_lanes()
    assert lanes >= 64 and lanes % 64 == 0
    assert L.mrgingham_amd_abi_version() == 4


def test_find_boards_files_refuses_deflate_device_without_tiff_device():
    with pytest.raises(ValueError):
        mrgingham_amd.find_boards_files([], tiff_deflate="device")
    with pytest.raises(ValueError):
        mrgingham_amd.find_boards_files([], tiff="device", tiff_deflate="gpu")


def test_tool_argument_errors_need_no_device(tmp_path):
    img = tmp_path / "a.pgm"
    files_cases.write_pgm(img, np.zeros((32, 32), np.uint8))
    for args, message in ((("--tiff-deflate", "device"), "--tiff-deflate is only accepted with --batch"),
                          (("--batch", "4", "--tiff-deflate", "device"), "--tiff-deflate device is only accepted with --tiff-lzw device"),
                          (("--batch", "4", "--tiff-lzw", "host", "--tiff-deflate", "device"),
                           "--tiff-deflate device is only accepted with --tiff-lzw device"),
                          (("--batch", "4", "--tiff-lzw", "device", "--tiff-deflate", "gpu"), "--tiff-deflate takes 'host' or 'device'")):
        r = subprocess.run([CLI, *args, str(img)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and message in r.stderr, (args, r.returncode, r.stderr)
        assert r.stdout == ""
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--tiff-deflate host|device" in r.stdout
