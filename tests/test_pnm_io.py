"""The host reader of binary PBM and PAM files (read_image, probe_image, pnm_header; csrc/image_io.cpp,
csrc/pnm_pixels.h), no GPU: files written by the writer of tests/pnm_cases.py and by Pillow (tests/golden/pnm_golden.npz)
against the arrays they were written from through the library's grey weights, the header grammar, one broken rule per
file, and the whole corpus and the pixel text through a stand-alone program under the address and undefined-behaviour
sanitizers.  Netpbm is lossless and the grey is integer arithmetic: no tolerance anywhere.

The host interface hands out 8 bits of a 16-bit file: its high byte, or with cli_scaling round(v * 255 / 65535).  Both are
compared here; the 16-bit samples themselves are compared on the device (tests/test_gpu_pnm.py) and inside the sanitizer
program, which holds read_image's uint16 samples against the pixel text at every phase."""
import ctypes
import io
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import mrgingham_amd
from mrgingham_amd import _lib
from tests import pnm_cases as pc
from tests.test_pgm_header import _cases as pgm_cases
from tests.host_program import build_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT = mrgingham_amd.PGM_HEADER_CUT


def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "pnm_golden.npz"))
    for i, name in enumerate(g["name"]):
        rgb = g[f"img_{i}"]
        yield str(name), g[f"pnm_{i}"].tobytes(), rgb


def read_all_three(tmp_path, data):
    """-> (read_image's array or None, probe_image's tuple or None, pnm_header's result: None where it calls the bytes
    unreadable or cut)"""
    path = str(tmp_path / "case.pnm")
    with open(path, "wb") as f:
        f.write(data)
    head = mrgingham_amd.pnm_header(data)
    return mrgingham_amd.read_image(path), mrgingham_amd.probe_image(path), None if head is None or head == CUT else head


def to_8bit(want, cli_scaling=False):
    if want.dtype == np.uint8:
        return want
    if cli_scaling:
        return np.rint(want.astype(np.float64) * (255. / 65535.)).astype(np.uint8)
    return (want >> 8).astype(np.uint8)


def assert_reads_to(tmp_path, data, want, what, **fields):
    img, probe, head = read_all_three(tmp_path, data)
    assert img is not None and probe is not None and head is not None, what
    depth = 16 if want.dtype == np.uint16 else 8
    h, w = want.shape
    assert probe == (h, w, depth, 6), what
    assert img.dtype == np.uint8 and np.array_equal(img, to_8bit(want)), what
    if depth == 16:
        assert np.array_equal(mrgingham_amd.read_image(str(tmp_path / "case.pnm"), cli_scaling=True), to_8bit(want, True)), what
    assert (head.height, head.width, head.depth) == (h, w, depth), what
    assert head.row_bytes == pc.row_bytes(w, head.bits, head.channels) and head.payload_offset + head.row_bytes * h <= len(data), what
    for name, v in fields.items():
        assert getattr(head, name) == int(v), (what, name)
    return head


@pytest.mark.parametrize("layout", pc.LAYOUTS, ids=pc.LAYOUT_IDS)
def test_every_width_and_height(tmp_path, layout):
    """widths 1 .. 40 x heights 1 .. 3: at P4 every bit phase and the padded last byte, elsewhere rows that begin at every
    byte phase"""
    _, magic, bits, ch, bw = layout
    for w, h in itertools.product(range(1, 41), (1, 2, 3)):
        data, want, _ = pc.write_layout(layout, w, h, seed=100 * w + h)
        head = assert_reads_to(tmp_path, data, want, (w, h), magic=magic, bits=bits, channels=ch, black_and_white=bw)
        assert head.payload_offset == len(data) - pc.row_bytes(w, bits, ch) * h


def test_maxvals_are_never_rescaled(tmp_path):
    """maxval 1, 255, 256 and 65535: below 256 one byte per sample, from 256 on big-endian pairs, the samples as they are"""
    for maxval, bits in ((1, 8), (200, 8), (255, 8), (256, 16), (4095, 16), (65535, 16)):
        for magic, ch in ((7, 1), (7, 2), (7, 3), (7, 4)):
            s = pc.random_samples(9, 3, bits, ch, seed=maxval + ch, maxval=maxval)
            s[0, 0, :], s[-1, -1, :] = maxval, 0
            assert s.max() == maxval
            head = assert_reads_to(tmp_path, pc.write(s, magic, bits, maxval=maxval), pc.expected(s, bits, ch), (maxval, magic, ch), bits=bits)
            assert head.black_and_white == 0
    # a PAM of maxval 1 without the BLACKANDWHITE tuple type: plain samples 0 and 1
    s = pc.random_samples(9, 3, 8, 1, bw=True, seed=5)
    data = pc.write(s, 7, 8, head=pc.pam_head(9, 3, 1, 1, "GRAYSCALE"))
    assert assert_reads_to(tmp_path, data, s[..., 0], "maxval 1, grey").black_and_white == 0
    assert assert_reads_to(tmp_path, pc.write(s, 7, 8, bw=True), s[..., 0] * 255, "maxval 1, black and white").black_and_white == 1


def test_black_and_white_reads_non_zero_as_white(tmp_path):
    """(a sample above maxval is the writer's mistake; it is non-zero all the same)"""
    s = pc.random_samples(17, 3, 8, 2, bw=True, seed=6)
    s[0, 0, 0], s[1, 5, 0], s[..., 1] = 7, 255, 0
    want = np.where(s[..., 0] != 0, 255, 0).astype(np.uint8)
    assert want[0, 0] == 255 and want[1, 5] == 255
    assert_reads_to(tmp_path, pc.write(s, 7, 8, bw=True), want, "bw alpha", channels=2, black_and_white=1)
    # the first TUPLTYPE decides; a later one is not judged
    head = pc.pam_head(17, 3, 2, 1, None, extra=(b"TUPLTYPE BLACKANDWHITE", b"TUPLTYPE _ALPHA"))
    assert_reads_to(tmp_path, pc.write(s, 7, 8, head=head), want, "two tuple types", black_and_white=1)
    head = pc.pam_head(17, 3, 2, 1, None, extra=(b"TUPLTYPE GRAYSCALE", b"TUPLTYPE BLACKANDWHITE"))
    assert_reads_to(tmp_path, pc.write(s, 7, 8, head=head), s[..., 0], "the second does not count", black_and_white=0)


def test_p4_bits_and_the_padded_last_byte(tmp_path):
    """bit 1 is black; the unused bits of a row's last byte are set in the writer's files and never read as pixels"""
    s = np.zeros((2, 11, 1), np.uint8)
    s[0, ::2, 0], s[1, -1, 0] = 1, 1
    data = pc.write(s, 4, 1)
    assert data == b"P4\n11\n2\n" + bytes([0b10101010, 0b10111111, 0b00000000, 0b00111111])
    want = np.full((2, 11), 255, np.uint8)
    want[0, ::2], want[1, -1] = 0, 0
    assert_reads_to(tmp_path, data, want, "bits", magic=4, bits=1, channels=1, row_bytes=2)


def test_pure_colours_and_the_weights(tmp_path):
    assert 4899 + 9617 + 1868 == 1 << 14
    v = np.arange(0, 65536, 257)
    assert np.array_equal(pc.grey(v, v, v), v)                           # (grey in all three channels reads back exactly)
    for bits, top in ((8, 255), (16, 65535)):
        s = np.zeros((1, 3, 3), np.uint16 if bits == 16 else np.uint8)
        s[0, 0, 0], s[0, 1, 1], s[0, 2, 2] = top, top, top
        want = pc.expected(s, bits, 3)
        assert want[0].tolist() == ([76, 150, 29] if bits == 8 else [int(pc.grey(top, 0, 0)), int(pc.grey(0, top, 0)), int(pc.grey(0, 0, top))])
        assert_reads_to(tmp_path, pc.write(s, 7, bits), want, bits)
        rgba = np.concatenate([s, np.full((1, 3, 1), top // 3, s.dtype)], axis=-1)
        assert_reads_to(tmp_path, pc.write(rgba, 7, bits), want, bits)       # alpha is ignored


HEADS_P4 = [b"P4\n11 3\n", b"P4 11 3 ", b"P4\n#c\n11\t3\r", b"P4 # one\n# two\n11 #w\n3\n", b"P411 3\n", b"P4\t11\r\n3\n", b"P4\n\n11 3\t",
            b"P4 # one\n# two.\n11\t3\n"]


def test_header_grammar_of_p4(tmp_path):
    bits = pc.random_samples(11, 3, 1, 1, seed=2)
    for head in HEADS_P4:
        h = assert_reads_to(tmp_path, pc.write(bits, 4, 1, head=head), pc.expected(bits, 1, 1), head)
        assert h.payload_offset == len(head)
    # ONE white-space byte follows the last number: a second one is the first byte of the raster
    data = b"P4\n8 1\n" + b"\n"
    assert_reads_to(tmp_path, data + bytes(8), np.array([[255, 255, 255, 255, 0, 255, 0, 255]], np.uint8), "white space as raster")
    # trailing bytes are ignored
    assert_reads_to(tmp_path, pc.write(bits, 4, 1) + b"P4 and more", pc.expected(bits, 1, 1), "trailing")


def test_header_grammar_of_p7(tmp_path):
    s = pc.random_samples(5, 3, 16, 4, seed=3)
    want = pc.expected(s, 16, 4)
    fields = ("WIDTH", "HEIGHT", "DEPTH", "MAXVAL")
    for order in itertools.permutations(fields):
        assert_reads_to(tmp_path, pc.write(s, 7, 16, head=pc.pam_head(5, 3, 4, 65535, "RGB_ALPHA", order=order)), want, order)
    heads = [
        pc.pam_head(5, 3, 4, 65535, None),                                                            # no TUPLTYPE at all
        pc.pam_head(5, 3, 4, 65535, "RGB_ALPHA", extra=(b"TUPLTYPE RGB", b"TUPLTYPE anything at all")),
        pc.pam_head(5, 3, 4, 65535, "RGB_ALPHA", extra=(b"# a comment", b"", b"#", b"   ", b"# WIDTH 9")),
        b"P7\nWIDTH\t5\nHEIGHT   3  \nDEPTH 4\r\nMAXVAL 65535\nTUPLTYPE\nENDHDR\n",
        b"P7\r\n\n# ENDHDR\nMAXVAL 65535\nDEPTH 4\nHEIGHT 3\nWIDTH 5\nENDHDR \n",
    ]
    for head in heads:
        h = assert_reads_to(tmp_path, pc.write(s, 7, 16, head=head), want, head, channels=4, bits=16)
        assert h.payload_offset == len(head)
    # a raster that begins with a newline byte: it begins right behind ENDHDR's own
    g = np.full((1, 3, 1), 10, np.uint8)
    assert_reads_to(tmp_path, pc.write(g, 7, 8), np.full((1, 3), 10, np.uint8), "newlines as samples")


def test_pnm_header_on_p5_is_pgm_header(tmp_path):
    """every case of tests/test_pgm_header.py: the same verdict, the same numbers; read_image and probe_image (kind 1) are
    not touched"""
    n = 0
    for label, (data, _) in pgm_cases(tmp_path).items():
        for part in (data, data[:4096]):
            a, b = mrgingham_amd.pgm_header(part), mrgingham_amd.pnm_header(part)
            if data[:2] != b"P5":
                assert a is None, label
                continue
            if a is None or a == CUT:
                assert b == a, label
            else:
                assert (b.height, b.width, b.bits, b.payload_offset) == a, label
                assert (b.magic, b.channels, b.black_and_white, b.row_bytes, b.depth) == (5, 1, 0, a[1] * a[2] // 8, a[2]), label
                n += 1
    assert n >= 24
    # and mrgingham_amd_pgm_header goes on refusing every other magic
    for layout in pc.LAYOUTS:
        assert mrgingham_amd.pgm_header(pc.write_layout(layout, 5, 3)[0]) is None


def test_a_header_longer_than_the_probe_reads(tmp_path):
    bits = pc.random_samples(11, 3, 1, 1, seed=2)
    head = b"P4\n#" + b"c" * 6000 + b"\n11 3\n"
    assert_reads_to(tmp_path, pc.write(bits, 4, 1, head=head), pc.expected(bits, 1, 1), "long comment")
    assert mrgingham_amd.pnm_header(pc.write(bits, 4, 1, head=head)[:4096]) == CUT
    assert read_all_three(tmp_path, pc.write(bits, 4, 1, head=head)[:-1]) == (None, None, None)
    s = pc.random_samples(5, 3, 16, 4, seed=3)
    head = pc.pam_head(5, 3, 4, 65535, "RGB_ALPHA", extra=[b"# line %d" % i for i in range(900)])
    assert len(head) > 2 * 4096
    assert_reads_to(tmp_path, pc.write(s, 7, 16, head=head), pc.expected(s, 16, 4), "many comments")
    head = b"P4 " + b"#x\n" * 3000 + b"11 3\n"
    assert_reads_to(tmp_path, pc.write(bits, 4, 1, head=head), pc.expected(bits, 1, 1), "many short comments")
    # a long raster behind a short header: probe_image sees a byte that is missing from the size alone
    big = pc.random_samples(130, 65, 8, 3, seed=4)
    data = pc.write(big, 7, 8)
    assert len(data) > 2 * 4096
    assert_reads_to(tmp_path, data, pc.expected(big, 8, 3), "long")
    assert read_all_three(tmp_path, data[:-1]) == (None, None, None)


def test_pillow_written_files_read_to_their_arrays(tmp_path):
    cases = list(golden())
    assert len(cases) >= 4 and {n.split("_")[0] for n, _, _ in cases} == {"1"}
    for name, data, rgb in cases:
        want = pc.grey(rgb[..., 0], rgb[..., 1], rgb[..., 2]).astype(np.uint8)
        head = assert_reads_to(tmp_path, data, want, name)
        assert head.magic == 4, name


def test_pillow_writes_what_the_library_reads_and_reads_what_the_writer_writes(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for w, h in ((1, 1), (7, 2), (8, 3), (17, 5), (33, 5), (65, 2)):
        im = Image.fromarray(rng.integers(0, 2, (h, w)).astype(bool))
        buf = io.BytesIO()
        im.save(buf, "PPM")
        rgb = np.asarray(im.convert("RGB"))
        assert buf.getvalue()[:2] == b"P4"
        assert_reads_to(tmp_path, buf.getvalue(), pc.grey(rgb[..., 0], rgb[..., 1], rgb[..., 2]).astype(np.uint8), (w, h))
        # the writer's P4 files through Pillow's decoder (Pillow reads no PAM)
        for layout in pc.LAYOUTS[:1]:
            data, want, _ = pc.write_layout(layout, w, h, seed=w)
            rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
            assert np.array_equal(pc.grey(rgb[..., 0], rgb[..., 1], rgb[..., 2]).astype(np.uint8), want), (layout[0], w, h)


def test_broken_files_are_unreadable_by_all_three(tmp_path):
    broken, goods = pc.broken_files()
    for good in goods:
        assert all(x is not None for x in read_all_three(tmp_path, good))
    assert len(broken) >= 40
    for name, data in broken.items():
        assert read_all_three(tmp_path, data) == (None, None, None), name
    cuts = pc.header_cuts()
    assert len(cuts) > 100
    for name, data in cuts.items():
        assert read_all_three(tmp_path, data) == (None, None, None), name
    # bytes that end inside a header ask for more; the whole header without a raster is a file too short
    for kind, head in (("p4", b"P4\n# bits\n11 3\n"), ("p4b", b"P4 # packed\n11\t# deep\n300\n")):
        for cut in range(2, len(head)):
            assert mrgingham_amd.pnm_header(head[:cut]) == CUT, (kind, cut)
        assert mrgingham_amd.pnm_header(head) is None


def test_files_ex5_takes_the_pnm_flag_and_files_ex4_goes_on_refusing_it():
    """With no files the call returns before it needs a device: flags 0 .. 63 are fine for _ex5 (Deflate only with TIFF), 64
    is not; _ex4 refuses 32."""
    L = _lib.lib()
    o = _lib.FilesOptions(1, 1, 10, -1, 1, 0, 0, 0, -1)
    cb = _lib.PROGRESS_F(lambda n, cookie: None)
    for flags in range(130):
        want = 0 if flags < 64 and not (flags & 8 and not flags & 4) else -1
        assert L.mrgingham_amd_find_boards_files_ex5(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, flags) == want, flags
    for flags in (32, 33, 36, 63):
        assert L.mrgingham_amd_find_boards_files_ex4(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, flags) == -1
    assert L.mrgingham_amd_find_boards_files_ex4(None, 0, ctypes.byref(o), None, None, None, None, cb, None, None, 0, 31) == 0
    with pytest.raises(ValueError, match='pnm is "host" or "device"'):
        mrgingham_amd.find_boards_files([], pnm="both")
    assert L.mrgingham_amd_abi_version() == 4


def test_geometry_is_exported():
    lanes, per_cu = mrgingham_amd.pnm_unpack_geometry()
    assert lanes == 256 and per_cu == 8


def corpus():
    """Good files, broken files and seeded byte mutations and truncations of both."""
    items = [d for _, d, _ in golden()]
    for k, layout in enumerate(pc.LAYOUTS):
        for w, h in ((1, 1), (7, 3), (17 + k, 3), (33, 2), (9, 2), (40 - k, 1)):
            items.append(pc.write_layout(layout, w, h, seed=k)[0])
    items += [pc.write(pc.random_samples(11, 3, 1, 1, seed=2), 4, 1, head=h) for h in HEADS_P4]
    items.append(b"P5\n7 3\n255\n" + bytes(range(21)))
    items.append(b"P5\n7 3\n65535\n" + bytes(range(42)))
    broken, goods = pc.broken_files()
    items += goods + [d for d in broken.values() if len(d) < 5000] + list(pc.header_cuts().values())[::7]
    rng = np.random.default_rng(23)
    mutated = []
    for data in items:
        if not data:
            continue
        for _ in range(20):
            b = bytearray(data)
            for _ in range(int(rng.integers(1, 4))):
                # (mostly in the header, where every byte is a rule)
                at = int(rng.integers(0, min(len(b), 70))) if rng.integers(0, 4) else int(rng.integers(0, len(b)))
                b[at] = int(rng.integers(0, 256)) if rng.integers(0, 2) else int(rng.choice(list(b"0123456789 \n#P")))
            mutated.append(bytes(b))
        mutated.append(data[:int(rng.integers(1, len(data) + 1))])
    return items + mutated


def test_corpus_and_pixel_text_under_address_and_undefined_sanitizers(tmp_path):
    """The corpus through the host readers (tests/host_program.py) built with -fsanitize=address,undefined into a stand-alone program
    (tests/boundary/pnm_fuzz_main.cpp), run as a child process: read_image, probe_image and pnm_header on every case, and
    pnm_pixels.h on rasters held in heap buffers of exactly the payload's padded size."""
    exe = build_sanitized(tmp_path, "pnm_fuzz_main.cpp")
    items = corpus()
    assert len(items) > 2000
    blob = tmp_path / "corpus.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for data in items:
            f.write(struct.pack("<I", len(data)) + data)
    scratch = tmp_path / "scratch.pnm"
    want_readable = 0
    for d in items:
        head = mrgingham_amd.pnm_header(d)
        want_readable += d[:2] in (b"P4", b"P7") and len(d) >= 8 and head is not None and head != CUT
    r = subprocess.run([exe, str(blob), str(scratch)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    words = r.stdout.split()
    assert words[:4] == ["cases", str(len(items)), "readable", str(want_readable)], r.stdout
    assert want_readable > 300 and int(words[5]) > 1000         # (rows walked through the pixel text, at every phase each)
