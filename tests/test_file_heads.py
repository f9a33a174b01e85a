"""What the host readers must agree on whoever reads a file's front (csrc/image_io.cpp), no GPU: probe_image's kind of one small
file per format is the named constant, and a PGM or PAM file whose samples a comment pushes to byte 4095, 4096, 4097 or
8193 -- around the 4096 bytes a reader holds first, behind twice as many -- reads exactly as the file without the comment
does.  Every check is an equality."""
import os
import re

import numpy as np
import pytest

import mrgingham_amd
from tests import files_cases, head_cases, tiff_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("PGM", "PNG", "JPEG", "TIFF", "BMP", "PNM")


def test_kind_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "mrgingham_amd.h")).read()
    defined = dict(re.findall(r"^#define MRGINGHAM_AMD_KIND_(\w+) (\d+)$", text, flags=re.M))
    assert defined == {name: str(i + 1) for i, name in enumerate(KINDS)}
    for name, value in defined.items():
        assert getattr(mrgingham_amd, "KIND_" + name) == int(value)


def test_probe_image_reports_the_named_kind_of_every_format(tmp_path):
    img = np.arange(12 * 9, dtype=np.uint8).reshape(9, 12)
    jpeg = next(data for _, data, readable, _, _ in files_cases.golden_jpegs() if readable)
    files = {"PGM": head_cases.pgm(8)[0], "PNM": head_cases.pam(8)[0], "BMP": head_cases.bmp24()[0], "JPEG": jpeg,
             "TIFF": tiff_cases.encode(img)[0]}
    files_cases.write_png(str(tmp_path / "PNG"), img)
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    for name in KINDS:
        probe = mrgingham_amd.probe_image(str(tmp_path / name))
        assert probe is not None and probe[3] == getattr(mrgingham_amd, "KIND_" + name), name
        assert mrgingham_amd.read_image(str(tmp_path / name)).shape == probe[:2], name


@pytest.mark.parametrize("bits", (8, 16))
@pytest.mark.parametrize("write", (head_cases.pgm, head_cases.pam), ids=("pgm", "pam"))
def test_a_padded_header_reads_as_the_plain_one(tmp_path, write, bits):
    def three(data, name):
        path = tmp_path / name
        path.write_bytes(data)
        head = (mrgingham_amd.pgm_header if write is head_cases.pgm else mrgingham_amd.pnm_header)(data)
        assert head is not None and head != mrgingham_amd.PGM_HEADER_CUT, name
        return mrgingham_amd.read_image(str(path)), mrgingham_amd.probe_image(str(path)), head

    data, off = write(bits)
    img, probe, head = three(data, "plain")
    kind = mrgingham_amd.KIND_PGM if write is head_cases.pgm else mrgingham_amd.KIND_PNM
    want = head_cases.grey(bits, 1 if write is head_cases.pgm else head_cases.PAM[bits][0])
    assert img is not None and np.array_equal(img, want if bits == 8 else (want >> 8).astype(np.uint8))   # (16 bit: the high bytes)
    assert probe == (head_cases.H, head_cases.W, bits, kind)
    if write is head_cases.pgm:
        assert head == (head_cases.H, head_cases.W, bits, off)
    fields = [n for n in mrgingham_amd.PnmHeader.FIELDS if n != "payload_offset"]
    for start in head_cases.STARTS:
        padded, at = write(bits, start)
        assert at == start and padded[at:] == data[off:]
        pimg, pprobe, phead = three(padded, f"padded{start}")
        assert pimg is not None and np.array_equal(pimg, img), start
        assert pprobe == probe, start
        if write is head_cases.pgm:
            assert phead == head[:3] + (start,), start
        else:
            assert phead.payload_offset == start and [getattr(phead, n) for n in fields] == [getattr(head, n) for n in fields], start
        # a file one byte short of its raster is unreadable to both, wherever the raster begins
        (tmp_path / "short").write_bytes(padded[:-1])
        assert mrgingham_amd.read_image(str(tmp_path / "short")) is None and mrgingham_amd.probe_image(str(tmp_path / "short")) is None, start
