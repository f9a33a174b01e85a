"""The batch loaders that read a file's front themselves (Detector.read_pgms, read_pnms, read_bmps) on files whose
raster begins around the 4096 bytes held first (tests/head_cases.py): 17 x 5 PGM and PAM files with the samples at byte
4095, 4096, 4097 and 8193, a 40 x 35 24-bit BMP whose pixel array crosses byte 4096.  Alone and in a list with plain files
and files one byte short of their raster.  The yardstick is read_image on the same file -- of a 16-bit file its high
bytes, so those frames are also held against the samples the file was written from; np.array_equal, no tolerance."""
import numpy as np
import pytest

import mrgingham_amd
from tests import bmp_cases, head_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector()
    yield d
    d.close()


def _load(read, tmp_path, files, dtype):
    """files: [(label, bytes, the grey it reads to or None for a file that is unreadable)] through `read`: status 0 and
    read_image's frame, or status -1 and a zero frame"""
    names = []
    for label, data, _ in files:
        names.append(str(tmp_path / label))
        with open(names[-1], "wb") as f:
            f.write(data)
    frames, status = read(names)
    got = frames.cpu().numpy()
    shape = next(want.shape for _, _, want in files if want is not None)
    assert got.dtype == dtype and got.shape == (len(files),) + shape
    assert status.tolist() == [0 if want is not None else -1 for _, _, want in files]
    for f, (label, _, want) in enumerate(files):
        img = mrgingham_amd.read_image(names[f])
        if want is None:
            assert img is None and not got[f].any(), label
        else:
            assert np.array_equal(got[f] >> 8 if dtype == np.uint16 else got[f], img) and np.array_equal(got[f], want), label


@pytest.mark.parametrize("bits", (8, 16))
@pytest.mark.parametrize("loader", ("pgms", "pnms_pgm", "pnms_pam"))
def test_netpbm_rasters_around_the_head(det, tmp_path, loader, bits):
    write = head_cases.pam if loader == "pnms_pam" else head_cases.pgm
    read = det.read_pgms if loader == "pgms" else det.read_pnms
    want = head_cases.grey(bits, head_cases.PAM[bits][0] if loader == "pnms_pam" else 1)
    dtype = np.uint8 if bits == 8 else np.uint16
    padded = [(f"at{start}", write(bits, start)[0], want) for start in head_cases.STARTS]
    for k, one in enumerate(padded):
        (tmp_path / f"alone{k}").mkdir()
        _load(read, tmp_path / f"alone{k}", [one], dtype)
    plain = write(bits)[0]
    mixed = [("plain", plain, want)]
    for label, data, _ in padded:
        mixed += [(label, data, want), (label + "_short", data[:-1], None)]
    mixed += [("plain_short", plain[:-1], None), ("plain_again", plain, want)]
    _load(read, tmp_path, mixed, dtype)


def test_a_bmp_whose_pixel_array_crosses_the_head(det, tmp_path):
    data, _, want = head_cases.bmp24()
    (tmp_path / "alone").mkdir()
    _load(det.read_bmps, tmp_path / "alone", [("crossing", data, want)], np.uint8)
    # with a file whose array lies inside the head (8 bit, a palette), and both a byte short of their arrays
    pixels, palette = bmp_cases.random_pixels(40, 35, 8, seed=4), bmp_cases.random_palette(256, seed=5)
    inside = bmp_cases.write(pixels, 8, palette)
    assert len(inside) < 4096
    _load(det.read_bmps, tmp_path, [("inside", inside, bmp_cases.expected(pixels, 8, palette)), ("crossing", data, want),
                                    ("crossing_short", data[:-1], None), ("inside_short", inside[:-1], None),
                                    ("crossing_again", data, want)], np.uint8)
