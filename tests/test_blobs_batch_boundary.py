"""CPU checks of the batch blob detector's boundary: mrgingham_amd_blobs_batch and mrgingham_amd_find_circle_grids_batch
are declared, exported and bound, refuse a NULL context without writing, and nothing computes without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from mrgingham_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mrgingham_amd_blobs_batch", "mrgingham_amd_find_circle_grids_batch")


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_declared_exported_and_listed(name):
    src = open(os.path.join(ROOT, "include", "mrgingham_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(", src)
    assert name in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    L = _lib.lib()
    assert len(getattr(L, name).argtypes) == 6
    assert L.mrgingham_amd_abi_version() == 4


def test_null_context_is_an_argument_error():
    L = _lib.lib()
    fr = _lib.Frames(None, 64, 1, 8, 8, 8)
    xy = np.full((4, 2), 7, np.int32)
    counts = np.full(1, 7, np.int32)
    assert L.mrgingham_amd_blobs_batch(None, ctypes.byref(fr), xy.ctypes.data, 4, counts.ctypes.data, 1) == -1
    assert (xy == 7).all() and (counts == 7).all()
    boards = np.full((4, 2), 7.0, np.float64)
    found = np.full(1, 7, np.int8)
    assert L.mrgingham_amd_find_circle_grids_batch(None, ctypes.byref(fr), 2, boards.ctypes.data, found.ctypes.data, 1) == -1
    assert (boards == 7.0).all() and (found == 7).all()


def test_no_cpu_path_for_blobs():
    import torch
    import mrgingham_amd
    frames = torch.zeros((2, 16, 16), dtype=torch.uint8)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            mrgingham_amd.Detector()
        return
    det = mrgingham_amd.Detector(0)
    with pytest.raises(ValueError, match="on the device"):
        det.blobs(frames)                           # host tensor: refused, not computed on the CPU
    det.close()
