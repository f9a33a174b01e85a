"""CPU checks of the 16-bit batch preprocessing's boundary: mrgingham_amd_preprocess16_batch is declared, exported and
bound, and nothing computes without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from mrgingham_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mrgingham_amd_preprocess16_batch"


def test_symbol_is_declared_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "mrgingham_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", src)
    assert NAME in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    L = _lib.lib()
    assert len(getattr(L, NAME).argtypes) == 11
    assert L.mrgingham_amd_abi_version() == 4


def test_null_context_is_an_argument_error():
    L = _lib.lib()
    out = np.full(64, 7, np.uint8)
    img = np.zeros(64, np.uint16)
    assert getattr(L, NAME)(None, img.ctypes.data, 64, 1, 8, 8, 8, 1, 1, out.ctypes.data, None) == -1
    assert (out == 7).all()


def test_no_cpu_path_for_16_bit_frames():
    import torch
    import mrgingham_amd
    frames = torch.zeros((2, 16, 16), dtype=torch.uint16)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            mrgingham_amd.Detector()
        return
    det = mrgingham_amd.Detector(0)
    with pytest.raises(ValueError, match="on the device"):
        det.preprocess(frames)                      # host tensor: refused, not computed on the CPU
    det.close()
