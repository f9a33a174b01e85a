"""The tool's --batch mode, the part that needs no GPU: the usage text, and the argument errors, which are reported
before the device count is asked for."""
import os
import subprocess

import numpy as np

from tests import files_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mrgingham_amd", "bin", "mrgingham-amd-from-image")


def _run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


def test_usage_names_batch_and_jpeg():
    r = _run("--help")
    assert r.returncode == 0
    assert "--batch" in r.stdout and "--jpeg-entropy" in r.stdout and "JPEG" in r.stdout
    assert "(binary PGM or PNG)" not in r.stdout
    assert "no worker stops" in r.stdout                      # an unreadable image does not end the run in this mode


def test_batch_argument_errors_need_no_device(tmp_path):
    img = tmp_path / "a.pgm"
    files_cases.write_pgm(img, np.zeros((32, 32), np.uint8))
    for args, message in ((("--batch", "0"), "--batch takes a positive frame count"),
                          (("--batch", "x"), "--batch takes a positive frame count"),
                          (("--batch", "-3"), "--batch takes a positive frame count"),
                          (("--batch", "4x"), "--batch takes a positive frame count"),
                          (("--batch", "4", "--debug"), "--batch works on one GPU"),
                          (("--batch", "4", "--blobs"), "--batch works on one GPU"),
                          (("--batch", "4", "--gpus", "2"), "--batch works on one GPU"),
                          (("--jpeg-entropy", "device"), "--jpeg-entropy is only accepted with --batch"),
                          (("--batch", "4", "--jpeg-entropy", "gpu"), "--jpeg-entropy takes 'host' or 'device'")):
        r = _run(*args, str(img))
        assert r.returncode == 1 and message in r.stderr, (args, r.returncode, r.stderr)
        assert r.stdout == ""                                 # nothing of the table was written
