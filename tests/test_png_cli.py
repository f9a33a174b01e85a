"""The tool's --png-reconstruct option, the part that needs no GPU: the usage text and the argument errors."""
import os
import subprocess

import numpy as np

from tests import files_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mrgingham_amd", "bin", "mrgingham-amd-from-image")


def _run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


def test_usage_names_png_reconstruct():
    r = _run("--help")
    assert r.returncode == 0 and "--png-reconstruct host|device" in r.stdout


def test_png_reconstruct_argument_errors_need_no_device(tmp_path):
    img = tmp_path / "a.pgm"
    files_cases.write_pgm(img, np.zeros((32, 32), np.uint8))
    for args, message in ((("--png-reconstruct", "device"), "--png-reconstruct is only accepted with --batch"),
                          (("--batch", "4", "--png-reconstruct", "gpu"), "--png-reconstruct takes 'host' or 'device'")):
        r = _run(*args, str(img))
        assert r.returncode == 1 and message in r.stderr, (args, r.returncode, r.stderr)
        assert r.stdout == ""
