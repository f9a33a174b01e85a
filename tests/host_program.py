"""Stand-alone programs out of the library's host sources under the address and undefined-behaviour sanitizers: the one
place that knows which sources the host readers are made of and how g++ is called.  The programs have a main of their
own (tests/boundary/*_main.cpp) and run as child processes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrgingham_amd", "csrc")
# HOST_SRCS of mrgingham_amd/csrc/Makefile (tests/test_host_program.py holds the two together)
HOST_SOURCES = ("image_io.cpp", "jpeg.cpp")
FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_sanitized(tmp_path, main_cpp):
    """tests/boundary/<main_cpp> and the host readers of csrc/ built into a program in tmp_path -> its path.  Skips where
    g++ has no sanitizer runtime; a program that does not compile fails the test with the compiler's words."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the sanitizer runtime of g++ is not installed")
    exe = str(tmp_path / main_cpp.replace("_main.cpp", ""))
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *FLAGS, "-I", CSRC, os.path.join(ROOT, "tests", "boundary", main_cpp),
                        *(os.path.join(CSRC, s) for s in HOST_SOURCES), "-lz", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe
