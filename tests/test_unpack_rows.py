"""The row schedule that bmp_unpack_kernel, pnm_unpack_kernel and raw_unpack_kernel share (csrc/unpack_rows.h), no GPU:
its word arithmetic and the launch shape through a stand-alone program under the address and undefined-behaviour
sanitizers.  Integer arithmetic: every check is an equality."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrgingham_amd", "csrc")


def test_word_arithmetic_and_launch_shape_under_address_and_undefined_sanitizers(tmp_path):
    """tests/boundary/unpack_rows_main.cpp: for ES 1 and 2, every phase 0 .. 15 of a row against the 16-byte words (even
    ones at ES 2) and every width 1 .. 70, the words 0 .. K-1 are ascending, disjoint ranges of 1 .. 16/ES pixels that
    cover the row exactly, a whole word lies on a 16-byte boundary, and K is what the launch shape counts on; lpr_shift
    and blocks equal the formula written out in the program, for 1 and 256 CUs."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        flags = []  # (the sanitizer runtime of g++ is not installed: the program's own checks still run)
    exe = str(tmp_path / "unpack_rows")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-I", CSRC,
                        os.path.join(ROOT, "tests", "boundary", "unpack_rows_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.stdout, r.stderr[-4000:])
    words = r.stdout.split()
    assert words[0::2] == ["words8", "words16", "shapes", "checks"], r.stdout
    words8, words16, shapes, checks = (int(v) for v in words[1::2])
    # 16 (8) phases x 70 widths, each row at least one word; 2 CU counts x 5 row counts x 16 row lengths x aligned or not
    assert words8 >= 16 * 70 and words16 >= 8 * 70 and shapes == 2 * 5 * 16 * 2 and checks > 4 * (words8 + words16)
