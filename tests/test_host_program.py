"""The helper that builds the stand-alone sanitizer programs (tests/host_program.py) against the Makefile.  No GPU."""
import os
import re

from tests.host_program import CSRC, HOST_SOURCES


def test_host_sources_are_the_makefiles():
    text = open(os.path.join(CSRC, "Makefile")).read()
    lists = re.findall(r"^HOST_SRCS\s*:=\s*(.*)$", text, flags=re.M)
    assert len(lists) == 1 and tuple(lists[0].split()) == HOST_SOURCES
    for name in HOST_SOURCES:
        assert os.path.isfile(os.path.join(CSRC, name)), name

