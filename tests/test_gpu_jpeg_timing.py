"""Kernel timing around the device entropy decoders (csrc/jpeg_huff.hip, csrc/jpeg_huff_sync.hip): how many pairs of events
one mrgingham_amd_jpeg_entropy_batch call leaves for mrgingham_amd_chess_kernel_ms -- one per decoder that has a file to
take, whichever phase option "jpeg_sync_time_phase" selects, none with timing off.  The 48 x 64 fixtures only."""
import pytest

import mrgingham_amd
from test_jpeg_io import case
from test_jpeg_scan import rst_case

pytestmark = pytest.mark.gpu

H, W = 64, 48


@pytest.fixture(scope="module")
def det():
    d = mrgingham_amd.Detector()
    yield d
    d.set_kernel_timing(0)
    d.chess_kernel_ms()
    d.close()


def _intervals():
    return [rst_case("noise_48x64_grey").data, rst_case("rows_48x64_420").data, rst_case("black_48x64").data]


def _plain():
    return [rst_case("nodri_48x64").data, rst_case("nodri_48x64").data]


def _pairs(det, datas, sync, want_status):
    """The pairs one call records: timing on, earlier pairs read out first."""
    det.set_kernel_timing(1)
    det.chess_kernel_ms()
    status = det.jpeg_entropy(datas, H, W, sync=sync)[2]
    assert status.tolist() == want_status
    return det.chess_kernel_ms()[1]


@pytest.mark.parametrize("memset", [0, 1])
def test_one_pair_for_a_batch_of_restart_interval_files(det, memset):
    det.set_option("jpeg_entropy_memset", memset)
    try:
        assert _pairs(det, _intervals(), False, [0, 0, 0]) == 1
    finally:
        det.set_option("jpeg_entropy_memset", 0)


@pytest.mark.parametrize("phase", [0, 1, 2, 3, 4])
def test_one_pair_for_a_batch_of_files_without_restart_intervals_at_every_phase(det, phase):
    det.set_option("jpeg_sync_time_phase", phase)
    try:
        assert _pairs(det, _plain(), True, [0, 0]) == 1
    finally:
        det.set_option("jpeg_sync_time_phase", 0)


def test_two_pairs_for_a_batch_of_both_kinds(det):
    assert _pairs(det, _intervals() + _plain(), True, [0, 0, 0, 0, 0]) == 2


def test_no_pair_where_no_decoder_has_a_file(det):
    assert _pairs(det, [case("progressive_48x64").data, case("noise_16x16_444").data], True, [-1, -2]) == 0


def test_no_pair_with_timing_off(det):
    assert _pairs(det, _intervals() + _plain(), True, [0, 0, 0, 0, 0]) == 2
    det.set_kernel_timing(0)
    assert det.jpeg_entropy(_intervals() + _plain(), H, W, sync=True)[2].tolist() == [0, 0, 0, 0, 0]
    assert det.chess_kernel_ms()[1] == 0
