"""ctypes binding of libmrgingham_amd.so (the C-ABI in include/mrgingham_amd.h).

The library is HIP-only.  If it is missing or cannot be loaded this module
raises -- there is no CPU implementation to fall back to.
"""
import ctypes
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MRGINGHAM_AMD_LIB") or os.path.join(_HERE, "libmrgingham_amd.so")  # override: A/B builds

ADD_POINTS_F64 = ctypes.CFUNCTYPE(ctypes.c_bool, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_void_p)
ADD_POINTS_INT = ctypes.CFUNCTYPE(ctypes.c_bool, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_double,
                                  ctypes.c_void_p)


PROGRESS_F = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_void_p)


class FilesOptions(ctypes.Structure):
    """mrgingham_amd_files_options"""
    _fields_ = [(n, ctypes.c_int) for n in ("do_clahe", "blur_radius", "gridn", "image_pyramid_level", "do_refine",
                                            "batch_frames", "nthreads", "jpeg_entropy", "device")]


class TiffInfo(ctypes.Structure):
    """mrgingham_amd_tiff_info"""
    _fields_ = [(n, ctypes.c_int32) for n in ("width", "height", "bits", "samples", "photometric", "compression", "predictor",
                                              "big_endian")]


class TiffStrip(ctypes.Structure):
    """mrgingham_amd_tiff_strip"""
    _fields_ = [("offset", ctypes.c_int64), ("nbytes", ctypes.c_int64), ("first_row", ctypes.c_int32), ("rows", ctypes.c_int32)]


class BmpInfo(ctypes.Structure):
    """mrgingham_amd_bmp_info"""
    _fields_ = [(n, ctypes.c_int32) for n in ("width", "height", "bits", "compression", "top_down", "row_bytes")] + [
        ("payload_offset", ctypes.c_int64), ("lut", ctypes.c_uint8 * 256), ("lut_identity", ctypes.c_int32)]


class PnmInfo(ctypes.Structure):
    """mrgingham_amd_pnm_info"""
    _fields_ = [(n, ctypes.c_int32) for n in ("width", "height", "bits", "channels", "black_and_white", "magic", "row_bytes")] + [
        ("payload_offset", ctypes.c_int64)]


class Frames(ctypes.Structure):
    """mrgingham_amd_frames"""
    _fields_ = [("frames", ctypes.c_void_p), ("frame_pitch", ctypes.c_int64), ("nframes", ctypes.c_int),
                ("width", ctypes.c_int), ("height", ctypes.c_int), ("stride", ctypes.c_int)]


# every symbol include/mrgingham_amd.h declares
EXPORTS = [
    "mrgingham_ChESS_response_5", "find_chessboard_corners_from_image_array_C",
    "refine_chessboard_corners_from_image_array_C", "find_chessboard_from_image_array_C",
    "mrgingham_amd_find_grid_from_points", "mrgingham_amd_find_grid_from_points_traced", "mrgingham_amd_find_grid_from_points_perturbed", "mrgingham_amd_find_boards_stats", "mrgingham_amd_grid_clock", "mrgingham_amd_packed_layout", "mrgingham_amd_gather_rccl", "mrgingham_amd_create", "mrgingham_amd_destroy",
    "mrgingham_amd_last_error", "mrgingham_amd_abi_version", "mrgingham_amd_device_count", "mrgingham_amd_level_dims",
    "mrgingham_amd_chess_response_batch", "mrgingham_amd_decimate_batch", "mrgingham_amd_box_blur_batch",
    "mrgingham_amd_preprocess_batch", "mrgingham_amd_preprocess16_batch", "mrgingham_amd_process_image", "mrgingham_amd_process_image_ex", "mrgingham_amd_preprocess_image16", "mrgingham_amd_preprocess_image",
    "find_chessboard_corners_from_image_file_C", "find_chessboard_from_image_file_C",
    "mrgingham_amd_detect_batch", "mrgingham_amd_refine_batch", "mrgingham_amd_chain_batch",
    "mrgingham_amd_find_boards_batch", "mrgingham_amd_cc_on_response_batch", "mrgingham_amd_scratch_bytes", "mrgingham_amd_chain_info", "mrgingham_amd_debug_refine_clock", "mrgingham_amd_debug_paths", "mrgingham_amd_read_image",
    "mrgingham_amd_set_option", "mrgingham_amd_sync", "mrgingham_amd_stream_wait", "mrgingham_amd_after_stream", "mrgingham_amd_set_kernel_timing",
    "mrgingham_amd_chess_kernel_ms", "mrgingham_amd_sclk_mhz", "mrgingham_amd_sparse_fallbacks", "mrgingham_amd_find_boards_submit",
    "mrgingham_amd_find_boards_collect", "mrgingham_amd_device_for_thread", "mrgingham_amd_set_thread_device",
    "mrgingham_amd_thread_device", "mrgingham_amd_host_alloc", "mrgingham_amd_host_free", "mrgingham_amd_host_register",
    "mrgingham_amd_host_unregister", "mrgingham_amd_shard_range", "mrgingham_amd_chain_multi", "mrgingham_amd_sync_multi",
    "mrgingham_amd_stream_wait_multi", "mrgingham_amd_kernel_id", "mrgingham_amd_set_wait_policy",
    "mrgingham_amd_blobs_batch", "mrgingham_amd_find_circle_grids_batch", "mrgingham_amd_blobs_stats",
    "mrgingham_amd_jpeg_coefficients", "mrgingham_amd_jpeg_idct_batch", "mrgingham_amd_read_jpegs_batch",
    "mrgingham_amd_jpeg_restart_intervals", "mrgingham_amd_jpeg_entropy_batch", "mrgingham_amd_jpeg_sync_rounds",
    "mrgingham_amd_find_boards_submit_ex", "mrgingham_amd_probe_image", "mrgingham_amd_files_plan",
    "mrgingham_amd_find_boards_files", "mrgingham_amd_debug_pixel_stage", "mrgingham_amd_debug_pixel_products",
    "mrgingham_amd_png_scanlines", "mrgingham_amd_png_reconstruct_batch", "mrgingham_amd_png_reconstruct_geometry",
    "mrgingham_amd_read_pngs_batch", "mrgingham_amd_find_boards_files_ex",
    "mrgingham_amd_pgm_header", "mrgingham_amd_pgm_unpack_batch", "mrgingham_amd_read_pgms_batch",
    "mrgingham_amd_tiff_layout", "mrgingham_amd_tiff_decode_batch", "mrgingham_amd_tiff_geometry",
    "mrgingham_amd_read_tiffs_batch", "mrgingham_amd_find_boards_files_ex2",
    "mrgingham_amd_tiff_layout_ex", "mrgingham_amd_tiff_inflate_lanes", "mrgingham_amd_find_boards_files_ex3",
    "mrgingham_amd_tiff_layout_tiled", "mrgingham_amd_tiff_decode_batch_tiled",
    "mrgingham_amd_bmp_layout", "mrgingham_amd_bmp_unpack_batch", "mrgingham_amd_bmp_unpack_geometry",
    "mrgingham_amd_read_bmps_batch", "mrgingham_amd_find_boards_files_ex4",
    "mrgingham_amd_pnm_header", "mrgingham_amd_pnm_unpack_batch", "mrgingham_amd_pnm_unpack_geometry",
    "mrgingham_amd_read_pnms_batch", "mrgingham_amd_find_boards_files_ex5",
    "mrgingham_amd_raw_row_bytes", "mrgingham_amd_raw_unpack_image", "mrgingham_amd_raw_unpack_batch",
    "mrgingham_amd_raw_unpack_geometry",
    "mrgingham_amd_bayer_grey_image", "mrgingham_amd_bayer_grey_batch", "mrgingham_amd_bayer_grey_geometry",
    "mrgingham_amd_colour_grey_image", "mrgingham_amd_colour_grey_batch", "mrgingham_amd_colour_grey_geometry",
    "mrgingham_amd_find_grids_batch", "mrgingham_amd_find_grids_host", "mrgingham_amd_find_grids_geometry",
    "mrgingham_amd_find_grids_stats",
]


def build(force=False):
    """hipcc --offload-arch=gfx950 build of the shared library, in-tree."""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-s", "-C", src, "clean"], stdout=sys.stderr)
    subprocess.check_call(["make", "-s", "-C", src, "-j4", "all"], stdout=sys.stderr)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch first: it brings its own libamdhip64, and device pointers / streams are
    # shared between torch and this library, so both must sit on ONE HIP runtime.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C mrgingham_amd/csrc` "
                           "(hipcc, gfx950).  mrgingham_amd has no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    c_int, c_vp, c_bool = ctypes.c_int, ctypes.c_void_p, ctypes.c_bool
    FP = ctypes.POINTER(Frames)
    L.mrgingham_ChESS_response_5.argtypes = [c_vp, c_vp, c_int, c_int, c_int]
    L.mrgingham_ChESS_response_5.restype = None
    L.find_chessboard_corners_from_image_array_C.argtypes = [c_int, c_int, c_int, c_vp, c_int, c_bool, c_bool,
                                                             ADD_POINTS_INT, c_vp]
    L.find_chessboard_corners_from_image_array_C.restype = c_bool
    L.refine_chessboard_corners_from_image_array_C.argtypes = [c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int,
                                                               c_bool]
    L.refine_chessboard_corners_from_image_array_C.restype = c_int
    L.find_chessboard_from_image_array_C.argtypes = [c_int, c_int, c_int, c_vp, c_int, c_int, c_bool, c_bool, c_int,
                                                     c_int, ADD_POINTS_F64, c_vp]
    L.find_chessboard_from_image_array_C.restype = c_bool
    L.mrgingham_amd_find_grid_from_points.argtypes = [c_vp, c_int, c_int, c_vp]
    L.mrgingham_amd_find_grid_from_points.restype = c_bool
    L.mrgingham_amd_find_grid_from_points_traced.argtypes = [c_vp, c_int, c_int, c_vp, c_int, c_int, c_int]
    L.mrgingham_amd_find_grid_from_points_traced.restype = c_bool
    L.mrgingham_amd_find_grid_from_points_perturbed.argtypes = [c_vp, c_int, c_int, c_vp, ctypes.c_uint, c_int]
    L.mrgingham_amd_find_grid_from_points_perturbed.restype = c_bool
    L.mrgingham_amd_find_boards_stats.argtypes = [c_vp, c_vp, c_int, c_int]
    L.mrgingham_amd_grid_clock.argtypes = [c_vp, c_int]
    L.mrgingham_amd_packed_layout.argtypes = [c_int, c_int, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    L.mrgingham_amd_gather_rccl.argtypes = [c_vp, c_vp, c_int, c_vp, ctypes.c_size_t, c_vp, c_vp]
    L.mrgingham_amd_create.argtypes = [c_int]
    L.mrgingham_amd_create.restype = c_vp
    L.mrgingham_amd_destroy.argtypes = [c_vp]
    L.mrgingham_amd_destroy.restype = None
    L.mrgingham_amd_last_error.argtypes = [c_vp]
    L.mrgingham_amd_last_error.restype = ctypes.c_char_p
    L.mrgingham_amd_abi_version.restype = c_int
    L.mrgingham_amd_kernel_id.restype = ctypes.c_char_p
    L.mrgingham_amd_device_count.restype = c_int
    L.mrgingham_amd_level_dims.argtypes = [c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    L.mrgingham_amd_chess_response_batch.argtypes = [c_vp, FP, c_int, c_int, c_vp, c_vp]
    L.mrgingham_amd_decimate_batch.argtypes = [c_vp, FP, c_int, c_vp, c_vp]
    L.mrgingham_amd_box_blur_batch.argtypes = [c_vp, FP, c_int, c_vp, c_vp]
    L.mrgingham_amd_preprocess_batch.argtypes = [c_vp, FP, c_int, c_int, c_vp, c_vp]
    L.mrgingham_amd_preprocess16_batch.argtypes = [c_vp, c_vp, ctypes.c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_vp,
                                                   c_vp]
    L.mrgingham_amd_detect_batch.argtypes = [c_vp, FP, c_int, c_vp, c_int, c_vp]
    L.mrgingham_amd_refine_batch.argtypes = [c_vp, FP, c_int, c_vp, c_vp, c_vp, c_int, c_vp]
    L.mrgingham_amd_chain_batch.argtypes = [c_vp, FP, c_int, c_vp, c_vp, c_vp, c_int]
    L.mrgingham_amd_find_boards_batch.argtypes = [c_vp, FP, c_int, c_int, c_vp, c_vp, c_int]
    L.mrgingham_amd_find_boards_submit.argtypes = [c_vp, FP, c_int, c_int, c_vp, c_vp, c_int]
    L.mrgingham_amd_find_boards_collect.argtypes = [c_vp, c_int]
    if hasattr(L, "mrgingham_amd_blobs_batch"):    # (an older A/B build behind MRGINGHAM_AMD_LIB has not got them:
        L.mrgingham_amd_blobs_batch.argtypes = [c_vp, FP, c_vp, c_int, c_vp, c_int]   # calling one fails in ctypes)
        L.mrgingham_amd_find_circle_grids_batch.argtypes = [c_vp, FP, c_int, c_vp, c_vp, c_int]
        L.mrgingham_amd_blobs_stats.argtypes = [c_vp, c_vp, c_int, c_int]
    if hasattr(L, "mrgingham_amd_jpeg_idct_batch"):
        L.mrgingham_amd_jpeg_coefficients.argtypes = [c_vp, ctypes.c_size_t, c_vp, ctypes.c_size_t, c_vp] + [ctypes.POINTER(c_int)] * 4
        L.mrgingham_amd_jpeg_idct_batch.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp,
                                                    ctypes.c_int64, c_int, c_vp]
        L.mrgingham_amd_read_jpegs_batch.argtypes = [c_vp, ctypes.POINTER(ctypes.c_char_p), c_int, c_int, c_int, c_vp,
                                                     ctypes.c_int64, c_int, c_int, c_vp]
    if hasattr(L, "mrgingham_amd_jpeg_entropy_batch"):
        L.mrgingham_amd_jpeg_restart_intervals.argtypes = [c_vp, ctypes.c_size_t, ctypes.POINTER(c_int), c_vp, ctypes.c_size_t,
                                                           ctypes.POINTER(ctypes.c_size_t)]
        L.mrgingham_amd_jpeg_entropy_batch.argtypes = [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, ctypes.c_int64, c_int, c_int,
                                                       c_vp, c_vp]
    if hasattr(L, "mrgingham_amd_jpeg_sync_rounds"):
        L.mrgingham_amd_jpeg_sync_rounds.argtypes = [c_vp, ctypes.c_size_t, c_int, ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_size_t)]
    if hasattr(L, "mrgingham_amd_find_boards_files"):
        L.mrgingham_amd_find_boards_submit_ex.argtypes = [c_vp, FP, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int]
        L.mrgingham_amd_probe_image.argtypes = [ctypes.c_char_p] + [ctypes.POINTER(c_int)] * 4
        L.mrgingham_amd_files_plan.argtypes = [c_vp, c_int, c_int, c_vp, c_vp, ctypes.POINTER(ctypes.c_int32)]
        L.mrgingham_amd_find_boards_files.argtypes = [ctypes.POINTER(ctypes.c_char_p), c_int, ctypes.POINTER(FilesOptions), c_vp, c_vp,
                                                      c_vp, c_vp, PROGRESS_F, c_vp, c_vp, c_int]
    if hasattr(L, "mrgingham_amd_png_reconstruct_batch"):
        L.mrgingham_amd_png_scanlines.argtypes = [c_vp, ctypes.c_size_t, c_vp, ctypes.c_size_t] + [ctypes.POINTER(c_int)] * 4
        L.mrgingham_amd_png_reconstruct_batch.argtypes = [c_vp, c_vp, ctypes.c_int64, c_int, c_int, c_int, c_int, c_int, c_vp,
                                                          ctypes.c_int64, c_int, c_vp]
        L.mrgingham_amd_png_reconstruct_geometry.argtypes = [ctypes.POINTER(c_int)] * 2
        L.mrgingham_amd_png_reconstruct_geometry.restype = None
        L.mrgingham_amd_read_pngs_batch.argtypes = [c_vp, ctypes.POINTER(ctypes.c_char_p), c_int, c_int, c_int, c_int, c_vp,
                                                    ctypes.c_int64, c_int, c_int, c_vp]
        L.mrgingham_amd_find_boards_files_ex.argtypes = [ctypes.POINTER(ctypes.c_char_p), c_int, ctypes.POINTER(FilesOptions), c_vp,
                                                         c_vp, c_vp, c_vp, PROGRESS_F, c_vp, c_vp, c_int, c_int]
    if hasattr(L, "mrgingham_amd_pgm_unpack_batch"):
        L.mrgingham_amd_pgm_header.argtypes = [c_vp, ctypes.c_size_t] + [ctypes.POINTER(c_int)] * 3 + [ctypes.POINTER(ctypes.c_size_t)]
        L.mrgingham_amd_pgm_unpack_batch.argtypes = [c_vp, c_vp, ctypes.c_int64, c_int, c_int, c_int, c_int, c_vp, ctypes.c_int64, c_int,
                                                     c_vp]
        L.mrgingham_amd_read_pgms_batch.argtypes = [c_vp, ctypes.POINTER(ctypes.c_char_p), c_int, c_int, c_int, c_int, c_vp,
                                                    ctypes.c_int64, c_int, c_int, c_vp]
    if hasattr(L, "mrgingham_amd_tiff_decode_batch"):
        L.mrgingham_amd_tiff_layout.argtypes = [c_vp, ctypes.c_size_t, ctypes.c_int64, ctypes.POINTER(TiffInfo), c_vp, ctypes.c_size_t,
                                                ctypes.POINTER(ctypes.c_size_t)]
        L.mrgingham_amd_tiff_decode_batch.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp, c_int, c_vp, c_int, ctypes.POINTER(TiffInfo), c_vp,
                                                      ctypes.c_int64, c_int, c_vp, c_vp, c_vp]
        L.mrgingham_amd_tiff_geometry.argtypes = [ctypes.POINTER(c_int)] * 3
        L.mrgingham_amd_tiff_geometry.restype = None
        L.mrgingham_amd_read_tiffs_batch.argtypes = [c_vp, ctypes.POINTER(ctypes.c_char_p), c_int, c_int, c_int, c_int, c_vp,
                                                     ctypes.c_int64, c_int, c_int, c_vp]
        L.mrgingham_amd_find_boards_files_ex2.argtypes = [ctypes.POINTER(ctypes.c_char_p), c_int, ctypes.POINTER(FilesOptions), c_vp,
                                                          c_vp, c_vp, c_vp, PROGRESS_F, c_vp, c_vp, c_int, c_int]
    if hasattr(L, "mrgingham_amd_tiff_layout_ex"):
        L.mrgingham_amd_tiff_layout_ex.argtypes = [c_vp, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(TiffInfo), c_vp,
                                                   ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        L.mrgingham_amd_tiff_inflate_lanes.argtypes = []
    if hasattr(L, "mrgingham_amd_tiff_layout_tiled"):
        L.mrgingham_amd_tiff_layout_tiled.argtypes = [c_vp, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(TiffInfo),
                                                      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), c_vp,
                                                      ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        L.mrgingham_amd_tiff_decode_batch_tiled.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp, c_int, c_vp, c_int, ctypes.POINTER(TiffInfo),
                                                            c_int, c_int, c_vp, ctypes.c_int64, c_int, c_vp, c_vp, c_vp]
        L.mrgingham_amd_find_boards_files_ex3.argtypes = [ctypes.POINTER(ctypes.c_char_p), c_int, ctypes.POINTER(FilesOptions), c_vp,
                                                          c_vp, c_vp, c_vp, PROGRESS_F, c_vp, c_vp, c_int, c_int]
    if hasattr(L, "mrgingham_amd_bmp_unpack_batch"):
        L.mrgingham_amd_bmp_layout.argtypes = [c_vp, ctypes.c_size_t, ctypes.POINTER(BmpInfo)]
        L.mrgingham_amd_bmp_unpack_batch.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp,
                                                     ctypes.c_int64, c_int, c_vp]
        L.mrgingham_amd_bmp_unpack_geometry.argtypes = [ctypes.POINTER(c_int)] * 2
        L.mrgingham_amd_bmp_unpack_geometry.restype = None
        L.mrgingham_amd_read_bmps_batch.argtypes = [c_vp, ctypes.POINTER(ctypes.c_char_p), c_int, c_int, c_int, c_vp, ctypes.c_int64,
                                                    c_int, c_int, c_vp]
        L.mrgingham_amd_find_boards_files_ex4.argtypes = [ctypes.POINTER(ctypes.c_char_p), c_int, ctypes.POINTER(FilesOptions), c_vp,
                                                          c_vp, c_vp, c_vp, PROGRESS_F, c_vp, c_vp, c_int, c_int]
    if hasattr(L, "mrgingham_amd_pnm_unpack_batch"):
        L.mrgingham_amd_pnm_header.argtypes = [c_vp, ctypes.c_size_t, ctypes.POINTER(PnmInfo)]
        L.mrgingham_amd_pnm_unpack_batch.argtypes = [c_vp, c_vp, ctypes.c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_vp,
                                                     ctypes.c_int64, c_int, c_vp]
        L.mrgingham_amd_pnm_unpack_geometry.argtypes = [ctypes.POINTER(c_int)] * 2
        L.mrgingham_amd_pnm_unpack_geometry.restype = None
        L.mrgingham_amd_read_pnms_batch.argtypes = [c_vp, ctypes.POINTER(ctypes.c_char_p), c_int, c_int, c_int, c_int, c_vp, ctypes.c_int64,
                                                    c_int, c_int, c_vp]
        L.mrgingham_amd_find_boards_files_ex5.argtypes = [ctypes.POINTER(ctypes.c_char_p), c_int, ctypes.POINTER(FilesOptions), c_vp,
                                                          c_vp, c_vp, c_vp, PROGRESS_F, c_vp, c_vp, c_int, c_int]
    if hasattr(L, "mrgingham_amd_raw_unpack_batch"):
        L.mrgingham_amd_raw_row_bytes.argtypes = [c_int, c_int]
        L.mrgingham_amd_raw_row_bytes.restype = ctypes.c_int64
        L.mrgingham_amd_raw_unpack_image.argtypes = [c_vp, ctypes.c_size_t, c_int, c_int, ctypes.c_int64, c_int, c_vp, c_int]
        L.mrgingham_amd_raw_unpack_batch.argtypes = [c_vp, c_vp, ctypes.c_int64, c_int, c_int, c_int, ctypes.c_int64, c_int, c_vp,
                                                     ctypes.c_int64, c_int, c_vp]
        L.mrgingham_amd_raw_unpack_geometry.argtypes = [ctypes.POINTER(c_int)] * 2
        L.mrgingham_amd_raw_unpack_geometry.restype = None
    if hasattr(L, "mrgingham_amd_bayer_grey_batch"):
        L.mrgingham_amd_bayer_grey_image.argtypes = [c_vp, c_int, c_int, c_int, ctypes.c_int64, c_int, c_vp, ctypes.c_int64]
        L.mrgingham_amd_bayer_grey_batch.argtypes = [c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.c_int64, ctypes.c_int64, c_int, c_vp,
                                                     ctypes.c_int64, ctypes.c_int64, c_vp]
        L.mrgingham_amd_bayer_grey_geometry.argtypes = [ctypes.POINTER(c_int)] * 3
        L.mrgingham_amd_bayer_grey_geometry.restype = None
    if hasattr(L, "mrgingham_amd_colour_grey_batch"):
        L.mrgingham_amd_colour_grey_image.argtypes = [c_vp, c_int, c_int, c_int, c_int, ctypes.c_int64, ctypes.c_int64, c_vp, ctypes.c_int64]
        L.mrgingham_amd_colour_grey_batch.argtypes = [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, ctypes.c_int64, ctypes.c_int64,
                                                      ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp]
        L.mrgingham_amd_colour_grey_geometry.argtypes = [ctypes.POINTER(c_int)] * 2
        L.mrgingham_amd_colour_grey_geometry.restype = None
    if hasattr(L, "mrgingham_amd_find_grids_batch"):
        L.mrgingham_amd_find_grids_batch.argtypes = [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp]
        L.mrgingham_amd_find_grids_host.argtypes = [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp]
        L.mrgingham_amd_find_grids_geometry.argtypes = [ctypes.POINTER(c_int)] * 5 + [ctypes.POINTER(ctypes.c_int64)]
        L.mrgingham_amd_find_grids_geometry.restype = None
        L.mrgingham_amd_find_grids_stats.argtypes = [c_vp, c_vp, c_int, c_int]
    L.mrgingham_amd_device_for_thread.argtypes = [c_int, c_int, ctypes.c_char_p]
    L.mrgingham_amd_set_thread_device.argtypes = [c_int]
    L.mrgingham_amd_host_alloc.argtypes = [ctypes.c_size_t]
    L.mrgingham_amd_host_alloc.restype = c_vp
    L.mrgingham_amd_host_free.argtypes = [c_vp]
    L.mrgingham_amd_host_free.restype = None
    L.mrgingham_amd_host_register.argtypes = [c_vp, ctypes.c_size_t]
    L.mrgingham_amd_host_unregister.argtypes = [c_vp]
    L.mrgingham_amd_set_wait_policy.argtypes = [c_int]
    L.mrgingham_amd_shard_range.argtypes = [c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    L.mrgingham_amd_chain_multi.argtypes = [ctypes.POINTER(c_vp), c_int, FP, c_int, c_vp, c_vp, c_vp, c_int]
    L.mrgingham_amd_sync_multi.argtypes = [ctypes.POINTER(c_vp), c_int]
    L.mrgingham_amd_stream_wait_multi.argtypes = [ctypes.POINTER(c_vp), c_int, c_vp]
    L.mrgingham_amd_cc_on_response_batch.argtypes = [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp,
                                                     c_vp, c_vp, c_vp, c_int, c_vp]
    L.mrgingham_amd_read_image.argtypes = [ctypes.c_char_p, c_int, c_vp, ctypes.c_size_t, ctypes.POINTER(c_int),
                                           ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    L.mrgingham_amd_debug_paths.argtypes = [c_vp, c_int, c_int, c_vp]
    L.mrgingham_amd_debug_pixel_stage.argtypes = [c_vp, c_int, FP, c_int, c_int, c_vp]
    L.mrgingham_amd_debug_pixel_products.argtypes = [c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
    L.mrgingham_amd_chain_info.argtypes = [c_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.mrgingham_amd_debug_refine_clock.argtypes = [c_vp, c_vp]
    L.mrgingham_amd_scratch_bytes.argtypes = [c_vp]
    L.mrgingham_amd_scratch_bytes.restype = ctypes.c_longlong
    L.mrgingham_amd_set_option.argtypes = [c_vp, ctypes.c_char_p, c_int]
    L.mrgingham_amd_sync.argtypes = [c_vp]
    L.mrgingham_amd_sparse_fallbacks.argtypes = [c_vp]
    L.mrgingham_amd_stream_wait.argtypes = [c_vp, c_vp]
    L.mrgingham_amd_after_stream.argtypes = [c_vp, c_vp]
    L.mrgingham_amd_set_kernel_timing.argtypes = [c_vp, c_int]
    L.mrgingham_amd_set_kernel_timing.restype = None
    L.mrgingham_amd_chess_kernel_ms.argtypes = [c_vp, ctypes.POINTER(c_int)]
    L.mrgingham_amd_chess_kernel_ms.restype = ctypes.c_double
    L.mrgingham_amd_sclk_mhz.argtypes = [c_vp]
    L.mrgingham_amd_sclk_mhz.restype = ctypes.c_double
    _lib = L
    return L
