"""mrgingham_amd: MI355X-native chessboard-corner candidate path of mrgingham.

Host-side mirror of the reference's Python module `mrgingham`
(mrgingham_pywrap.c:357-368) for the path this library covers, plus a batch
interface over torch tensors that already live in HBM.  Everything computes in
libmrgingham_amd.so (hand-written HIP, gfx950); PyTorch only supplies device
memory and streams.

    import mrgingham_amd as mrgingham
    r   = mrgingham.ChESS_response_5(image)            # int16[..., H, W]
    pts = mrgingham.find_points(image, image_pyramid_level=0)   # float64[N, 2]
    board = mrgingham.find_board(image, gridn=10)               # float64[100, 2] or None
"""
from .api import (ChESS_response_5, find_points, find_chessboard_corners, refine_points, find_board, find_chessboard,
                  find_grid_from_points, preprocess, read_image, jpeg_coefficients, jpeg_restart_intervals, jpeg_sync_rounds, Detector, level_dims,
                  find_boards_files, probe_image, KIND_PGM, KIND_PNG, KIND_JPEG, KIND_TIFF, KIND_BMP, KIND_PNM, files_plan, png_scanlines, png_reconstruct_geometry, PNG_NOT_TAKEN, pgm_header, PGM_HEADER_CUT,
                  tiff_layout, tiff_geometry, TIFF_NOT_TAKEN, TiffLayout, bmp_layout, bmp_unpack_geometry, BMP_NOT_TAKEN, BmpLayout,
                  pnm_header, pnm_unpack_geometry, PnmHeader, raw_row_bytes, raw_unpack, raw_unpack_geometry, RAW_FORMATS,
                  bayer_grey, bayer_grey_geometry, BAYER_PATTERNS, colour_grey, colour_grey_geometry, COLOUR_FORMATS,
                  find_grids_host, find_grids_geometry, boards_of_indices, GRID_DECLINES)

__all__ = ["ChESS_response_5", "find_points", "find_chessboard_corners", "refine_points", "find_board",
           "find_chessboard", "find_grid_from_points", "preprocess", "read_image", "jpeg_coefficients", "jpeg_restart_intervals", "jpeg_sync_rounds", "Detector",
           "level_dims", "find_boards_files", "probe_image", "KIND_PGM", "KIND_PNG", "KIND_JPEG", "KIND_TIFF", "KIND_BMP", "KIND_PNM", "files_plan", "png_scanlines", "png_reconstruct_geometry", "PNG_NOT_TAKEN", "pgm_header", "PGM_HEADER_CUT",
           "tiff_layout", "tiff_geometry", "TIFF_NOT_TAKEN", "TiffLayout", "bmp_layout", "bmp_unpack_geometry", "BMP_NOT_TAKEN", "BmpLayout",
           "pnm_header", "pnm_unpack_geometry", "PnmHeader", "raw_row_bytes", "raw_unpack", "raw_unpack_geometry", "RAW_FORMATS",
           "bayer_grey", "bayer_grey_geometry", "BAYER_PATTERNS", "colour_grey", "colour_grey_geometry", "COLOUR_FORMATS",
           "find_grids_host", "find_grids_geometry", "boards_of_indices", "GRID_DECLINES"]
