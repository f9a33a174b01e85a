/*
 * mrgingham_amd.h -- C-ABI of the MI355X-native chessboard-corner candidate path.
 *
 * One shared library (mrgingham_amd/libmrgingham_amd.so, HIP for gfx950) exports
 *
 *   (1) the reference's own C symbols for this path, same names, arguments and
 *       error behaviour, so the reference's callers bind to it unchanged;
 *   (2) a batch API over frames that already live in HBM, which is what the
 *       single-frame symbols are thin wrappers of, and what bench.py measures.
 *
 * Plain pointers and sizes only: no torch, OpenCV or C++ types cross this
 * boundary.  INTEGRATION.md shows the reference-side bindings.  "file:line"
 * citations are into the upstream dkogan/mrgingham tree.
 *
 * There is no CPU fallback anywhere behind this header: with no usable HIP
 * device every entry point fails loudly (message on stderr, false / 0 / NULL /
 * negative status), it never computes on the host.
 */
#pragma once
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* History of the boundary (mrgingham_amd_abi_version() reports what the LIBRARY was built as; compare with this macro):
 *   1  rounds 1-3.
 *   2  round 4: MRGINGHAM_AMD_ERR_SPARSE (-4) left the status enum -- value -4 stays RESERVED, it is never returned and
 *      will not be reused --; option "sparse_refine" defaults to 1 (a context that runs sparse chains keeps a third scratch
 *      set, up to 16 GB: INTEGRATION.md 5e); find_boards_submit / _collect, chain_multi, host_alloc / _register,
 *      set_wait_policy, set_thread_device and the file entry points were added.
 *   3  round 5: mrgingham_amd_find_boards_stats, _grid_clock, _packed_layout, _gather_rccl added; the packed corner block
 *      is a multiple of 8 bytes; the reference-symbol wrappers restore the caller's current HIP device.
 *   4  round 6: mrgingham_amd_sclk_mhz added; options "chess_seg" / "chess16_seg" are per context (they were process-wide) and
 *      mean balanced segments, option "preprocess_fused"; _gather_rccl, _chain_multi, _sync_multi, _stream_wait_multi restore
 *      the caller's current HIP device; _gather_rccl needs no RCCL header or library at build time and never loads a second RCCL.
 *      Later, additive: mrgingham_amd_preprocess16_batch (16-bit frames on the device; option "preprocess_fused" covers it).
 *      Later, additive: mrgingham_amd_blobs_batch, _find_circle_grids_batch, _blobs_stats (the blob path over a batch on the
 *      device); option "blob_chunk_frames".
 *      Later, additive: mrgingham_amd_jpeg_coefficients, _jpeg_idct_batch, _read_jpegs_batch (baseline JPEG: entropy decode on
 *      the host, inverse DCT on the device); option "jpeg_chunk_frames"; mrgingham_amd_read_image and the file entry points
 *      read baseline JPEG.
 *      Later, additive: mrgingham_amd_jpeg_entropy_batch, _jpeg_restart_intervals (restart intervals Huffman-decoded on the
 *      device); options "jpeg_entropy", "jpeg_entropy_max_interval", "jpeg_entropy_memset".
 *      Later, additive and backward compatible: mrgingham_amd_jpeg_sync_rounds; options "jpeg_sync", "jpeg_sync_subsequence",
 *      "jpeg_sync_max_rounds" (files without restart markers Huffman-decoded on the device; off by default, and then every
 *      call behaves as before).
 *      Later, additive: mrgingham_amd_find_boards_submit_ex (no refinement, the corners' refinement levels),
 *      mrgingham_amd_probe_image, _files_plan, _find_boards_files (a list of image files to boards, loader and detector
 *      pipelined on two contexts).
 *      Later, additive: mrgingham_amd_debug_pixel_stage, _debug_pixel_products (test hooks: the pixel stage of a call alone
 *      and what it hands to the component search).
 *      Later, additive: mrgingham_amd_png_scanlines, _png_reconstruct_batch, _png_reconstruct_geometry, _read_pngs_batch (PNG:
 *      inflate on the host, row filters and grey on the device); option "png_chunk_frames"; mrgingham_amd_find_boards_files_ex
 *      (loader flags: MRGINGHAM_AMD_FILES_PNG_DEVICE).  Off unless asked for: every earlier call behaves as before.
 *      Later, additive (the version stays 4: new symbols and a new flag value break no caller): mrgingham_amd_pgm_header,
 *      _pgm_unpack_batch, _read_pgms_batch (binary PGM payloads to frames on the device); option "pgm_chunk_frames"; loader
 *      flag MRGINGHAM_AMD_FILES_DEEP_CHUNKS (16-bit PGM / PNG files in chunks).  Off unless asked for.
 *      Later, additive (the version stays 4): mrgingham_amd_read_image and _probe_image (MRGINGHAM_AMD_KIND_TIFF) read strip TIFF;
 *      mrgingham_amd_tiff_layout, _tiff_decode_batch, _tiff_geometry, _read_tiffs_batch (TIFF: LZW strips, predictor and
 *      grey on the device); options "tiff_chunk_frames", "tiff_lzw_max_strip", "tiff_lzw_lanes";
 *      mrgingham_amd_find_boards_files_ex2 (loader flag MRGINGHAM_AMD_FILES_TIFF_DEVICE).  The device route is off unless
 *      asked for.
 *      Later, additive (the version stays 4): mrgingham_amd_tiff_layout_ex and _tiff_inflate_lanes;
 *      mrgingham_amd_tiff_decode_batch takes compression 8 and 32946 (Deflate strips on the device); options "tiff_deflate",
 *      "tiff_deflate_max_strip", "tiff_deflate_lanes"; mrgingham_amd_find_boards_files_ex3 (loader flag
 *      MRGINGHAM_AMD_FILES_TIFF_DEFLATE_DEVICE).  Off unless asked for: mrgingham_amd_tiff_layout goes on leaving Deflate
 *      files to the host decoder.
 *      Later, additive (the version stays 4): mrgingham_amd_tiff_layout_tiled and _tiff_decode_batch_tiled (tiled TIFF:
 *      LZW and Deflate tiles one lane each, tile rows gathered into image rows on the device); mrgingham_amd_read_image,
 *      _probe_image, _read_tiffs_batch and the file-list entry points read tiled files, which were unreadable before.
 *      mrgingham_amd_tiff_layout and _tiff_layout_ex go on calling any tile tag unreadable, and no option changes.
 *      Later, additive (the version stays 4): mrgingham_amd_read_image and _probe_image (MRGINGHAM_AMD_KIND_BMP) read Windows Bitmap files,
 *      which were unreadable before; mrgingham_amd_bmp_layout, _bmp_unpack_batch, _bmp_unpack_geometry, _read_bmps_batch (BMP:
 *      row order, row padding, sub-byte indices, the palette and grey on the device); options "bmp_chunk_frames",
 *      "bmp_unpack"; mrgingham_amd_find_boards_files_ex4 (loader flag MRGINGHAM_AMD_FILES_BMP_DEVICE, which _ex3 goes on
 *      refusing).  The device route of the file list is off unless asked for.
 *      Later, additive (the version stays 4): mrgingham_amd_read_image and _probe_image (MRGINGHAM_AMD_KIND_PNM) read binary PBM (P4)
 *      and PAM (P7) files, which were unreadable before; mrgingham_amd_pnm_header, _pnm_unpack_batch,
 *      _pnm_unpack_geometry, _read_pnms_batch (colour to grey, big-endian pairs and packed bits on the device); options
 *      "pnm_chunk_frames", "pnm_unpack"; mrgingham_amd_find_boards_files_ex5 (loader flag MRGINGHAM_AMD_FILES_PNM_DEVICE,
 *      which _ex4 goes on refusing).  mrgingham_amd_pgm_header goes on refusing every magic but P5; ASCII Netpbm (P1, P2, P3)
 *      stays unreadable, and so does P6.  The device route of the file list is off unless asked for.
 *      Later, additive (the version stays 4): mrgingham_amd_raw_row_bytes, _raw_unpack_image, _raw_unpack_batch,
 *      _raw_unpack_geometry and the MRGINGHAM_AMD_RAW_* formats (packed 10 / 12 / 14-bit camera frames -- Mono10p, Mono12p,
 *      Mono14p, Mono10Packed, Mono12Packed -- to uint16 frames, on the host and on the device).  No earlier call, option
 *      or default changes; no file reader takes such frames (a headerless frame carries no size).
 *      Later, additive (the version stays 4): mrgingham_amd_bayer_grey_image, _bayer_grey_batch, _bayer_grey_geometry and the
 *      MRGINGHAM_AMD_BAYER_* patterns (Bayer mosaics, uint8 or uint16, to grey frames of the same type, on the host and on
 *      the device).  No earlier call, option or default changes; no file reader and no tool option takes a mosaic.
 *      Later, additive (the version stays 4): mrgingham_amd_colour_grey_image, _colour_grey_batch, _colour_grey_geometry and
 *      the MRGINGHAM_AMD_COLOUR_* formats (colour frames -- interleaved RGB / BGR with 3 or 4 samples, planar, packed YUV
 *      4:2:2 -- to grey frames of the same sample type, on the host and on the device).  No earlier call, option or default
 *      changes; no file reader and no tool option takes such frames.
 *      Later, additive (the version stays 4): mrgingham_amd_find_grids_batch, _find_grids_host, _find_grids_geometry,
 *      _find_grids_stats, the MRGINGHAM_AMD_GRID_DECLINE_* statuses and the options "find_boards_grid" and
 *      "find_grids_guard_bits" (the grid finder on the device: candidate lists to board indices).  No earlier call or
 *      default changes: find_boards keeps the host finder unless the option asks for the device's. */
#define MRGINGHAM_AMD_ABI_VERSION 4

/* ------------------------------------------------------------------------ */
/* (1) Reference symbols                                                    */
/* ------------------------------------------------------------------------ */

/* Replaces mrgingham_ChESS_response_5 (ChESS.h:31-34, ChESS.c:55-106).
 * HOST pointers, caller-owned.  `image` is w x h bytes with `stride` bytes per
 * row, `response` is a dense w x h int16 image.  Exactly like the reference,
 * only the interior [7,w-7) x [7,h-7) is written; the 7-pixel frame of
 * `response` is left untouched.  No return value; a device failure prints a
 * message on stderr and leaves `response` unwritten. */
void mrgingham_ChESS_response_5(int16_t* response, const uint8_t* image, int w, int h, int stride);

/* Replaces find_chessboard_corners_from_image_array_C
 * (mrgingham_pywrap_cplusplus_bridge.h:10-23, .cc:28-70), the extern "C" face
 * of mrgingham::find_chessboard_corners_from_image_array
 * (find_chessboard_corners.hh:12-30, .cc:568-587).
 * HOST image buffer (Nrows x Ncols bytes, `stride` bytes per row).  On success
 * calls add_points(xy, N, 1/1000., cookie) once with N > 0 interleaved
 * (x,y)*1000 ints in the reference's order (valid only during the callback)
 * and returns its result.  Returns false without calling add_points when
 * nothing was found or on an error (message on stderr):
 *   - image_pyramid_level outside [0,10]            (find_chessboard_corners.cc:433-441)
 *   - level 0 and stride != Ncols (non-continuous)  (find_chessboard_corners.cc:461-466)
 * doblobs (bridge.cc:50-55): the blob detector, find_blobs_from_image_array (find_blobs.cc:14-46: a
 * cv::SimpleBlobDetector with minArea 20, maxArea 80000, minDistBetweenBlobs 5, dark blobs), at level 0
 * only (any other level: false); like the reference it always "finds", i.e. add_points is called even with
 * N = 0.  debug: the reference's /tmp/mrgingham-* dumps of the pass
 * (find_chessboard_corners.cc:282-315, :453-459, :513-541). */
bool find_chessboard_corners_from_image_array_C(int Nrows, int Ncols, int stride, char* imagebuffer,
                                                int image_pyramid_level, bool doblobs, bool debug,
                                                bool (*add_points)(int* xy, int N, double scale, void* cookie),
                                                void* cookie);

/* C face of mrgingham::refine_chessboard_corners_from_image_array
 * (find_chessboard_corners.hh:51-72, .cc:591-619), which the reference only
 * exposes with std::vector / cv::Mat arguments.  points_xy: Npoints interleaved
 * doubles (full-resolution pixel coordinates), updated in place; level[i] is
 * the pyramid level point i was computed at and is lowered to
 * image_pyramid_level for each point that gets refined.  Returns the number of
 * refined points (0 on error, like the reference). */
int refine_chessboard_corners_from_image_array_C(int Nrows, int Ncols, int stride, char* imagebuffer,
                                                 double* points_xy, signed char* level, int Npoints,
                                                 int image_pyramid_level, bool debug);

/* Replaces find_chessboard_from_image_array_C (mrgingham_pywrap_cplusplus_bridge.h:25-42,
 * .cc:72-138) = mrgingham::find_chessboard_from_image_array with refinement on
 * (mrgingham.hh:28-56, mrgingham.cc:38-140): image_pyramid_level >= 0 uses that level,
 * < 0 tries levels 3, 2, 1, 0 until the grid finder succeeds; the gridn x gridn corners are then
 * refined towards level 0 and handed to add_points(xy, gridn*gridn, cookie) in board order.
 * The detector and the refinement run on the GPU, the grid finder (find_grid.cc) on the host.
 * Returns false when no board is found or on an error; doblobs (level 0 only, bridge.cc:104-113) is
 * find_circle_grid_from_image_array: blob detector + grid finder, no refinement;
 * debug writes the detector's / refinement's dumps (see above); debug_sequence_x, _y both >= 0 (bridge.cc:97-104)
 * make the grid finder trace, on stderr, the sequences it tries from the candidate nearest to that pixel
 * (find_grid.cc:247-306, :515-553: "Looking at sequences from", "Considering connection ...", "rejecting" /
 * "accepting"). */
bool find_chessboard_from_image_array_C(int Nrows, int Ncols, int stride, char* imagebuffer, const int gridn,
                                        int image_pyramid_level, bool doblobs, bool debug, int debug_sequence_x,
                                        int debug_sequence_y,
                                        bool (*add_points)(double* xy, int N, void* cookie), void* cookie);

/* C face of mrgingham::find_grid_from_points (mrgingham.hh:83-87, find_grid.cc:1216-1445), host
 * only: npoints interleaved (x,y)*1000 candidates in, gridn*gridn interleaved (x,y) corners out
 * (rows top to bottom, each left to right).  false when no grid is found. */
bool mrgingham_amd_find_grid_from_points(const int* xy_scaled, int npoints, int gridn, double* xy_out);

/* The same with the reference's debug arguments (mrgingham::find_grid_from_points(..., debug, debug_sequence),
 * mrgingham.hh:83-87).  debug != 0: the finder writes its self-plotting vnlog dumps /tmp/mrgingham-2-voronoi.vnl,
 * -3-candidates(.vnl, -detailed.vnl), -4-outer-edges(.vnl, -detailed.vnl), -5-outer-edge-cycles,
 * -6-identified-outer-edge-cycle and says on stderr what it found or why it gave up (find_grid.cc:385-779, :1229-1442).
 * debug_sequence_x, _y >= 0 name a pixel; the sequences tried from the candidate nearest to it are reported on
 * stderr (find_grid.cc:247-306, :515-553). */
bool mrgingham_amd_find_grid_from_points_traced(const int* xy_scaled, int npoints, int gridn, double* xy_out,
                                                int debug, int debug_sequence_x, int debug_sequence_y);

/* TEST HOOK: the same with the parts of the visiting order that cannot be checked against the
 * reference's boost::polygon graph perturbed -- ring_seed != 0 starts every site's neighbour ring at a
 * pseudo-random position, bit 0 of last_match takes the last neighbour that continues a sequence instead of
 * the first (find_grid.cc:216-222).  tests/test_grid.py asserts the results do not change.  Bit 1 of last_match
 * is the canonical start: every site's ring begins at its first neighbour counter-clockwise from +x (and ring_seed
 * rotates it from there), the rule of the stand-in Voronoi diagram under which tests/test_oracle_grid.py holds this
 * finder to the reference's own find_grid.cc bit for bit. */
bool mrgingham_amd_find_grid_from_points_perturbed(const int* xy_scaled, int npoints, int gridn, double* xy_out,
                                                   unsigned ring_seed, int last_match);

/* ------------------------------------------------------------------------ */
/* (2) Batch API over device-resident frames                                */
/* ------------------------------------------------------------------------ */

typedef struct mrgingham_amd_ctx mrgingham_amd_ctx;

/* A batch of equally-sized 8-bit frames in DEVICE memory:
 * frame f, row y starts at frames + f*frame_pitch + y*stride. */
typedef struct {
    const uint8_t* frames;
    int64_t frame_pitch; /* bytes between consecutive frames */
    int nframes;
    int width, height;
    int stride; /* bytes between consecutive rows */
} mrgingham_amd_frames;

enum {
    MRGINGHAM_AMD_OK = 0,
    MRGINGHAM_AMD_ERR_ARG = -1,      /* bad argument (level, sizes, NULL) */
    MRGINGHAM_AMD_ERR_DEVICE = -2,   /* HIP error; see mrgingham_amd_last_error */
    MRGINGHAM_AMD_ERR_CAPACITY = -3, /* an output capacity given by the caller was too small */
    /* -4 is reserved (MRGINGHAM_AMD_ERR_SPARSE of ABI 1: never returned since ABI 2) */
};

/* One context = one device, two HIP streams (the HBM-bound pixel kernels of a
 * batch run back to back on one, the latency-bound component kernels underneath
 * them on the other) and the per-level scratch buffers (level images, responses,
 * component tables), grown on demand and reused.  Not thread-safe: use one
 * context per host thread. */
mrgingham_amd_ctx* mrgingham_amd_create(int device_ordinal);
void mrgingham_amd_destroy(mrgingham_amd_ctx* ctx);
const char* mrgingham_amd_last_error(const mrgingham_amd_ctx* ctx);
int mrgingham_amd_abi_version(void);
/* Identity of the ChESS kernel sources the library was built from (16 hex digits of a SHA-256 over chess.hip and the
 * headers it includes): bench.py replays counter evidence collected in an earlier run (profiles/chess_l0_*.json) only
 * when that run used a library with the same id. */
const char* mrgingham_amd_kernel_id(void);
/* Number of usable HIP devices (0 = none: every entry point will fail, there is no CPU path). */
int mrgingham_amd_device_count(void);

/* How many frames the sparse refinement (option "sparse_refine") handed back to the dense kernels since the last call
 * of this function (they are repeated inside the call that met them; the outputs do not depend on it).  Synchronises. */
int mrgingham_amd_sparse_fallbacks(mrgingham_amd_ctx* ctx);

/* ---- several GPUs ---------------------------------------------------------------------------------------------
 * The reference-symbol wrappers of section (1) (and mrgingham_amd_process_image*, the file entry points) work on the
 * CALLING THREAD's context.  Which device that context lives on: MRGINGHAM_AMD_DEVICE if the variable is set (every
 * thread on that device); otherwise the k-th thread that calls into the library gets device k modulo the number of
 * devices -- the reference parallelises over worker threads with image i on worker i % N (mrgingham-from-image.cc:50,
 * :374-379), and mapped this way its workers spread over the GPUs of a node by themselves; a thread can also choose:
 * mrgingham_amd_set_thread_device (before its first call, or later: its context is then rebuilt on the new device). */
int mrgingham_amd_device_for_thread(int thread_index, int ndevices, const char* env_value);  /* the policy, as a function */
int mrgingham_amd_set_thread_device(int device_ordinal);
int mrgingham_amd_thread_device(void);  /* the device of the calling thread's context (created if need be); -1: none */

/* Host memory the device can read directly (page-locked, usable with every device): a frame handed to the wrappers
 * out of such memory is uploaded at the speed of the link, with no staging copy and no pinning on the fly (12 MB:
 * ~0.25 ms instead of ~0.45).  _register does the same for memory the caller already owns (it must stay allocated
 * until _unregister). */
void* mrgingham_amd_host_alloc(size_t bytes);
void mrgingham_amd_host_free(void* p);
int mrgingham_amd_host_register(void* p, size_t bytes);
int mrgingham_amd_host_unregister(void* p);

/* How the calling threads of this PROCESS wait for the device (hipSetDeviceFlags on every device): 0 = the runtime's
 * choice, 1 = spin, 2 = yield the core while waiting, 3 = block.  The runtime's default spins, which is the lowest
 * latency while every waiting thread has a core of its own -- and a cliff when it has not: a spinning thread burns the
 * time slice the thread that feeds the device is waiting for (32 callers on 16 cores, 4096 small images: 10-13 s
 * spinning, 4-6 s blocking, 1.4 s with four callers).  Better than any policy is FEWER callers per GPU -- the
 * command-line tool hands the images of all its workers to eight device threads per GPU --; a host that cannot
 * arrange that asks for 3.  Call it before the process creates its first context.  Returns 0, MRGINGHAM_AMD_ERR_ARG,
 * or MRGINGHAM_AMD_ERR_DEVICE when a device refused (the HIP runtime of the process is already running with another
 * policy: e.g. inside a PyTorch process). */
int mrgingham_amd_set_wait_policy(int policy);

/* Contiguous shards of `total` frames over n contexts / ranks: shard k = frames [*first, *first + *count), the first
 * total % n shards one frame longer (the split bench.py and mrgingham_amd/parallel.py use). */
int mrgingham_amd_shard_range(int total, int k, int n, int* first, int* count);

/* mrgingham_amd_chain_batch over several contexts -- one per device of a node -- in ONE call: context k takes
 * shards[k], a batch in the memory of ITS device (shards[k].nframes may be 0), and the corner lists of every shard
 * arrive in d_points / d_levels / d_npoints: buffers on the device of ctxs[0], laid out like mrgingham_amd_chain_batch's
 * for the sum of the shards' frames, shard after shard (frame-major).  A shard on the first context's device writes its
 * block in place; any other writes into buffers of its own context and the block travels device to device behind its
 * chain (a peer copy: xGMI between the GPUs of a node) -- the one exchange of the path.  Asynchronous like chain_batch;
 * consecutive calls need their own output buffers.  mrgingham_amd_sync_multi waits for every context and every gather
 * and returns the first error (MRGINGHAM_AMD_ERR_CAPACITY: as mrgingham_amd_sync -- make the call again);
 * mrgingham_amd_stream_wait_multi makes `stream` wait for them on the device instead.  Call these from one thread. */
int mrgingham_amd_chain_multi(mrgingham_amd_ctx* const* ctxs, int nctx, const mrgingham_amd_frames* shards, int start_level,
                              double* d_points, signed char* d_levels, int32_t* d_npoints, int points_pitch);
int mrgingham_amd_sync_multi(mrgingham_amd_ctx* const* ctxs, int nctx);
int mrgingham_amd_stream_wait_multi(mrgingham_amd_ctx* const* ctxs, int nctx, void* stream);

/* ---- one process per GPU: the exchange over RCCL ---------------------------------------------------------------
 * A host that runs one process (rank) per GPU calls mrgingham_amd_chain_batch on its shard with the three outputs laid
 * out in ONE device block -- mrgingham_amd_packed_layout: points at offset 0, levels at *off_levels, counts at
 * *off_npoints, *bytes in all (the layout of mrgingham_amd/parallel.py) -- and then mrgingham_amd_gather_rccl: ONE
 * ncclGather (rccl.h:745) of that block to rank `root` on `stream` (a hipStream_t of the context's device), queued behind
 * the chain on the device, asynchronous.  d_gathered (root only, may be NULL elsewhere): world x bytes, rank after rank,
 * i.e. frame-major over the global batch when ranks own contiguous shards (mrgingham_amd_shard_range).  nccl_comm is the
 * caller's ncclComm_t (this header names no RCCL type); the library does not link RCCL, it calls the ncclGather of the RCCL
 * the process already runs on.  Returns 0, MRGINGHAM_AMD_ERR_ARG, or MRGINGHAM_AMD_ERR_DEVICE (no RCCL in the process / the
 * collective failed: mrgingham_amd_last_error has RCCL's text). */
int mrgingham_amd_packed_layout(int nframes, int points_pitch, size_t* off_levels, size_t* off_npoints, size_t* bytes);
int mrgingham_amd_gather_rccl(mrgingham_amd_ctx* ctx, void* nccl_comm, int root, const void* d_packed, size_t bytes,
                              void* d_gathered, void* stream);

/* Size of pyramid level `level` of a width x height frame: what
 * cv::resize(.., 1/2^level, 1/2^level) produces (find_chessboard_corners.cc:449-450). */
int mrgingham_amd_level_dims(int width, int height, int level, int* w, int* h);

/* Dense ChESS response of every frame at pyramid level `level` (0 = the frame
 * itself): d_response receives nframes dense w_L x h_L int16 images back to
 * back.  clamp = 0: the raw reference response in the interior (ChESS.c:104),
 * zeros in the 7-pixel frame.  clamp = 1: negatives replaced by 0, i.e. the
 * buffer the reference's component search starts from
 * (find_chessboard_corners.cc:506-529).  `stream` is a hipStream_t, used as given
 * (NULL = HIP's default stream); the call is asynchronous on it. */
int mrgingham_amd_chess_response_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* frames, int level,
                                       int clamp, int16_t* d_response, void* stream);

/* Pyramid level images alone (find_chessboard_corners.cc:445-452): d_out
 * receives nframes dense w_L x h_L byte images. */
int mrgingham_amd_decimate_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* frames, int level,
                                 uint8_t* d_out, void* stream);

/* 3x3.. box blur the reference CLI applies before detection
 * (mrgingham-from-image.cc:106-111): d_out receives nframes dense byte images. */
int mrgingham_amd_box_blur_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* frames, int radius,
                                 uint8_t* d_out, void* stream);

/* The contrast preprocessing the reference CLI applies to an 8-bit frame before
 * detection (mrgingham-from-image.cc:38-45, :71-79, :106-111): when do_clahe,
 * cv::normalize(0, 255, NORM_MINMAX) then CLAHE (clip limit 8, 8x8 tiles); then a
 * (2*blur_radius+1)^2 box blur (0 = none).  d_out receives nframes dense byte
 * images and must not alias the input.  OpenCV arithmetic: parity unpinned. */
int mrgingham_amd_preprocess_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* frames, int do_clahe,
                                   int blur_radius, uint8_t* d_out, void* stream);

/* The same for 16-bit frames (mrgingham-from-image.cc:85-92, :106-111): when do_clahe, cv::normalize(0, 65535,
 * NORM_MINMAX) then CLAHE (clip limit 8, 8x8 tiles, 65 536 bins); convertTo(CV_8U, 255/65535); the box blur.
 * frames: device uint16, frame f row y at d_frames + f*frame_pitch + y*stride (pitch and stride in ELEMENTS);
 * d_out: nframes dense width x height bytes, must not alias the input.  Asynchronous on `stream` (NULL = default).
 * Arguments are checked like mrgingham_amd_preprocess_batch's (MRGINGHAM_AMD_ERR_ARG, nothing written).  The tile
 * tables take up to 24 MiB per frame (full-range data); a batch is worked through in chunks of frames whose tables stay
 * within 1 GiB of context scratch.  Same bytes as mrgingham_amd_preprocess_image16 per frame. */
int mrgingham_amd_preprocess16_batch(mrgingham_amd_ctx* ctx, const uint16_t* d_frames, int64_t frame_pitch, int nframes,
                                     int width, int height, int stride, int do_clahe, int blur_radius,
                                     uint8_t* d_out, void* stream);

/* find_chessboard_corners_from_image_array for every frame of the batch at one
 * pyramid level.  Device outputs: d_xy holds nframes blocks of
 * capacity_per_frame interleaved (x,y)*1000 int pairs in the reference's
 * order, d_counts[f] the number of candidates of frame f (may exceed
 * capacity_per_frame: then only the first capacity_per_frame were stored).
 * Asynchronous on the context's streams; mrgingham_amd_sync() waits. */
int mrgingham_amd_detect_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* frames, int level,
                               int32_t* d_xy, int capacity_per_frame, int32_t* d_counts);

/* refine_chessboard_corners_from_image_array for every frame at one level.
 * d_points: nframes blocks of points_pitch interleaved (x,y) doubles;
 * d_levels: nframes blocks of points_pitch signed chars; d_npoints[f] points
 * are live in frame f.  Updated in place; d_nrefined[f] (may be NULL) receives
 * the reference's return value. */
int mrgingham_amd_refine_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* frames, int level,
                               double* d_points, signed char* d_levels, const int32_t* d_npoints,
                               int points_pitch, int32_t* d_nrefined);

/* The reference's found-frame schedule for image_pyramid_level < 0 with the
 * grid finder left on the host (mrgingham.cc:50, :81-99): detect at
 * start_level, take every candidate as a corner ((double)x/1000,
 * find_grid.cc:353-354), then refine through start_level-1 .. 0.  Outputs as
 * mrgingham_amd_refine_batch; d_npoints[f] receives the candidate count. */
int mrgingham_amd_chain_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* frames, int start_level,
                              double* d_points, signed char* d_levels, int32_t* d_npoints, int points_pitch);

/* The connected-component stage ALONE, on caller-supplied responses: what
 * process_connected_components (find_chessboard_corners.cc:284-397) does with the buffer the
 * reference hands it, for the rule tests (running-maximum order dependence, thresholds 15 / 120,
 * N >= 2, margin columns, variance window, response mutation between refined points) that a natural
 * image only meets by chance.  d_response: nframes dense w x h int16 images (device), used the way
 * the reference's buffer arrives there: negatives count as 0 (:527-529) and everything outside
 * [7,w-7) x [7,h-7) as 0 (:506; the ChESS pass never writes there) -- the input is not modified.
 * d_level_image: nframes dense w x h byte images, the image the variance test reads (:50-88).
 * `level` only scales the output coordinates (:319, :346, :369, :390).  Exactly one mode:
 *   detect  d_xy / capacity_per_frame / d_counts as mrgingham_amd_detect_batch, d_points NULL;
 *   refine  d_points / d_levels / d_npoints / points_pitch / d_nrefined as
 *           mrgingham_amd_refine_batch, d_xy NULL.
 * Asynchronous like the other batch calls. */
int mrgingham_amd_cc_on_response_batch(mrgingham_amd_ctx* ctx, const int16_t* d_response,
                                       const uint8_t* d_level_image, int nframes, int w, int h, int level,
                                       int32_t* d_xy, int capacity_per_frame, int32_t* d_counts,
                                       double* d_points, signed char* d_levels, const int32_t* d_npoints,
                                       int points_pitch, int32_t* d_nrefined);

/* C faces of find_chessboard_corners_from_image_file (find_chessboard_corners.hh:32-44, .cc:623-648)
 * and find_chessboard_from_image_file (mrgingham.hh:77-83, mrgingham.cc:145-170): the image file is
 * decoded (binary PGM, non-interlaced PNG or baseline JPEG; the reference uses cv::imread) and handed to the array
 * functions above.  false when the file cannot be read or nothing is found. */
bool find_chessboard_corners_from_image_file_C(const char* filename, int image_pyramid_level, bool debug,
                                               bool (*add_points)(int* xy, int N, double scale, void* cookie),
                                               void* cookie);
bool find_chessboard_from_image_file_C(const char* filename, const int gridn, int image_pyramid_level, bool debug,
                                       bool (*add_points)(double* xy, int N, void* cookie), void* cookie);

/* The image decoder behind the two functions above and the command-line tool, on its own (host only, no
 * device needed): binary PGM (8 / 16 bit), non-interlaced PNG, baseline JPEG (see
 * mrgingham_amd_jpeg_coefficients for what is accepted), strip or tiled TIFF (see mrgingham_amd_tiff_layout
 * and _tiff_layout_tiled for what is accepted), Windows Bitmap (see mrgingham_amd_bmp_layout for what is accepted) and
 * binary PBM and PAM (see mrgingham_amd_pnm_header for what is accepted).
 * `out` (may be NULL: sizes only)
 * receives width*height grey bytes.  16-bit samples: cli_scaling = 0 keeps the high byte, what
 * cv::imread(IMREAD_GRAYSCALE) gives the file entry points; 1 rescales by 255/65535 with rounding, what
 * the CLI's convertTo does (mrgingham-from-image.cc:85-92).  Returns 0; -1 unreadable, unsupported or
 * malformed file (never throws, never reads or writes out of bounds on a crafted file; sides above
 * 32767 are rejected); -2 out_capacity too small (sizes are still reported). */
int mrgingham_amd_read_image(const char* filename, int cli_scaling, uint8_t* out, size_t out_capacity, int* width,
                             int* height, int* depth);

/* Baseline JPEG, first half (host only, no device needed): the marker parse and the Huffman decode of a file held in
 * memory.  What cv::imread(IMREAD_GRAYSCALE) gives for a grey or YCbCr file is the luma plane after libjpeg's default
 * integer inverse DCT, so only luma is kept: coef (may be NULL: sizes only) receives the quantised coefficients as int16
 * [blocks_h][blocks_w][64] -- row-major inside a block, blocks in raster order --, quant (may be NULL) the 64 entries of
 * the luma table in the same order.  blocks_w / blocks_h are the luma block counts padded to whole MCUs (4:2:0 at
 * 31 x 33: 4 x 6).  Accepted: SOF0 / SOF1 (sequential Huffman, 8 bit), 1 component or 3 taken as YCbCr with luma first and
 * at the frame's maximum sampling factors, one scan, 8- / 16-bit DQT, DHT / DRI anywhere before SOS, restart markers in
 * sequence exactly at the interval, APPn / COM skipped, EXIF orientation ignored (IMREAD_IGNORE_ORIENTATION).
 * Unreadable: progressive, arithmetic, lossless, 12 bit, 4 components, Adobe transform 0 (RGB), several scans, DNL /
 * height 0, sides above 32767, and ANY malformed stream (truncated data is not padded).  Returns 0; -1 unreadable (never
 * throws, never reads or writes out of bounds on a crafted file); -2 coef_capacity (in elements) too small (sizes and
 * quant are still reported). */
int mrgingham_amd_jpeg_coefficients(const uint8_t* data, size_t nbytes, int16_t* coef, size_t coef_capacity,
                                    uint16_t* quant, int* width, int* height, int* blocks_w, int* blocks_h);

/* Baseline JPEG, second half: dequantisation and the 8x8 inverse DCT of nframes frames on the device, bit for bit what
 * mrgingham_amd_read_image computes on the host (libjpeg's default integer transform; sums and products modulo 2^32 on
 * crafted input).  d_coef: frame f at d_coef + f*coef_pitch (ELEMENTS), laid out as above with the given blocks_w /
 * blocks_h (blocks_w*8 >= width, blocks_h*8 >= height, coef_pitch >= blocks_w*blocks_h*64; d_coef 16-byte aligned and
 * coef_pitch a multiple of 8).  d_quant: nframes x 64.  d_out: frame f row y at d_out + f*frame_pitch + y*stride; only
 * the width x height pixels are written, the bytes between width and stride stay untouched.  Asynchronous on `stream`
 * (NULL = default).  Arguments are checked like mrgingham_amd_preprocess_batch's (MRGINGHAM_AMD_ERR_ARG, nothing
 * written). */
int mrgingham_amd_jpeg_idct_batch(mrgingham_amd_ctx* ctx, const int16_t* d_coef, int64_t coef_pitch,
                                  const uint16_t* d_quant, int nframes, int width, int height, int blocks_w,
                                  int blocks_h, uint8_t* d_out, int64_t frame_pitch, int stride, void* stream);

/* The restart intervals of a baseline JPEG held in memory (host only, no device needed): what a decoder needs to
 * take the file apart into independent streams.  *restart_interval: MCUs per interval from the DRI segment, 0 when the
 * file has none (then *nintervals is 0).  offsets (may be NULL: counts only) receives *nintervals = ceil(MCUs /
 * restart_interval) pairs [begin, end) of byte offsets into `data`: an interval ends at the first FF that is not
 * followed by 00, or at the end of the file; then any number of FF and D0 + (i & 7) must follow, or the file is
 * unreadable; what follows the last interval is not examined.  The marker parse is mrgingham_amd_jpeg_coefficients' and
 * accepts what it accepts; the entropy-coded data is only searched for markers, so a file this call accepts may still
 * fail to decode.  Returns 0; -1 unreadable; -2 capacity (in pairs) too small (the counts are still reported). */
int mrgingham_amd_jpeg_restart_intervals(const uint8_t* data, size_t nbytes, int* restart_interval, int64_t* offsets,
                                         size_t capacity, size_t* nintervals);

/* How the self-synchronising decoder that option "jpeg_sync" switches on fares on a baseline JPEG held in memory (host
 * only, no device needed; the same decoder text and the same schedule as on the device, serially).  The entropy-coded
 * segment of the file's one scan is cut into *nsubsequences pieces of subsequence_bytes raw bytes (a multiple of 4 in
 * 8..1024); every piece is first decoded from its own first byte as if a block began there, then re-entered, round
 * after round, from the state its left neighbour ended in, until a round changes nothing: then every piece holds what
 * the serial decoder computes.  *rounds: the update rounds that changed at least one piece -- the device takes the file
 * iff that is at most option "jpeg_sync_max_rounds".  Returns 0 for a readable file without restart intervals; -1
 * unreadable (what mrgingham_amd_jpeg_coefficients calls unreadable, or a bad subsequence_bytes); -3 a readable file that
 * has restart intervals; -4 a readable file without them whose entropy-coded segment has 2^29 bytes or more (the device
 * leaves it to the host: status -3 of mrgingham_amd_jpeg_entropy_batch).  *rounds and *nsubsequences are 0 unless 0 is
 * returned. */
int mrgingham_amd_jpeg_sync_rounds(const uint8_t* data, size_t nbytes, int subsequence_bytes, int* rounds,
                                   size_t* nsubsequences);

/* The device twin of mrgingham_amd_jpeg_coefficients for files that carry restart markers: nfiles baseline JPEG files
 * held in memory, of ONE size, are Huffman-decoded ON THE DEVICE, one lane per restart interval; the host only finds the
 * markers and uploads the compressed bytes.  d_coef / d_quant receive what mrgingham_amd_jpeg_idct_batch takes: file f's
 * luma coefficients at d_coef + f*coef_pitch (elements) as int16 [blocks_h][blocks_w][64] with the GIVEN blocks_w /
 * blocks_h (a file's own block counts may be smaller: its blocks lie in the top left corner, the rest of its area is not
 * touched), its luma table at d_quant + f*64.  Int16 for int16 what mrgingham_amd_jpeg_coefficients gives, and a file
 * is accepted exactly when that function accepts it.  h_status[f]: 0 decoded; -1 unreadable; -2 another size (or block
 * counts above the given ones); -3 readable, but not taken by the device: the file has no restart interval, or one of
 * more than option "jpeg_entropy_max_interval" MCUs -- decode it with mrgingham_amd_jpeg_coefficients.  Every file whose
 * status is not 0 has its blocks_w*blocks_h*64 coefficients and its table zeroed.
 * With option "jpeg_sync" 1 the files WITHOUT restart intervals are decoded as well (see mrgingham_amd_jpeg_sync_rounds
 * for the method; one lane per "jpeg_sync_subsequence" bytes): 0 decoded, with the same coefficients and table; -1
 * unreadable; -3 not converged within "jpeg_sync_max_rounds" update rounds (or an entropy-coded segment of 2^29 bytes or
 * more), zeroed like the others.  Files with restart intervals are treated as without the option.  SYNCHRONOUS; runs on the context's
 * pixel stream, completes the find_boards jobs in flight first and restores the caller's HIP device.  Arguments are
 * checked like mrgingham_amd_jpeg_idct_batch's (MRGINGHAM_AMD_ERR_ARG, nothing written); width and height are at
 * least 1.  A corrupt file costs a status, never a fault: every index the stream supplies is checked on the device. */
int mrgingham_amd_jpeg_entropy_batch(mrgingham_amd_ctx* ctx, const uint8_t* const* data, const size_t* nbytes, int nfiles,
                                     int width, int height, int16_t* d_coef, int64_t coef_pitch, int blocks_w,
                                     int blocks_h, uint16_t* d_quant, int32_t* h_status);

/* nfiles baseline JPEG files of ONE size straight into device frames (layout as d_out above): nthreads host threads
 * (<= 0: all cores, at most 32) entropy-decode a chunk of files into page-locked staging while the chunk before it
 * uploads and runs mrgingham_amd_jpeg_idct_batch; the decoded pixels never exist on the host.  h_status[f]: 0 decoded,
 * -1 unreadable / unsupported / malformed, -2 a JPEG of another size; the frame of a failed file is zero-filled.
 * SYNCHRONOUS: d_out is complete on return.  Returns MRGINGHAM_AMD_OK also when files failed.  Completes the
 * find_boards jobs in flight first and restores the caller's HIP device.  The two device coefficient buffers stay within
 * 1 GiB of context scratch (12 MP: ~20 frames each; option "jpeg_chunk_frames").
 * With option "jpeg_entropy" 1 the host threads read the files and find their restart markers; the files that have
 * restart intervals (of at most "jpeg_entropy_max_interval" MCUs) are uploaded as compressed bytes and Huffman-decoded
 * on the device (mrgingham_amd_jpeg_entropy_batch's kernel) in front of the inverse DCT, the others are decoded by the
 * host threads as without the option.  Same frames, same statuses.
 * With option "jpeg_sync" 1 on top of it the files without restart intervals are uploaded as compressed bytes too and
 * decoded by the self-synchronising kernels in front of the inverse DCT.  Whether such a file converged within
 * "jpeg_sync_max_rounds" is known only once its chunk has passed the stream: the ones that did not are then decoded by
 * the host threads, uploaded, and the inverse DCT runs over their frames again.  Same frames, same statuses. */
int mrgingham_amd_read_jpegs_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width,
                                   int height, uint8_t* d_out, int64_t frame_pitch, int stride, int nthreads,
                                   int32_t* h_status);

/* PNG, first half (host only, no device needed): the chunk walk and the inflate of a file held in memory, under the rules
 * of mrgingham_amd_read_image's decoder -- IHDR first, once and 13 bytes long, sides at most 32767 (checked before
 * anything is sized), IDAT chunks concatenated, no interlace, 8 or 16 bits, colour types 0, 2, 3 (8 bit), 4, 6.  scan (may
 * be NULL: sizes only, nothing is inflated) receives the FILTERED scanlines as they leave zlib: row y at
 * scan + (rowbytes + 1) * y, its filter byte first, rowbytes = width * bpp with bpp = 1, 3, 2, 4 bytes for colour types
 * 0, 2, 4, 6 at 8 bit and twice that at 16.  Returns 0; MRGINGHAM_AMD_PNG_NOT_TAKEN for a readable file the device route
 * leaves to mrgingham_amd_read_image -- colour type 3, palette: sizes reported, scan untouched --; -1 for everything the
 * decoder rejects (interlace, other depths, chunk order, an inflate error or another inflated length) and for ANY filter
 * byte above 4, checked here so that the device never meets one; -2 scan_capacity (bytes) below (rowbytes + 1) * height
 * (sizes are still reported).  Never throws, never reads or writes out of bounds on a crafted file. */
#define MRGINGHAM_AMD_PNG_NOT_TAKEN -3
int mrgingham_amd_png_scanlines(const uint8_t* data, size_t nbytes, uint8_t* scan, size_t scan_capacity, int* width,
                                int* height, int* bits, int* color_type);

/* PNG, second half: the row filters (None, Sub, Up, Average, Paeth) undone and the samples reduced to grey for nframes
 * frames on the device, byte for byte what mrgingham_amd_read_image computes on the host.  d_scan: frame f's scanlines, as
 * above, at d_scan + f*scan_pitch (BYTES; d_scan 4-byte aligned, scan_pitch >= (width*bpp + 1)*height); every filter byte
 * is 0 .. 4 (mrgingham_amd_png_scanlines has checked it).  bits 8 or 16, color_type 0, 2, 4 or 6.  d_out: uint8_t frames
 * for bits 8, uint16_t frames for bits 16 (native endian, from the file's big-endian pairs); frame f row y at
 * d_out + f*frame_pitch + y*stride, ELEMENTS; only the width x height samples are written, what lies between width and
 * stride stays untouched.  Grey is the first channel of types 0 and 4, (R*4899 + G*9617 + B*1868 + 8192) >> 14 of types 2
 * and 6; alpha is ignored.  One workgroup per frame; asynchronous on `stream` (NULL = default); allocates nothing beyond
 * context scratch (one padded row per frame).  Arguments are checked like mrgingham_amd_jpeg_idct_batch's
 * (MRGINGHAM_AMD_ERR_ARG, nothing written). */
int mrgingham_amd_png_reconstruct_batch(mrgingham_amd_ctx* ctx, const uint8_t* d_scan, int64_t scan_pitch, int nframes,
                                        int width, int height, int bits, int color_type, void* d_out,
                                        int64_t frame_pitch, int stride, void* stream);

/* The two constants of that kernel's schedule, for tests that place their shapes on its seams: the rows of a frame in
 * flight at once (the lanes of its workgroup) and the pixels of a row a lane reconstructs per step. */
void mrgingham_amd_png_reconstruct_geometry(int* rows_in_flight, int* segment_pixels);

/* nfiles PNG files of ONE size and depth straight into device frames (layout and element type as d_out above): nthreads
 * host threads (<= 0: all cores, at most 32) inflate a chunk of files into page-locked staging while the chunk before it
 * uploads and runs mrgingham_amd_png_reconstruct_batch (one launch per run of files of one colour type); neither the
 * reconstructed nor the grey pixels exist on the host.  A palette file is decoded by the host threads with
 * mrgingham_amd_read_image's decoder and uploaded: same bytes.  h_status[f]: 0 decoded, -1 unreadable / unsupported /
 * malformed (or not a PNG), -2 a PNG of another size or depth; the frame of a failed file is zero-filled.  SYNCHRONOUS:
 * d_out is complete on return.  Returns MRGINGHAM_AMD_OK also when files failed.  Completes the find_boards jobs in
 * flight first and restores the caller's HIP device.  The chunk buffers are those of mrgingham_amd_read_jpegs_batch, within
 * the same 1 GiB (12 MP grey: ~40 files each; option "png_chunk_frames"). */
int mrgingham_amd_read_pngs_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height,
                                  int bits, void* d_out, int64_t frame_pitch, int stride, int nthreads,
                                  int32_t* h_status);

/* Binary PGM (P5).  The header of a file held in memory, whole or only its first nbytes (host only): the one parser behind
 * mrgingham_amd_read_image, _probe_image and _read_pgms_batch.  0: "P5", three decimal numbers separated by white space
 * and # comments, one byte after the last; sides 1 .. 32767, maxval 1 .. 65535; *bits 8 (maxval < 256) or 16,
 * *payload_offset the byte the samples begin at.  -1: not such a file, or a rule broken.  -2: the bytes end inside the
 * header (of a whole file: unreadable; of a file's first bytes: more are needed).  A file is readable when it holds
 * width*height*bits/8 bytes from *payload_offset on.  Any output pointer may be NULL. */
int mrgingham_amd_pgm_header(const uint8_t* data, size_t nbytes, int* width, int* height, int* bits, size_t* payload_offset);

/* PGM payloads to frames on the device: frame f's payload as it lies in the file -- width*height bytes for bits 8,
 * width*height BIG-ENDIAN pairs for bits 16 -- at d_payload + f*payload_pitch (BYTES; d_payload 16-byte aligned,
 * payload_pitch a multiple of 16 and >= width*height*bits/8).  d_out as for mrgingham_amd_png_reconstruct_batch: uint8_t
 * or native-endian uint16_t frames, frame f row y at d_out + f*frame_pitch + y*stride, ELEMENTS; only the width x height
 * samples are written, what lies between width and stride stays untouched.  d_out may be d_payload itself where the two
 * layouts coincide (stride == width, frame_pitch*bits/8 == payload_pitch): every sample is then read and written by the
 * same lane.  A streaming kernel, 16-byte loads, one byte permute per dword, 16-byte stores between a row's head and
 * tail; the launch is sized to the device.  Asynchronous on `stream` (NULL = default); allocates nothing.  Arguments are
 * checked like mrgingham_amd_png_reconstruct_batch's (MRGINGHAM_AMD_ERR_ARG, nothing written). */
int mrgingham_amd_pgm_unpack_batch(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, int nframes,
                                   int width, int height, int bits, void* d_out, int64_t frame_pitch, int stride,
                                   void* stream);

/* nfiles binary PGM files of ONE size and depth straight into device frames (layout and element type as d_out above):
 * per file a host thread (nthreads of them; <= 0: all cores, at most 32) parses the header and reads the payload from the
 * file straight into page-locked staging, at a 16-byte aligned offset -- no byte is swapped or copied a second time on the
 * host --; a chunk of files goes up in one copy and through one launch of mrgingham_amd_pgm_unpack_batch while the host
 * threads read the next.  h_status[f]: 0 loaded, -1 unreadable or not a PGM by mrgingham_amd_read_image's rules (a file
 * shorter than its header promises included), -2 a PGM of another size or depth; the frame of a failed file is
 * zero-filled.  SYNCHRONOUS: d_out is complete on return.  Returns MRGINGHAM_AMD_OK also when files failed.  Completes the
 * find_boards jobs in flight first and restores the caller's HIP device.  The chunk buffers are those of
 * mrgingham_amd_read_jpegs_batch, within the same 1 GiB (12 MP at 16 bit: ~20 files each; option "pgm_chunk_frames"). */
int mrgingham_amd_read_pgms_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height,
                                  int bits, void* d_out, int64_t frame_pitch, int stride, int nthreads,
                                  int32_t* h_status);

/* Windows Bitmap (BMP), host half (host only, no device needed): the one parser of a BMP's headers and palette, behind
 * mrgingham_amd_read_image, _probe_image (MRGINGHAM_AMD_KIND_BMP) and _read_bmps_batch.  `data` is a whole file held in memory.  The subset
 * is closed, and everything outside it is unreadable; every offset and product is checked in 64 bits against nbytes before
 * anything is sized from it:
 *   a "BM" file header; an info header of 40, 52, 56, 108 or 124 bytes (the 12-byte core header and the 64-byte OS/2 header:
 *   unreadable); planes 1; width 1 .. 32767, |height| 1 .. 32767, a negative height = top-down rows;
 *   bits 1, 4, 8 with compression 0: palette indices, the leftmost pixel in the most significant bits of a byte;
 *   bits 8 with compression 1 (RLE8), bottom-up only: the host decoder's alone (MRGINGHAM_AMD_BMP_NOT_TAKEN);
 *   bits 24 (B G R) and 32 (B G R X, the fourth byte ignored) with compression 0; bits 32 with compression 3 only with the
 *   masks R 0x00FF0000, G 0x0000FF00, B 0x000000FF, behind a 40-byte header or inside a longer one;
 *   16-bit files, RLE4, compressions 4, 5, 6, other masks, top-down RLE: unreadable.
 *   Palette (bits <= 8): clrUsed entries, 2^bits when it is 0, more than 2^bits unreadable; B G R x per entry behind the
 *   header (and its masks); it lies inside the file and ends at or before bfOffBits.  It is reduced to lut[256], the grey of
 *   every index ((4899 R + 9617 G + 1868 B + 8192) >> 14; entries the file does not define are 0, so an index beyond the
 *   palette reads 0); lut_identity: lut[i] == i for every index the depth can produce -- the grey camera file.
 *   Rows are row_bytes = ((width*bits + 31) / 32) * 4 bytes; an uncompressed file is readable only when it holds
 *   row_bytes * |height| bytes from payload_offset (bfOffBits) on.  bfSize and biSizeImage are neither trusted nor required.
 *   RLE8: the stream runs from bfOffBits to the end of the file -- encoded runs, absolute runs padded to even, end of line,
 *   end of bitmap, delta; pixels never written are index 0; a run that crosses the row's width or leaves the image is
 *   unreadable, and so is a stream that ends without end-of-bitmap before the last row was begun.
 * Returns 0: mrgingham_amd_bmp_unpack_batch takes the file; MRGINGHAM_AMD_BMP_NOT_TAKEN (-3): readable, but the host
 * decoder's alone (RLE8; the sizes and the table are reported); -1 unreadable.  info may be NULL.  Allocates nothing,
 * never throws.  The output is always 8-bit grey. */
typedef struct mrgingham_amd_bmp_info {
    int32_t width, height;  /* height: rows (positive, whatever the row order) */
    int32_t bits;           /* 1, 4, 8, 24, 32 */
    int32_t compression;    /* 0, 1 (RLE8), 3 (the one set of masks: pixels as with 0) */
    int32_t top_down;       /* 1: the first row of the pixel array is the top row */
    int32_t row_bytes;
    int64_t payload_offset; /* bfOffBits */
    uint8_t lut[256];
    int32_t lut_identity;
} mrgingham_amd_bmp_info;
#define MRGINGHAM_AMD_BMP_NOT_TAKEN -3
int mrgingham_amd_bmp_layout(const uint8_t* data, size_t nbytes, mrgingham_amd_bmp_info* info);

/* BMP pixel arrays to grey frames on the device: frame f's pixel array as it lies in the file -- height rows of row_bytes
 * bytes -- at d_payload + f*payload_pitch (BYTES; d_payload 16-byte aligned, payload_pitch a multiple of 16 and
 * >= row_bytes*height), its grey table at d_lut + 256*f (not read for bits 24 and 32, nor for bits 8 with lut_identity;
 * may then be NULL).  d_out: uint8_t frames, frame f row y at d_out + f*frame_pitch + y*stride; only the width x height
 * samples are written, what lies between width and stride stays untouched; d_out may sit at any byte address.  Row y of a
 * frame is row height-1-y of its pixel array unless top_down.  One streaming launch sized to the device: a lane produces
 * one 16-byte word of a destination row per step from the 2, 8, 16, 48 or 64 source bytes of its 16 pixels, read as
 * aligned dwords and never beyond the row's padded length, with the text the host decoder runs (csrc/bmp_pixels.h).
 * Asynchronous on `stream` (NULL = default); allocates nothing.  Arguments are checked like mrgingham_amd_pgm_unpack_batch's
 * (MRGINGHAM_AMD_ERR_ARG, nothing written); bits outside {1, 4, 8, 24, 32} are refused. */
int mrgingham_amd_bmp_unpack_batch(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch,
                                   const uint8_t* d_lut, int nframes, int width, int height, int bits, int top_down,
                                   int lut_identity, uint8_t* d_out, int64_t frame_pitch, int stride, void* stream);

/* the schedule of that launch: lanes per workgroup, and the workgroups per compute unit the grid is capped at; a row is
 * taken by the power of two of lanes that covers its 16-byte words, so a launch has
 * CUs * max_workgroups_per_cu * (lanes_per_workgroup / lanes of a row) row slots and loops over the rows beyond */
void mrgingham_amd_bmp_unpack_geometry(int* lanes_per_workgroup, int* max_workgroups_per_cu);

/* nfiles BMP files of ONE size straight into device frames (uint8, layout as d_out above); depth, row order and palette
 * may differ from file to file.  Per file a host thread (nthreads of them; <= 0: all cores, at most 32) reads the header
 * bytes, runs mrgingham_amd_bmp_layout and reads the grey table and the pixel array from the file straight into page-locked
 * staging, at a 16-byte aligned offset -- no sample is touched on the host --; a chunk of files goes up in one copy and
 * through one launch of mrgingham_amd_bmp_unpack_batch per run of files with equal bits, row order and lut_identity while
 * the host threads read the next.  An RLE8 file is decoded by its host thread and copied into its frame.  h_status[f]: 0
 * loaded, -1 unreadable or not a BMP by mrgingham_amd_read_image's rules, -2 a BMP of another size; the frame of a failed
 * file is zero-filled.  SYNCHRONOUS: d_out is complete on return.  Returns MRGINGHAM_AMD_OK also when files failed.
 * Completes the find_boards jobs in flight first and restores the caller's HIP device.  The chunk buffers are those of
 * mrgingham_amd_read_jpegs_batch, within the same 1 GiB (options "bmp_chunk_frames", "bmp_unpack"). */
int mrgingham_amd_read_bmps_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height,
                                  uint8_t* d_out, int64_t frame_pitch, int stride, int nthreads, int32_t* h_status);

/* Binary Netpbm beyond P5 (PBM "P4", PAM "P7"), host half (host only, no device needed): the one parser of a
 * Netpbm header, behind mrgingham_amd_read_image, _probe_image (MRGINGHAM_AMD_KIND_PNM) and _read_pnms_batch.  `data` is a whole file held
 * in memory, or its first bytes.  The subset is closed, and everything outside it is unreadable:
 *   Sides are 1 .. 32767.  Every product is checked in 64 bits against the file size before anything is sized from it.  A
 *   file shorter than its header promises is unreadable.  Trailing bytes are ignored, as for P5.  Samples are never rescaled
 *   by maxval, which is the library's P5 rule.
 *   P4: magic, width, height.  White space and # comments are handled as in mrgingham_amd_pgm_header.  ONE white-space byte
 *     follows the last number.  Rows are (width + 7) / 8 bytes, most significant bit first.  Bit 1 is black and reads 0.
 *     Bit 0 reads 255.  Depth is reported as 8.
 *   P5: exactly mrgingham_amd_pgm_header's verdicts and outputs (MRGINGHAM_AMD_KIND_PGM, unchanged; the payload is not measured here).
 *   P6: unreadable, as before (tests/test_pgm_header.py pins such a file); R G B comes as P7 of depth 3.
 *   P7: line 1 is "P7".  Then come lines of WIDTH, HEIGHT, DEPTH, MAXVAL, each followed by a decimal number.  Each must
 *     appear exactly once, in any order.  TUPLTYPE lines may appear any number of times.  # lines and empty lines are
 *     ignored.  A line ENDHDR closes the header.  The raster begins right behind its newline.  Any other token, a missing
 *     or repeated field, or a DEPTH outside 1 .. 4 makes the file unreadable.  DEPTH decides the layout: 1 is grey, 2 is
 *     grey plus an ignored sample, 3 is R G B, 4 is R G B plus an ignored sample.  Alpha is ignored, as PNG's is.  Samples
 *     are one byte each below maxval 256, big-endian pairs from 256 on.  Grey of R G B is (4899 R + 9617 G + 1868 B + 8192)
 *     >> 14, at 16 bits on the 16-bit samples, as 16-bit RGB PNG does.  A first
 *     TUPLTYPE that begins with BLACKANDWHITE is taken only with depth 1 or 2 and maxval 1.  The first sample then reads
 *     255 when non-zero and 0 otherwise.  With any other depth or maxval such a file is unreadable.  TUPLTYPE is otherwise
 *     not judged.
 *   ASCII Netpbm (P1, P2, P3), PAM depths above 4: unreadable.  Of a multi-image stream the first image is read.
 * Byte identity with cv::imread on colour files is not claimed, as for PNG, TIFF and BMP (its conversion depends on the
 * codec build).
 * Returns 0; -1 unreadable; MRGINGHAM_AMD_PNM_HEADER_CUT (-2): the bytes end inside the header (of a whole file:
 * unreadable; of a file's first bytes: more are needed).  info may be NULL.  Allocates nothing, never throws. */
typedef struct mrgingham_amd_pnm_info {
    int32_t width, height;
    int32_t bits;            /* of a sample in the file: 1 (P4), 8, 16 */
    int32_t channels;        /* samples per pixel, 1 .. 4; the grey comes from the first (1, 2) or the first three (3, 4) */
    int32_t black_and_white; /* 1: the first sample reads 255 when non-zero and 0 otherwise (P7 BLACKANDWHITE) */
    int32_t magic;           /* the digit: 4, 5, 6, 7 */
    int32_t row_bytes;       /* (width + 7) / 8, or width * channels * bits / 8: rows follow each other without padding */
    int64_t payload_offset;
} mrgingham_amd_pnm_info;
#define MRGINGHAM_AMD_PNM_HEADER_CUT -2
int mrgingham_amd_pnm_header(const uint8_t* data, size_t nbytes, mrgingham_amd_pnm_info* info);

/* Netpbm rasters to grey frames on the device: frame f's raster as it lies in the file -- height rows of row_bytes bytes,
 * row y at byte y * row_bytes, whatever its alignment -- at d_payload + f*payload_pitch (BYTES; d_payload 16-byte aligned,
 * payload_pitch a multiple of 16 and >= row_bytes*height).  bits 1: packed bits (channels 1); bits 8 and 16: channels
 * 1 .. 4 samples per pixel, big-endian pairs at 16; black_and_white only with bits 8 and channels 1 or 2.  d_out: uint8_t
 * frames for bits 1 and 8, native uint16_t frames for bits 16; frame f row y at d_out + f*frame_pitch + y*stride (SAMPLES);
 * only the width x height samples are written, what lies between width and stride stays untouched; d_out may sit at any
 * byte address (any even address at 16 bits).  One streaming launch sized to the device: a lane produces one 16-byte word
 * of a destination row per step from the source bytes of its 16 (8 at 16 bits) pixels, read as aligned dwords, each once
 * and none behind the payload's padded area, with the text the host decoder runs (csrc/pnm_pixels.h).  Asynchronous on
 * `stream` (NULL = default); allocates nothing.  Arguments are checked like mrgingham_amd_bmp_unpack_batch's
 * (MRGINGHAM_AMD_ERR_ARG, nothing written). */
int mrgingham_amd_pnm_unpack_batch(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, int nframes,
                                   int width, int height, int bits, int channels, int black_and_white, void* d_out,
                                   int64_t frame_pitch, int stride, void* stream);

/* the schedule of that launch: lanes per workgroup, and the workgroups per compute unit the grid is capped at; a row is
 * taken by the power of two of lanes that covers its 16-byte words, so a launch has
 * CUs * max_workgroups_per_cu * (lanes_per_workgroup / lanes of a row) row slots and loops over the rows beyond */
void mrgingham_amd_pnm_unpack_geometry(int* lanes_per_workgroup, int* max_workgroups_per_cu);

/* nfiles binary Netpbm files (P4, P5, P7 in any mix) of ONE size and output depth (bits 8: uint8 frames -- P4 files and
 * files of maxval below 256; bits 16: uint16 frames) straight into device frames (layout as d_out above).  Per file a host
 * thread (nthreads of them; <= 0: all cores, at most 32) reads the header bytes, runs mrgingham_amd_pnm_header and reads
 * the raster from the file straight into page-locked staging, at a 16-byte aligned offset -- no sample is touched on the
 * host --; a chunk of files goes up in one copy and through one launch of mrgingham_amd_pnm_unpack_batch per run of files
 * with the same layout while the host threads read the next.  h_status[f]: 0 loaded, -1 unreadable or not Netpbm by
 * mrgingham_amd_read_image's rules, -2 another size or depth; the frame of a failed file is zero-filled.  SYNCHRONOUS:
 * d_out is complete on return.  Returns MRGINGHAM_AMD_OK also when files failed.  Completes the find_boards jobs in flight
 * first and restores the caller's HIP device.  The chunk buffers are those of mrgingham_amd_read_jpegs_batch, within the
 * same 1 GiB (options "pnm_chunk_frames", "pnm_unpack"). */
int mrgingham_amd_read_pnms_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height,
                                  int bits, void* d_out, int64_t frame_pitch, int stride, int nthreads, int32_t* h_status);

/* Packed camera frames: 10, 12 or 14-bit samples as machine-vision cameras and frame grabbers deliver them.  A frame is
 * `height` rows; row y begins at byte y * row_bytes of the frame's payload; nothing is shared between rows, and row_bytes
 * may exceed the minimum (row padding).  The layouts, which govern (the names are the common ones):
 *   MRGINGHAM_AMD_RAW_P10 / _P12 / _P14 (GenICam Mono10p / Mono12p / Mono14p), N = 10 / 12 / 14: a row is one bit stream,
 *     least significant bit first: stream bit b is bit b % 8 of byte b / 8; sample x is the stream bits [x*N, (x+1)*N),
 *     least significant first.  Minimum row_bytes: ceil(width*N/8).
 *   MRGINGHAM_AMD_RAW_GEV10 / _GEV12 (GigE Vision Mono10Packed / Mono12Packed), L = 2 / 4: pixels 2g, 2g+1 are the bytes
 *     3g .. 3g+2: p0 = byte0 << L | (byte1 & (2^L - 1)), p1 = byte2 << L | ((byte1 >> 4) & (2^L - 1)); with L = 2 the
 *     bits 2, 3, 6, 7 of byte1 are ignored.  Minimum row_bytes: 3*ceil(width/2).
 * The output is the sample as it is, 0 .. 2^N - 1, in a native uint16_t -- not left-justified (mrgingham_amd_preprocess16_batch
 * normalises by min/max).  Every bit pattern is a valid frame; padding bits and bytes are not looked at.  Rows that begin
 * inside a byte (one bit stream across a whole frame) and MSB-first streams are not read.  The samples of a colour camera
 * (BayerRG12p and the like) come out as they are, a mosaic; mrgingham_amd_bayer_grey_batch below takes it to grey. */
#define MRGINGHAM_AMD_RAW_P10 0
#define MRGINGHAM_AMD_RAW_P12 1
#define MRGINGHAM_AMD_RAW_P14 2
#define MRGINGHAM_AMD_RAW_GEV10 3
#define MRGINGHAM_AMD_RAW_GEV12 4

/* the minimum row_bytes of the table above; -1 for a format that is none of the five or a width outside 1 .. 32767 */
int64_t mrgingham_amd_raw_row_bytes(int width, int format);

/* One packed frame to uint16 samples on the HOST (no device needed; the text the kernel runs, csrc/raw_pixels.h): row y of
 * `out` begins at out + y*stride (ELEMENTS, stride >= width); only the width x height samples are written.  `payload` may
 * sit at any address; no byte at or beyond payload + nbytes is read.  MRGINGHAM_AMD_ERR_ARG, with nothing written, for a
 * NULL pointer, a bad format, sides outside 1 .. 32767, row_bytes below the minimum, stride < width or
 * nbytes < (height-1)*row_bytes + minimum.  This is the route a caller without the device call has; it is not a fallback
 * of mrgingham_amd_raw_unpack_batch. */
int mrgingham_amd_raw_unpack_image(const uint8_t* payload, size_t nbytes, int width, int height, int64_t row_bytes, int format,
                                   uint16_t* out, int stride);

/* Packed frames to uint16 frames on the device: frame f's payload at d_payload + f*payload_pitch (BYTES; d_payload 16-byte
 * aligned, payload_pitch a multiple of 16 and >= (height-1)*row_bytes + minimum; row_bytes at least the minimum, sides
 * 1 .. 32767).  d_out, frame_pitch and stride as for mrgingham_amd_pgm_unpack_batch: native uint16_t frames, frame f row y
 * at d_out + f*frame_pitch + y*stride, ELEMENTS, d_out at any even address; only the width x height samples are written,
 * what lies between width and stride stays untouched.  Input and output must not overlap.  One streaming launch sized to
 * the device: a lane produces one 16-byte word (8 samples) of a destination row per step from their 10 / 12 / 14 source
 * bytes, read as the aligned dwords that cover them, each once, and none beyond d_payload + nframes*payload_pitch.
 * Asynchronous on `stream` (NULL = default); allocates nothing.  Every violation is MRGINGHAM_AMD_ERR_ARG with nothing
 * written. */
int mrgingham_amd_raw_unpack_batch(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, int nframes,
                                   int width, int height, int64_t row_bytes, int format, uint16_t* d_out, int64_t frame_pitch,
                                   int stride, void* stream);

/* the schedule of that launch, as mrgingham_amd_pnm_unpack_geometry's */
void mrgingham_amd_raw_unpack_geometry(int* lanes_per_workgroup, int* max_workgroups_per_cu);

/* Bayer mosaics to grey frames, 8 and 16 bit.  The definition, which governs (the names are the common ones):
 *
 * Inputs.  A mosaic is height x width samples of one dtype, uint8 or native uint16, any values.  Sides are 2 .. 32767.
 * The pattern names the colours of pixels (0,0), (0,1), (1,0), (1,1), repeated with period 2 in both directions:
 *   MRGINGHAM_AMD_BAYER_RGGB 0 (GenICam BayerRG), _GRBG 1 (BayerGR), _GBRG 2 (BayerGB), _BGGR 3 (BayerBG).
 * Borders.  Samples outside the frame are taken by reflect-101 (index -1 is 1, index n is n-2), which keeps the colour
 * phase.
 * Sums.  Let v be the sample at the pixel, and: cross = N + S + W + E; diag = the four diagonal neighbours; hor = W + E;
 * ver = N + S.
 * Coefficients.  cR = 4899, cG = 9617, cB = 1868.  They sum to 16384.
 * Output.  The output has the same dtype as the input.  It is rounded once, in unsigned 32-bit arithmetic:
 *   red site: (4*cR*v + cG*cross + cB*diag + 32768) >> 16
 *   blue site: the same with cR and cB exchanged
 *   green site in a row whose other colour is red: (2*cG*v + cR*hor + cB*ver + 16384) >> 15
 *   green site in a row whose other colour is blue: the same with cR and cB exchanged
 * This is bilinear demosaicing followed by the fixed-point luma the colour readers use, folded into one rounding.  The
 * largest intermediate is 4*16384*65535 + 32768, which is below 2^32.  A constant mosaic comes out unchanged.  Nothing is
 * edge-aware, white-balanced or colour; 16-bit input gives 16-bit output. */
#define MRGINGHAM_AMD_BAYER_RGGB 0
#define MRGINGHAM_AMD_BAYER_GRBG 1
#define MRGINGHAM_AMD_BAYER_GBRG 2
#define MRGINGHAM_AMD_BAYER_BGGR 3

/* One mosaic to grey on the HOST (no device needed; the text the kernel runs, csrc/bayer_pixels.h): bits 8 (uint8_t) or 16
 * (native uint16_t); row y of the mosaic begins at mosaic + y*stride, row y of the output at out + y*out_stride, ELEMENTS,
 * at any address.  Only the width x height outputs are written.  MRGINGHAM_AMD_ERR_ARG, with nothing written, for a NULL
 * pointer, a bad pattern, bits outside 8 / 16, sides outside 2 .. 32767 or a stride below the width.  `out` must not
 * overlap the mosaic.  This is the route a caller without the device call has; it is not a fallback of
 * mrgingham_amd_bayer_grey_batch. */
int mrgingham_amd_bayer_grey_image(const void* mosaic, int bits, int width, int height, int64_t stride, int pattern, void* out,
                                   int64_t out_stride);

/* Mosaics to grey frames on the device: frame f row y at d_in + f*in_frame_pitch + y*in_stride and at
 * d_out + f*out_frame_pitch + y*out_stride, ELEMENTS of bits / 8 bytes, at any element-aligned address and any stride
 * >= width (torch views); frames of the output must not overlap each other (out_frame_pitch >= (height-1)*out_stride +
 * width where nframes > 1), those of the input may.  Only the width x height outputs of a frame are written.  Input and
 * output must not overlap: the stencil reads its neighbours, so the call cannot work in place.  One streaming launch: a
 * lane owns a column of 16-byte destination words and rolls down a slab of rows with three source rows in registers;
 * whole words that are 16-byte aligned leave as one store, the ends of a row and unaligned rows sample by sample.  It reads
 * the aligned dwords that hold samples of the frames and no others.  Asynchronous on `stream` (NULL = default);
 * allocates nothing; nframes == 0 is OK.  Every other violation is MRGINGHAM_AMD_ERR_ARG with nothing launched. */
int mrgingham_amd_bayer_grey_batch(mrgingham_amd_ctx* ctx, const void* d_in, int bits, int nframes, int width, int height,
                                   int64_t in_frame_pitch, int64_t in_stride, int pattern, void* d_out, int64_t out_frame_pitch,
                                   int64_t out_stride, void* stream);

/* the schedule of that launch: the lanes of a workgroup (side by side along a row, one 16-byte word each), the rows of a
 * slab, and the workgroups per CU the grid is capped at (0: it is not capped, one workgroup per slab and span of a row) */
void mrgingham_amd_bayer_grey_geometry(int* lanes_per_workgroup, int* rows_per_slab, int* max_workgroups_per_cu);

/* Colour frames to grey frames, 8 and 16 bit.  The definition, which governs:
 *
 * Inputs.
 * - Frames of `height` x `width` pixels, sides 1 .. 32767.
 * - Samples are `uint8`, or native-endian `uint16` where the format allows it.
 * - Formats (`MRGINGHAM_AMD_COLOUR_*`, Python names in brackets):
 *
 *   value  name                          layout                                                       bits
 *   0      RGB ("rgb")                   interleaved, 3 samples per pixel, R G B                      8, 16
 *   1      BGR ("bgr")                   interleaved, 3 samples per pixel, B G R                      8, 16
 *   2      RGBA ("rgba")                 interleaved, 4 samples, the fourth ignored                   8, 16
 *   3      BGRA ("bgra")                 interleaved, 4 samples, the fourth ignored                   8, 16
 *   4      RGB_PLANAR ("rgb_planar")     three planes R, G, B, `plane_pitch` elements apart           8, 16
 *   5      BGR_PLANAR ("bgr_planar")     three planes B, G, R, `plane_pitch` elements apart           8, 16
 *   6      YUYV ("yuyv")                 2 bytes per pixel, Y of pixel x at byte 2x                   8
 *   7      UYVY ("uyvy")                 2 bytes per pixel, Y of pixel x at byte 2x+1                 8
 *
 * Output.
 * - A grey frame of the input's sample type.
 * - Formats 0-5: `grey = (4899 R + 9617 G + 1868 B + 8192) >> 14`, unsigned 32-bit.  The largest intermediate is
 *   `65535*16384 + 8192 < 2^32`.  This is `png_grey` itself, called, not restated.
 * - The fourth sample of formats 2 and 3 is never looked at.  There is no compositing and no premultiplication, as in the
 *   PNG type 6 and PAM depth 4 readers.
 * - Formats 6 and 7: the Y byte as it is.  There is no range expansion, and the chroma bytes are never looked at.  Any
 *   width is allowed, odd ones included.
 * - Known answers:
 *   - 8 bit: pure R, G, B at 255 give 76, 150, 29.
 *   - 16 bit: pure R, G, B at 65535 give 19596, 38467, 7472.
 *   - Equal samples v in all three channels give v.
 *
 * (The expression is png_grey's -- csrc/png_filter.h, the one formula of the colour file readers -- written in
 * csrc/colour_pixels.h with the weights of the first and the third sample as two values that change places between the
 * R G B and the B G R orders; the tests hold it equal to png_grey through the PNG and PAM readers.)
 *
 * Not done: YUV to RGB or chroma of any kind; 4:2:0 / NV12 / P010 (their Y plane is already a [B,H,W] view that the existing
 * calls take); 10-bit packed YUV; XRGB / ARGB orders; float samples; 8-bit output from 16-bit input; a file or tool route. */
#define MRGINGHAM_AMD_COLOUR_RGB 0
#define MRGINGHAM_AMD_COLOUR_BGR 1
#define MRGINGHAM_AMD_COLOUR_RGBA 2
#define MRGINGHAM_AMD_COLOUR_BGRA 3
#define MRGINGHAM_AMD_COLOUR_RGB_PLANAR 4
#define MRGINGHAM_AMD_COLOUR_BGR_PLANAR 5
#define MRGINGHAM_AMD_COLOUR_YUYV 6
#define MRGINGHAM_AMD_COLOUR_UYVY 7

/* One colour frame to grey on the HOST (no device needed; the text the kernel runs, csrc/colour_pixels.h): bits 8 (uint8_t)
 * or 16 (native uint16_t); row y of the image begins at image + y*stride (planar: plane k's at image + k*plane_pitch +
 * y*stride), row y of the output at out + y*out_stride, ELEMENTS of the sample type.  stride >= samples per pixel x width
 * (3, 4, or 2 for the 4:2:2 forms; planar: >= width); plane_pitch >= 0 is read for formats 4 and 5 only.  It reads and
 * writes bytewise, at any address, and no byte outside the samples of the frame; only the width x height outputs are
 * written.  MRGINGHAM_AMD_ERR_ARG, with nothing written, for a NULL pointer, a bad format, bits outside 8 / 16, 16 bits with
 * formats 6 / 7, sides outside 1 .. 32767, a stride below a row or a negative plane_pitch.  `out` must not overlap the
 * image.  This is the route a caller without the device call has; it is not a fallback of mrgingham_amd_colour_grey_batch. */
int mrgingham_amd_colour_grey_image(const void* image, int bits, int format, int width, int height, int64_t stride,
                                    int64_t plane_pitch, void* out, int64_t out_stride);

/* Colour frames to grey frames on the device: frame f row y at d_in + f*in_frame_pitch + y*in_stride (planar: plane k's at
 * + k*in_plane_pitch) and at d_out + f*out_frame_pitch + y*out_stride, ELEMENTS of bits / 8 bytes, at any element-aligned
 * address (torch views).  in_stride >= samples per pixel x width (planar: >= width), out_stride >= width; in_plane_pitch
 * >= 0 is read for formats 4 and 5 only (planes may lie further apart than frames); an in_frame_pitch of 0 (an expanded
 * view) is allowed.  Only the width x height outputs of a frame are written.  One streaming launch on the row schedule of
 * the unpack kernels: a lane produces one 16-byte word of a destination row per step from the source bytes of its
 * pixels, read as 16-byte loads where their address allows it, else as the aligned dwords that hold them; it reads the
 * aligned dwords that hold samples of the frames and no others.  Asynchronous on `stream` (NULL = default); allocates
 * nothing; nframes == 0 is OK.  MRGINGHAM_AMD_ERR_ARG with nothing launched and nothing written for: a NULL pointer or
 * context; a bad format, bits outside 8 / 16, or 16 bits with formats 6 / 7; sides outside 1 .. 32767; strides below a row,
 * negative pitches, an odd uint16 address; output frames that overlap each other; output that overlaps any byte of the
 * input's extent (first to last sample of all frames), with "overlap" in mrgingham_amd_last_error. */
int mrgingham_amd_colour_grey_batch(mrgingham_amd_ctx* ctx, const void* d_in, int bits, int format, int nframes, int width,
                                    int height, int64_t in_frame_pitch, int64_t in_plane_pitch, int64_t in_stride, void* d_out,
                                    int64_t out_frame_pitch, int64_t out_stride, void* stream);

/* the schedule of that launch, as mrgingham_amd_pnm_unpack_geometry's */
void mrgingham_amd_colour_grey_geometry(int* lanes_per_workgroup, int* max_workgroups_per_cu);

/* TIFF, host half (host only, no device needed): the one parser of a TIFF's first image file directory, behind
 * mrgingham_amd_read_image, _probe_image and _read_tiffs_batch.  `data` is a whole file held in memory.  The subset is
 * closed, and everything outside it is unreadable; every field is checked before anything is sized from it:
 *   classic TIFF (magic 42; BigTIFF is unreadable), byte orders II and MM, the first IFD only; the entries looked at have
 *   type BYTE, SHORT or LONG, inline or at an offset, offsets and counts checked against nbytes in 64 bits; a tag twice is
 *   unreadable; ImageWidth, ImageLength, BitsPerSample, PhotometricInterpretation, StripOffsets and StripByteCounts are
 *   required;
 *   BitsPerSample 8 or 16, one value per sample, all equal; SampleFormat absent or 1; SamplesPerPixel 1 .. 4 (samples
 *   behind the first -- grey -- or the third -- RGB -- are extra samples and ignored); PlanarConfiguration, FillOrder and
 *   Orientation absent or 1; Photometric 0 (WhiteIsZero: read as maxval - v), 1, or 2 (RGB, at least 3 samples: grey is
 *   (R*4899 + G*9617 + B*1868 + 8192) >> 14); strips only HERE (any tile tag: unreadable to this function and to
 *   _tiff_layout_ex; mrgingham_amd_tiff_layout_tiled reads tiled files), RowsPerStrip absent or above the
 *   height = one strip, the last strip may be short, strips lie anywhere in the file in any order; sides 1 .. 32767;
 *   Compression 1 (none), 5 (LZW: MSB-first codes of 9 .. 12 bits, ClearCode 256, EOI 257, the width growing one code
 *   early), 32773 (PackBits, a run never crossing its row), 8 and 32946 (Deflate); Predictor absent, 1 or 2 (horizontal
 *   differences per sample, mod 2^bits, on 16-bit samples in value order).
 * A strip whose byte count cannot give its rows -- uncompressed: fewer bytes than rows x rowbytes; compressed: fewer than
 * the best ratio of the scheme allows -- makes the file unreadable here; whether a compressed strip gives EXACTLY its
 * rows x rowbytes is the decoder's to find out (LZW: a code above the next free one, a non-clear code after code 4095 has
 * been assigned, EOI or the end of the strip's bytes before its bytes are out; what follows the last needed code is
 * ignored; the decoder starts cleared whether or not the stream opens with ClearCode).
 * Outputs: *info (may be NULL); strips (may be NULL: counts only) receives up to `capacity` records, strip i covering
 * rows [first_row, first_row + rows) from `nbytes` bytes at `offset` of the file; *nstrips (may be NULL) the number of
 * strips.  lzw_max_strip: the decoded bytes of an LZW strip above which the file is left to the host decoder (<= 0 or
 * above 2^20: 2^20, the limit of the kernel's table entries; option "tiff_lzw_max_strip" of a context).
 * Returns 0: mrgingham_amd_tiff_decode_batch takes the file (compression 1 or 5); MRGINGHAM_AMD_TIFF_NOT_TAKEN: readable,
 * but mrgingham_amd_read_image's decoder alone reads it (PackBits, Deflate, an LZW strip above lzw_max_strip), outputs as
 * for 0; -1: unreadable; -2: capacity below the strip count (*info and *nstrips are still reported).  Never throws,
 * allocates nothing, never reads out of bounds on a crafted file. */
#define MRGINGHAM_AMD_TIFF_NOT_TAKEN -3
typedef struct mrgingham_amd_tiff_info {
    int32_t width, height, bits, samples, photometric, compression, predictor, big_endian;
} mrgingham_amd_tiff_info;
typedef struct mrgingham_amd_tiff_strip {
    int64_t offset, nbytes;   /* in the file */
    int32_t first_row, rows;  /* of the image */
} mrgingham_amd_tiff_strip;
int mrgingham_amd_tiff_layout(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, mrgingham_amd_tiff_info* info,
                              mrgingham_amd_tiff_strip* strips, size_t capacity, size_t* nstrips);

/* mrgingham_amd_tiff_layout that also takes Deflate files (compression 8 and 32946) whose strips each decode to at most
 * deflate_max_strip bytes (above 2^20: 2^20; option "tiff_deflate_max_strip" of a context): it returns 0 for them, and
 * MRGINGHAM_AMD_TIFF_NOT_TAKEN with a larger strip, and with a strip of more bytes in the file than what it decodes to
 * plus an eighth plus 512: a Deflate block need not give a byte, so a lane's work goes with the strip's bytes, and no zlib
 * stream of the rows needs more (such a file keeps the host decoder, which reads it as before).  deflate_max_strip <= 0: no Deflate file is taken, which is
 * mrgingham_amd_tiff_layout.  A Deflate strip is a zlib stream (RFC 1950 around RFC 1951) and the contract is zlib's: the
 * device accepts a strip exactly when uncompress() into a buffer of exactly rows x rowbytes returns Z_OK with that many
 * bytes, which is the host decoder's test -- the decoder goes on behind the last byte to the final block and checks the
 * Adler-32; bytes behind the trailer are ignored (csrc/tiff_inflate.h). */
int mrgingham_amd_tiff_layout_ex(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, int64_t deflate_max_strip,
                                 mrgingham_amd_tiff_info* info, mrgingham_amd_tiff_strip* strips, size_t capacity,
                                 size_t* nstrips);

/* mrgingham_amd_tiff_layout_ex that also reads TILED files: the parser behind mrgingham_amd_read_image, _probe_image and
 * _read_tiffs_batch.  (mrgingham_amd_tiff_layout and _tiff_layout_ex go on calling a file with any tile tag unreadable:
 * their callers hand the records to mrgingham_amd_tiff_decode_batch, which would read tiles as strips.)
 * A file is tiled when TileWidth (322), TileLength (323), TileOffsets (324) and TileByteCounts (325) are all present and
 * neither StripOffsets nor StripByteCounts is; any other mixture of tile and strip tags is unreadable.  RowsPerStrip in a
 * tiled file is ignored.  Everything else of the subset above holds, and on top of it: tile width tw and length tl
 * 1 .. 32767 each (any value, multiples of 16 or not); across = ceil(width / tw), down = ceil(height / tl), and both count
 * tags hold exactly across x down values; tile i (row-major) covers the image's rows from (i / across) x tl and its columns
 * from (i % across) x tw; every tile decodes to exactly tl x tw x samples x bits/8 bytes -- tiles at the right and bottom
 * edges are padded to the full size, and the padding may hold anything; predictor 2 runs along each row OF A TILE and
 * restarts at every tile's left edge; PackBits runs do not cross a tile's row.  The rules on a byte count that cannot give
 * its rows hold per tile, with the tile's full size.
 * A strip file: exactly mrgingham_amd_tiff_layout_ex, with *tile_width = *tile_length = 0.  A tiled file: *tile_width = tw,
 * *tile_length = tl, record i is tile i with first_row = (i / across) x tl and rows = tl (what it decodes to, not what the
 * image keeps of it), *nrecords = across x down.  Returns 0 when mrgingham_amd_tiff_decode_batch_tiled takes the file: tw a
 * multiple of 16, compression 1, or 5 with every tile decoding to at most lzw_max_strip bytes, or 8 / 32946 with
 * deflate_max_strip > 0, every tile decoding to at most that and held in no more bytes than its decoded size plus an
 * eighth plus 512; otherwise MRGINGHAM_AMD_TIFF_NOT_TAKEN, -1 or -2 as above.  tile_width and tile_length may be NULL (a
 * tiled file is read all the same).  Never throws, allocates nothing, never reads out of bounds on a crafted file. */
int mrgingham_amd_tiff_layout_tiled(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, int64_t deflate_max_strip,
                                    mrgingham_amd_tiff_info* info, int32_t* tile_width, int32_t* tile_length,
                                    mrgingham_amd_tiff_strip* records, size_t capacity, size_t* nrecords);

/* TIFF, device half: nframes files of ONE size, depth, sample count, photometric, compression (1, 5, or 8 / 32946),
 * predictor and byte order (`info`, HOST; what mrgingham_amd_tiff_layout or _tiff_layout_ex reported for every one of them) from their bytes to grey frames,
 * byte for byte what mrgingham_amd_read_image computes.  d_files: file f's bytes at d_files + f*file_pitch (BYTES; d_files
 * 16-byte aligned, file_pitch a multiple of 16).  d_strips (DEVICE): file f's strip records, as mrgingham_amd_tiff_layout
 * wrote them, at d_strips + f*strips_pitch, d_nstrips[f] (DEVICE) of them, at most strips_pitch.  d_out: uint8_t frames
 * for bits 8, native-endian uint16_t frames for bits 16; frame f row y at d_out + f*frame_pitch + y*stride, ELEMENTS; only
 * the width x height samples are written, what lies between width and stride stays untouched.  d_status (DEVICE, nframes
 * words, written): 0 decoded; -1 an LZW or Deflate strip broke a rule of the decoder, or a strip record does not fit its file or
 * frame (offset + nbytes above file_pitch, rows outside the frame or not in strip order, a decoded size above 1 MiB, a
 * Deflate strip of more bytes than its decoded size plus an eighth plus 512, which mrgingham_amd_tiff_layout_ex never hands out) --
 * that frame is zero-filled, the others are not affected.  d_strip_status (DEVICE, may be NULL; nframes*strips_pitch
 * words): per LZW or Deflate strip 0, or what stopped its lane (tiff_lzw.h, tiff_inflate.h).
 * Compression 5 first runs tiff_lzw_kernel, one lane per strip: a fixed number of lanes loops over the strips, each with
 * a table of 4096 dwords in context scratch (interleaved by lane: at most 16384 lanes x 16 KiB = 256 MiB, whatever the
 * batch), decoding into context scratch of nframes x rowbytes x height; a lane reads nothing beyond its strip's byte
 * count and writes nothing beyond its strip's rows.  Compression 8 / 32946 runs tiff_inflate_kernel on the same schedule,
 * each lane with 1280 16-bit words of decode tables in context scratch (at most 131072 lanes x 2560 bytes = 320 MiB, sized by the strips of the call); a match
 * never reaches before the first byte of its own strip.  Then tiff_finish_kernel, one wave per row: value order, predictor 2
 * undone by a prefix sum mod 2^bits, WhiteIsZero inverted, grey.  Asynchronous on `stream` (NULL = default); allocates
 * nothing beyond context scratch.  Arguments are checked like mrgingham_amd_png_reconstruct_batch's (MRGINGHAM_AMD_ERR_ARG,
 * nothing written). */
int mrgingham_amd_tiff_decode_batch(mrgingham_amd_ctx* ctx, const uint8_t* d_files, int64_t file_pitch,
                                    const mrgingham_amd_tiff_strip* d_strips, int strips_pitch, const int32_t* d_nstrips,
                                    int nframes, const mrgingham_amd_tiff_info* info, void* d_out, int64_t frame_pitch,
                                    int stride, int32_t* d_status, int32_t* d_strip_status, void* stream);

/* mrgingham_amd_tiff_decode_batch for tiled files: nframes files that also agree in tile_width and tile_length, d_records
 * what mrgingham_amd_tiff_layout_tiled wrote for them (record i = tile i).  tile_width == tile_length == 0 is
 * mrgingham_amd_tiff_decode_batch.  MRGINGHAM_AMD_ERR_ARG, nothing written: only one of the two is 0, tile_width is not a
 * multiple of 16, either is negative or above 32767.  Everything else as above: the alignment rules, the status words (-1
 * also for a frame whose record count is not across x down, or with a record whose first_row is not (i / across) x
 * tile_length or whose rows is not tile_length, or a tile decoding to more than 1 MiB), d_strip_status per TILE, failed
 * frames zero-filled, asynchronous on `stream`.  tiff_lzw_kernel / tiff_inflate_kernel decode tile i of frame f to context
 * scratch at f*raw_pitch + i * tile bytes, dense and tile-major (nframes x across x down x tile bytes, which may be well above
 * the samples of the frames where the edge tiles are mostly padding), a lane writing its own tile's bytes alone.  Then
 * tiff_finish_tiles_kernel, one wave per image row: lane l takes 16 pixels, which lie in one tile because tile_width is a
 * multiple of 16, from that tile's row in the scratch or -- compression 1 -- in the file's bytes at any byte address; the
 * prefix sum of predictor 2 is a segmented scan that restarts at every tile's left edge; columns at or beyond the width and
 * tile rows at or beyond the height are never stored. */
int mrgingham_amd_tiff_decode_batch_tiled(mrgingham_amd_ctx* ctx, const uint8_t* d_files, int64_t file_pitch,
                                          const mrgingham_amd_tiff_strip* d_records, int records_pitch,
                                          const int32_t* d_nrecords, int nframes, const mrgingham_amd_tiff_info* info,
                                          int tile_width, int tile_length, void* d_out, int64_t frame_pitch, int stride,
                                          int32_t* d_status, int32_t* d_strip_status, void* stream);

/* The constants of those kernels' schedules, for tests that place their shapes on the seams: the lanes in flight of the
 * LZW launch (strip s is decoded by lane s modulo that many; option "tiff_lzw_lanes" lowers it), the pixels of a row a
 * lane of the finish kernel takes, and the pixels of a row a wave takes per step (the prefix sum of predictor 2 is carried
 * from lane to lane inside a step and from step to step). */
void mrgingham_amd_tiff_geometry(int* lzw_lanes, int* segment_pixels, int* step_pixels);
/* the lanes in flight of the Deflate launch, scheduled like the LZW one (option "tiff_deflate_lanes" lowers it) */
int mrgingham_amd_tiff_inflate_lanes(void);

/* nfiles TIFF files of ONE size and depth straight into device frames (layout and element type as d_out above): per file
 * a host thread (nthreads of them; <= 0: all cores, at most 32) reads the file straight into page-locked staging and runs
 * mrgingham_amd_tiff_layout -- no sample is touched on the host --; a chunk of files goes up in three copies (the files, their strip tables packed
 * to the chunk's largest strip count, their strip counts) and through one
 * mrgingham_amd_tiff_decode_batch per run of files of equal (samples, photometric, compression, predictor, byte order)
 * while the host threads read the next.  A file the device route does not take (MRGINGHAM_AMD_TIFF_NOT_TAKEN, or a file
 * much larger than its samples) is decoded by the host thread with mrgingham_amd_read_image's decoder and uploaded: same
 * bytes.  Deflate files are among those unless option "tiff_deflate" is 1: then the layouts come from
 * mrgingham_amd_tiff_layout_ex with option "tiff_deflate_max_strip", and a file with a larger strip keeps the host thread.
 * Tiled files: the directories are parsed by mrgingham_amd_tiff_layout_tiled, and strip and tiled files of one size may
 * share a call and a chunk (runs are also split by tile width and length; they go through
 * mrgingham_amd_tiff_decode_batch_tiled).  A slot keeps `height` records per file: a tiled file with MORE TILES THAN ROWS
 * keeps the host thread, and so does one the route does not take -- a tile width that is not a multiple of 16, PackBits, a
 * tile that decodes to more than "tiff_lzw_max_strip" / "tiff_deflate_max_strip" bytes, Deflate without "tiff_deflate",
 * tiles that are mostly padding (all of them decoded take more than 16 x the frame's grey bytes + 1 MiB) --
 * both through mrgingham_amd_read_image's decoder: same bytes.  h_status[f]: 0 decoded, -1 unreadable / unsupported / malformed (or not a TIFF), -2 a TIFF of another size or
 * depth; the frame of a failed file is zero-filled.  SYNCHRONOUS: d_out is complete on return.  Returns MRGINGHAM_AMD_OK
 * also when files failed.  Completes the find_boards jobs in flight first and restores the caller's HIP device.  The
 * chunk buffers are those of mrgingham_amd_read_jpegs_batch, within the same 1 GiB (option "tiff_chunk_frames"). */
int mrgingham_amd_read_tiffs_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height,
                                   int bits, void* d_out, int64_t frame_pitch, int stride, int nthreads,
                                   int32_t* h_status);

/* The same preprocessing for one HOST image (out: dense width x height bytes, host): what the Python
 * recipe of find_board.docstring:8-10 does with cv2 before find_board.  Uses the calling thread's
 * context.  Returns 0, or -2 on an argument or device error. */
int mrgingham_amd_preprocess_image(const uint8_t* image, int width, int height, int stride, int do_clahe,
                                   int blur_radius, uint8_t* out);

/* The 16-bit branch of the tool's preprocessing for one HOST image (mrgingham-from-image.cc:85-111; `stride`
 * in elements): out receives width*height bytes.  Returns 0, or -2. */
int mrgingham_amd_preprocess_image16(const uint16_t* image, int width, int height, int stride, int do_clahe,
                                     int blur_radius, uint8_t* out);

/* What one worker of the reference CLI does with one decoded 8-bit image
 * (mrgingham-from-image.cc:71-111, :160-171): [normalize + CLAHE(8)] -> box blur of
 * blur_radius -> find_chessboard_from_image_array(gridn, image_pyramid_level), with the
 * per-corner refinement when do_refine.  Host image in, gridn*gridn corners (xy_out,
 * interleaved doubles) and their refinement levels (levels_out, may be NULL) out.  Uses the
 * calling thread's context.  Returns the level the board was found at, -1 if there is
 * none, -2 on an argument or device error. */
int mrgingham_amd_process_image(const uint8_t* image, int width, int height, int stride, int do_clahe,
                                int blur_radius, int gridn, int image_pyramid_level, int do_refine,
                                double* xy_out, signed char* levels_out);

/* The same with the tool's whole option set, and for 16-bit images (mrgingham-from-image.cc:85-92:
 * cv::normalize to 0..65535 and CLAHE on 16 bits when do_clahe, then convertTo(CV_8U, 255/65535)).
 * bits = 8 or 16; `stride` in ELEMENTS.  debug != 0 writes the reference's dumps: the preprocessed
 * image as /tmp/<basename of filename>_preprocessed.png (:113-148) and, per detector / refinement pass,
 * the level image, the normalised ChESS responses and a self-plotting corner vnlog
 * (find_chessboard_corners.cc:282-315, :453-459, :513-541) -- same names, same messages on stderr. */
typedef struct mrgingham_amd_cli_options {
    int do_clahe, blur_radius, gridn, image_pyramid_level, do_refine, do_blobs, debug;
    int debug_sequence_x, debug_sequence_y; /* both >= 0: the grid finder's sequence trace on stderr (--debug-sequence) */
    const char* filename;                   /* names the debug dumps only; may be NULL */
} mrgingham_amd_cli_options;
int mrgingham_amd_process_image_ex(const void* image, int bits, int width, int height, int stride,
                                   const mrgingham_amd_cli_options* options, double* xy_out,
                                   signed char* levels_out);

/* Batch form of the full detector (what find_chessboard_from_image_array_C does per frame, for
 * image_pyramid_level < 0 the reference's default "first level of 3,2,1,0 at which the grid finder
 * succeeds", mrgingham.cc:116-139): the GPU detects candidates for the whole batch (levels 3, 2 and 1 in one pass; what
 * is still open after them level by level), up to `nthreads` host threads (<= 0: all cores, at most 32) run the grid
 * finder on the frames that have no board yet, and the boards found are refined to level 0 on the GPU.  Synchronous.
 * h_boards (HOST): nframes x gridn*gridn x 2 doubles, board order; h_found_level[f] (HOST): the
 * level frame f's grid was found at, or -1 (then its h_boards block is left untouched). */
int mrgingham_amd_find_boards_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* frames, int gridn,
                                    int image_pyramid_level, double* h_boards, signed char* h_found_level,
                                    int nthreads);

/* The same in two halves, so that consecutive batches overlap: _submit queues the device passes of a batch (level
 * images, candidates of levels 3, 2 and 1 -- or of the one level asked for) and returns a ticket (>= 0; < 0: an error code)
 * without waiting for them; _collect(ticket) returns when h_boards / h_found_level of that batch are complete (status as
 * mrgingham_amd_find_boards_batch, which is _submit + _collect).  Between the two, the library runs the host part of
 * a batch -- the grid finder on the candidates, level 3 first, then 2, then 1 (mrgingham.cc:127-138) -- inside the NEXT
 * _submit, after that call has queued its own device passes, and queues the refinement of the boards it found
 * (mrgingham.cc:81-99; with option "sparse_refine": the response only around the corners) on a stream of its own.  So
 *     t0 = submit(batch 0); t1 = submit(batch 1); loop: t(n+2) = submit(batch n+2); collect(t(n)); ...
 * keeps the device, the host threads and the refinement busy at the same time (64 frames of 4096x3072 on one
 * MI355X: see DESIGN.md 4.5).  Frames that show no board at levels 3, 2 and 1 are finished at level 0 inside
 * _collect.  Results do not depend on how calls are interleaved: they are the synchronous dense schedule's (option
 * "find_boards_pipeline" 0), double for double.
 * The frames, h_boards and h_found_level of a batch must stay valid and untouched until its _collect returns.  As many
 * batches as the context has scratch sets (2 or 3, option "scratch_sets") can be in flight; a further _submit completes
 * the oldest one first (its _collect then returns at once).  One thread per context, as for every other call.  Any
 * other batch call or mrgingham_amd_set_option on the same context completes the batches in flight first (they stay
 * collectable), so mixing calls is safe but gives the overlap away; mrgingham_amd_destroy abandons what is in flight. */
int mrgingham_amd_find_boards_submit(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* frames, int gridn,
                                     int image_pyramid_level, double* h_boards, signed char* h_found_level,
                                     int nthreads);
int mrgingham_amd_find_boards_collect(mrgingham_amd_ctx* ctx, int ticket);
/* mrgingham_amd_find_boards_submit with the two things the one-image wrappers have on top of it (_submit is
 * _submit_ex(.., do_refine 1, .., h_levels NULL, ..)); _collect is the same.  do_refine 0: the boards stay as the grid
 * finder made them (mrgingham-from-image --no-refine).  h_levels (HOST, may be NULL): nframes x gridn*gridn signed chars,
 * the pyramid level every corner of a found board ended at -- what the reference's refinement_level array holds
 * (mrgingham.cc:81-99); with do_refine 0 every entry is the found level; the block of a frame without a board is left
 * untouched.  It must stay valid until the job's _collect returns, like h_boards. */
int mrgingham_amd_find_boards_submit_ex(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* frames, int gridn,
                                        int image_pyramid_level, int do_refine, double* h_boards, signed char* h_levels,
                                        signed char* h_found_level, int nthreads);

/* ---- a list of image files to boards ---------------------------------------------------------------------------
 * What mrgingham_amd_read_image would produce for a file, from its header alone (host only, no device needed, nothing
 * is decoded): *width, *height, *bits (8 or 16), *kind (MRGINGHAM_AMD_KIND_*, below: 1 binary PGM, 2 PNG, 3 baseline
 * JPEG: the header parse of mrgingham_amd_jpeg_coefficients, up to and including SOS; 4 TIFF:
 * mrgingham_amd_tiff_layout's parse of the directory and the strip table; 5 BMP: mrgingham_amd_bmp_layout's parse of the headers and the palette, from the file's first
 * 4096 bytes and its size -- an RLE8 file is read whole and its stream walked; 6 binary PBM or PAM:
 * mrgingham_amd_pnm_header's parse, bits 8 for P4).  Any output pointer may be NULL.  Returns 0; -1 for what
 * read_image calls unreadable at header level: a missing or empty file, another format, a header that is cut short or
 * breaks a rule (sides above 32767, interlaced PNG, progressive JPEG, ...), a PGM shorter than its header promises.  A
 * file that passes may still fail to decode.  Never sizes anything from an unchecked field. */
int mrgingham_amd_probe_image(const char* filename, int* width, int* height, int* bits, int* kind);
#define MRGINGHAM_AMD_KIND_PGM 1
#define MRGINGHAM_AMD_KIND_PNG 2
#define MRGINGHAM_AMD_KIND_JPEG 3
#define MRGINGHAM_AMD_KIND_TIFF 4
#define MRGINGHAM_AMD_KIND_BMP 5
#define MRGINGHAM_AMD_KIND_PNM 6

/* How mrgingham_amd_find_boards_files cuts a list into chunks, as a function (host only): key[i] >= 0 -- files of equal
 * key can share a chunk; key[i] < 0 -- the file is not batched (chunk_of_file[i] = slot_in_chunk[i] = -1).  Chunks are
 * created in this order: the next chunk belongs to the key of the lowest-index file not yet placed and takes that key's
 * next batch_frames files in list order.  So files keep their order inside a key, and every chunk holds the first batched
 * file the chunks before it left out: with chunks completed in order, the files known to be final form a prefix of the
 * list that grows with every chunk and never shrinks.  Returns 0, or MRGINGHAM_AMD_ERR_ARG (nfiles < 0, batch_frames < 1,
 * a NULL pointer) with nothing written. */
int mrgingham_amd_files_plan(const int32_t* key, int nfiles, int batch_frames, int32_t* chunk_of_file,
                             int32_t* slot_in_chunk, int32_t* nchunks);

/* A list of image files to boards: per file exactly what mrgingham_amd_read_image's decoder followed by
 * mrgingham_amd_process_image_ex(.., the same options, do_blobs 0, debug 0) gives -- status, found level, the boards
 * double for double, the corners' levels -- whatever batch_frames, nthreads, jpeg_entropy or the file's place in the list.
 * SYNCHRONOUS.  The call creates two contexts on ONE device and destroys them: a loader thread fills a ring of three
 * chunks of device frames on the first, the calling thread runs mrgingham_amd_preprocess_batch (not when do_clahe and
 * blur_radius are 0) and mrgingham_amd_find_boards_submit_ex per chunk on the second, keeps as many chunks in flight as
 * that context has scratch sets and collects them in chunk order.  The two are ordered by events and by what has been
 * collected; nothing synchronises the device in the steady state.  Restores the caller's current HIP device.
 * Routing by mrgingham_amd_probe_image: 8-bit files of one size share chunks (mrgingham_amd_files_plan, key = size) --
 * JPEG files through mrgingham_amd_read_jpegs_batch straight into the chunk's frames, PGM / PNG / TIFF files decoded by the
 * loader's host threads into page-locked staging and uploaded; 16-bit files (unless mrgingham_amd_find_boards_files_ex is
 * given MRGINGHAM_AMD_FILES_DEEP_CHUNKS), and sizes the batch entry points refuse
 * while the one-image path takes them (CLAHE below 8 x 8 pixels), go one at a time through the one-image path on the
 * CALLING THREAD's context (mrgingham_amd_thread_device), when the prefix of final files reaches them.  A file the
 * probe rejects, or accepts and the decoder then rejects, has status -1.
 * Memory: the ring is 3 x (raw + preprocessed) device buffers of batch_frames frames of the largest batched size;
 * batch_frames is lowered until one buffer stays within 1 GiB (12 MP: 85 frames), so the ring stays within 6 GiB; the
 * page-locked staging (lists with PGM / PNG files only) within 3 GiB.
 * Outputs (HOST, nfiles entries each, all required): h_status 0 processed / -1 unreadable; h_found_level the level, or
 * -1; h_boards (gridn*gridn*2 doubles per file) and h_levels (gridn*gridn signed chars per file) are written only where
 * a board was found.  progress (may be NULL) is called from the calling thread with non-decreasing values: files
 * [0, nfinal) are final and will not be written again; the last call passes nfiles.  stats (may be NULL): up to nstats
 * of the MRGINGHAM_AMD_FILES_STATS doubles below.  Returns MRGINGHAM_AMD_OK (also when files were unreadable; nfiles 0 is
 * fine), MRGINGHAM_AMD_ERR_ARG with nothing written (NULL pointers, gridn outside 2..1024, level above 10, blur radius outside
 * 0..64, no such device), or the device error that stopped the pipeline (every wait in it ends when the other side
 * fails); the outputs of files beyond the last progress value are then undefined. */
typedef struct mrgingham_amd_files_options {
    int do_clahe, blur_radius, gridn, image_pyramid_level, do_refine;
    int batch_frames; /* frames per chunk; <= 0: 64 */
    int nthreads;     /* host threads of the loader and of the grid finder, each (<= 0: all cores, at most 32) */
    int jpeg_entropy; /* 0: the loader's host threads Huffman-decode; 1: options "jpeg_entropy" 1 and "jpeg_sync" 1 on the loader context */
    int device;       /* -1: the device of the calling thread's context (mrgingham_amd_thread_device) */
} mrgingham_amd_files_options;
#define MRGINGHAM_AMD_FILES_CHUNKS 0           /* chunks that went through the ring */
#define MRGINGHAM_AMD_FILES_DEVICE_LOADED 1    /* files through mrgingham_amd_read_jpegs_batch (readable JPEG) or, if asked for, _read_pngs_batch (PNG_DEVICE) / _read_pgms_batch (DEEP_CHUNKS: 16-bit PGM) / _read_tiffs_batch (TIFF_DEVICE) / _read_bmps_batch (BMP_DEVICE) / _read_pnms_batch (PNM_DEVICE) */
#define MRGINGHAM_AMD_FILES_HOST_DECODED 2     /* files decoded on host threads into a chunk (8-bit PGM / PNG / TIFF / PBM / PAM, BMP; 16-bit PNG / TIFF / PAM with DEEP_CHUNKS alone) */
#define MRGINGHAM_AMD_FILES_ONE_IMAGE 3        /* files through the one-image path */
#define MRGINGHAM_AMD_FILES_UNREADABLE 4       /* files with status -1 ([1] + [2] + [3] + [4] = nfiles) */
#define MRGINGHAM_AMD_FILES_DETECTOR_WAIT_MS 5 /* wall ms the calling thread waited for a loaded chunk: the loader bounds the run */
#define MRGINGHAM_AMD_FILES_LOADER_WAIT_MS 6   /* wall ms the loader thread waited for a free ring slot: the detector bounds it */
#define MRGINGHAM_AMD_FILES_STATS 7
int mrgingham_amd_find_boards_files(const char* const* filenames, int nfiles, const mrgingham_amd_files_options* options,
                                    double* h_boards, signed char* h_levels, signed char* h_found_level, int32_t* h_status,
                                    void (*progress)(int nfinal, void* cookie), void* cookie, double* stats, int nstats);

/* mrgingham_amd_find_boards_files with loader flags (0: exactly that call).  MRGINGHAM_AMD_FILES_PNG_DEVICE: runs of
 * consecutive 8-bit PNG slots of a chunk go through mrgingham_amd_read_pngs_batch on the loader context, like the JPEG
 * runs -- the host threads only inflate -- and are counted under MRGINGHAM_AMD_FILES_DEVICE_LOADED; palette files keep
 * the host decoder (and MRGINGHAM_AMD_FILES_HOST_DECODED), 16-bit files the one-image path.  Same outputs.
 * MRGINGHAM_AMD_FILES_DEEP_CHUNKS: 16-bit PGM and PNG files of one size share chunks of their own (key = size and depth: a
 * chunk holds one size AND one depth; CLAHE below 8 x 8 pixels keeps the one-image path) instead of going one at a time
 * through the calling thread.  PGM slots go through mrgingham_amd_read_pgms_batch (MRGINGHAM_AMD_FILES_DEVICE_LOADED); PNG
 * slots through mrgingham_amd_read_pngs_batch if PNG_DEVICE is set as well (DEVICE_LOADED), else through the host decoder
 * on the loader's host threads and an upload of native uint16 samples (HOST_DECODED).  The calling thread runs
 * mrgingham_amd_preprocess16_batch on every such chunk (always: it is what makes the 8-bit frames), then
 * mrgingham_amd_find_boards_submit_ex.  The ring buffers are sized in BYTES of the largest batched frame: a 16-bit chunk
 * holds half the frames of an 8-bit one under the same 1 GiB.  Same outputs.  The flags may be combined; any other bit
 * is MRGINGHAM_AMD_ERR_ARG. */
#define MRGINGHAM_AMD_FILES_PNG_DEVICE 1
#define MRGINGHAM_AMD_FILES_DEEP_CHUNKS 2
int mrgingham_amd_find_boards_files_ex(const char* const* filenames, int nfiles, const mrgingham_amd_files_options* options,
                                       double* h_boards, signed char* h_levels, signed char* h_found_level,
                                       int32_t* h_status, void (*progress)(int nfinal, void* cookie), void* cookie,
                                       double* stats, int nstats, int loader_flags);

/* mrgingham_amd_find_boards_files_ex with one more loader flag (the older entry point goes on refusing it).  Without it
 * TIFF files behave as PGM and PNG files do: 8-bit files of one size share chunks and are decoded by the loader's host
 * threads (MRGINGHAM_AMD_FILES_HOST_DECODED), 16-bit files take the one-image path or, with DEEP_CHUNKS, chunks of their own.
 * MRGINGHAM_AMD_FILES_TIFF_DEVICE: runs of consecutive TIFF slots of a chunk (8-bit; 16-bit under DEEP_CHUNKS) go through
 * mrgingham_amd_read_tiffs_batch on the loader context and are counted under MRGINGHAM_AMD_FILES_DEVICE_LOADED.  Same
 * outputs.  Any bit above the three flags is MRGINGHAM_AMD_ERR_ARG. */
#define MRGINGHAM_AMD_FILES_TIFF_DEVICE 4
int mrgingham_amd_find_boards_files_ex2(const char* const* filenames, int nfiles, const mrgingham_amd_files_options* options,
                                        double* h_boards, signed char* h_levels, signed char* h_found_level,
                                        int32_t* h_status, void (*progress)(int nfinal, void* cookie), void* cookie,
                                        double* stats, int nstats, int loader_flags);

/* mrgingham_amd_find_boards_files_ex2 with one more loader flag (which _ex2 goes on refusing).
 * MRGINGHAM_AMD_FILES_TIFF_DEFLATE_DEVICE: the TIFF runs also send their Deflate files through the device (option
 * "tiff_deflate" of the loader context).  It is part of the TIFF device route: without MRGINGHAM_AMD_FILES_TIFF_DEVICE it is
 * MRGINGHAM_AMD_ERR_ARG, as is any bit above the four flags.  Same outputs. */
#define MRGINGHAM_AMD_FILES_TIFF_DEFLATE_DEVICE 8
int mrgingham_amd_find_boards_files_ex3(const char* const* filenames, int nfiles, const mrgingham_amd_files_options* options,
                                        double* h_boards, signed char* h_levels, signed char* h_found_level,
                                        int32_t* h_status, void (*progress)(int nfinal, void* cookie), void* cookie,
                                        double* stats, int nstats, int loader_flags);

/* mrgingham_amd_find_boards_files_ex3 with one more loader flag (which _ex3 goes on refusing).  Without it BMP files behave
 * as 8-bit PGM files do: files of one size share chunks and are decoded by the loader's host threads
 * (MRGINGHAM_AMD_FILES_HOST_DECODED).  MRGINGHAM_AMD_FILES_BMP_DEVICE: runs of consecutive BMP slots of a chunk go through
 * mrgingham_amd_read_bmps_batch on the loader context and are counted under MRGINGHAM_AMD_FILES_DEVICE_LOADED.  Same
 * outputs.  Any bit above the five flags is MRGINGHAM_AMD_ERR_ARG. */
#define MRGINGHAM_AMD_FILES_BMP_DEVICE 16
int mrgingham_amd_find_boards_files_ex4(const char* const* filenames, int nfiles, const mrgingham_amd_files_options* options,
                                        double* h_boards, signed char* h_levels, signed char* h_found_level,
                                        int32_t* h_status, void (*progress)(int nfinal, void* cookie), void* cookie,
                                        double* stats, int nstats, int loader_flags);

/* mrgingham_amd_find_boards_files_ex4 with one more loader flag (which _ex4 goes on refusing).  Without it P4 and P7
 * files (MRGINGHAM_AMD_KIND_PNM) behave as PGM files do: 8-bit files of one size share chunks and are decoded by the loader's host threads
 * (MRGINGHAM_AMD_FILES_HOST_DECODED); 16-bit ones take the one-image path, or with MRGINGHAM_AMD_FILES_DEEP_CHUNKS the
 * 16-bit chunks.  MRGINGHAM_AMD_FILES_PNM_DEVICE: runs of consecutive MRGINGHAM_AMD_KIND_PNM slots of a chunk go through
 * mrgingham_amd_read_pnms_batch on the loader context and are counted under MRGINGHAM_AMD_FILES_DEVICE_LOADED.  P5 files keep
 * their routes and counters under every flag.  Same outputs.  Any bit above the six flags is MRGINGHAM_AMD_ERR_ARG. */
#define MRGINGHAM_AMD_FILES_PNM_DEVICE 32
int mrgingham_amd_find_boards_files_ex5(const char* const* filenames, int nfiles, const mrgingham_amd_files_options* options,
                                        double* h_boards, signed char* h_levels, signed char* h_found_level,
                                        int32_t* h_status, void (*progress)(int nfinal, void* cookie), void* cookie,
                                        double* stats, int nstats, int loader_flags);

/* Where the find_boards calls of this context spent their HOST time since the last reset, and what their grid-finder
 * threads did (the reference's find_grid_from_points, mrgingham.cc:51, is the host part of the product call; on a busy
 * batch it is what bounds it).  out[0 .. n) receives up to MRGINGHAM_AMD_FB_STATS doubles:
 *   [0] batches submitted   [1] host threads of the most recent batch (grid-finder workers + the calling thread)
 *   host milliseconds, totals over the batches:
 *   [2] submit: checks + scratch   [3] submit: the previous batch's host part begun (waits for its first device pass)
 *   [4] submit: this batch's device passes queued   [5] host part: grid finder joined (wall time the caller waits)
 *   [6] host part: refinement queued   [7] collect: wait for the refinement   [8] collect: boards copied
 *   grid finder, summed over the threads:
 *   [9] calls   [10] calls that found a grid   microseconds in [11] neighbour graph (sort, Delaunay, site rings)
 *   [12] adjacency lists   [13] sequence-candidate search   [14] outer edges, 4-cycles, rows
 *   device milliseconds (hipEvents), totals over the batches:
 *   [15] first pass: from its first kernel on the pixel stream to the candidates on the host (runs behind the pass of the
 *        batch before it, so in a full pipeline this is the pass's own time)   [16] refinement: boards up, levels, boards down
 * Completes the batches in flight first (they stay collectable).  Returns MRGINGHAM_AMD_FB_STATS, or an error code. */
#define MRGINGHAM_AMD_FB_STATS 17
int mrgingham_amd_find_boards_stats(mrgingham_amd_ctx* ctx, double* out, int n, int reset);
/* The same clock of the CALLING thread's own mrgingham_amd_find_grid_from_points* calls (host only, no device):
 * out6 = calls, found, then the four microsecond sums. */
int mrgingham_amd_grid_clock(double* out6, int reset);

/* THE GRID FINDER ON THE DEVICE.  Candidate lists that lie in device memory -- what mrgingham_amd_detect_batch leaves:
 * d_xy = nlists blocks of `capacity` interleaved (x, y) * 1000 int pairs, d_counts[l] = candidates of list l -- to boards
 * as INDICES: d_index = nlists blocks of gridn * gridn candidate indices in board order (rows top to bottom, each left to
 * right; -1 throughout where the status is not 1), d_status[l] =
 *    1  board found          0  the host finder would find none          < 0  declined: the list is the host finder's
 *   MRGINGHAM_AMD_GRID_DECLINE_COUNT (-1)  more candidates than the device takes (mrgingham_amd_find_grids_geometry),
 *                                          or count > capacity, or count < 0
 *   MRGINGHAM_AMD_GRID_DECLINE_RING  (-2)  a degenerate neighbour structure the kernel does not resolve
 *   MRGINGHAM_AMD_GRID_DECLINE_GUARD (-3)  a floating-point decision of the sequence walk inside the guard band
 *   MRGINGHAM_AMD_GRID_DECLINE_TABLE (-4)  a table or a loop bound of the kernel was exceeded
 *   MRGINGHAM_AMD_GRID_DECLINE_COORD (-5)  a coordinate with |x| or |y| >= 2^24
 * The corners of a board are xy[index] / 1000.0 (find_grid.cc:353-354): the device makes decisions and no double that
 * anyone sees.  THE RULE: an answer (1 or 0, and the indices) is the one mrgingham_amd_find_grid_from_points_perturbed
 * gives with canonical_start -- every neighbour ring started at the first neighbour counter-clockwise from +x, the one
 * ring rule this finder has, under which the host finder is pinned to upstream's find_grid.cc; where the device cannot be
 * sure of that it declines, and never answers differently.  The guard band: every comparison of the walk against 0.984,
 * 0.7, 1.4 and +-0.35 (find_grid.cc:204-207) is made with a band of 2^-bits, option "find_grids_guard_bits" (8 .. 45,
 * default 33: 1.2e-10 where the host's hypot and the device's sqrt move a quotient by some 1e-16); a value inside the band
 * declines the whole list.  gridn 2 .. 16.  One workgroup of 256 lanes per list, one launch.
 * Queued like mrgingham_amd_detect_batch: on the context's streams, behind what mrgingham_amd_after_stream has named and
 * behind earlier calls of the context that touch the same buffers; mrgingham_amd_stream_wait / _sync wait for it.  Grows
 * context scratch (a slot of rings and adjacency lists per workgroup).  Completes find_boards jobs in flight first.
 * MRGINGHAM_AMD_ERR_ARG, nothing queued: a NULL pointer, gridn outside 2 .. 16, a negative nlists or capacity. */
enum {
    MRGINGHAM_AMD_GRID_DECLINE_COUNT = -1,
    MRGINGHAM_AMD_GRID_DECLINE_RING = -2,
    MRGINGHAM_AMD_GRID_DECLINE_GUARD = -3,
    MRGINGHAM_AMD_GRID_DECLINE_TABLE = -4,
    MRGINGHAM_AMD_GRID_DECLINE_COORD = -5
};
int mrgingham_amd_find_grids_batch(mrgingham_amd_ctx* ctx, const int32_t* d_xy, const int32_t* d_counts, int nlists, int capacity,
                                   int gridn, int32_t* d_index, int32_t* d_status);
/* The same text (csrc/grid_phases.h) run serially on the host, over lists in host memory: no device, no context.  It equals
 * the kernel list for list, every status and decline reason included -- both make the same IEEE operations --, and is what
 * a debugger steps through when the two disagree.  guard_bits 8 .. 45.  Returns 0 or MRGINGHAM_AMD_ERR_ARG. */
int mrgingham_amd_find_grids_host(const int32_t* xy, const int32_t* counts, int nlists, int capacity, int gridn, int guard_bits,
                                  int32_t* index, int32_t* status);
/* The caps of the kernel (each pointer may be NULL): lanes of a workgroup, candidates per list it takes, the gridn range,
 * the workgroups of a launch (more lists take turns) and the bytes of context scratch each of them uses. */
void mrgingham_amd_find_grids_geometry(int* lanes_per_workgroup, int* max_candidates, int* min_gridn, int* max_gridn,
                                       int* max_workgroups, int64_t* scratch_bytes_per_workgroup);
/* Lists the device finder of this context has answered since the last reset, in mrgingham_amd_find_grids_batch and in
 * find_boards under option "find_boards_grid": out[0 .. n) receives up to MRGINGHAM_AMD_FIND_GRIDS_STATS doubles:
 *   [0] lists   [1] found   [2] none   [3] .. [7] declined with -1 .. -5
 *   [8] lists of find_boards jobs that the host finder answered because the device had declined them
 * Synchronises; completes find_boards jobs in flight first.  Returns MRGINGHAM_AMD_FIND_GRIDS_STATS, or an error code. */
#define MRGINGHAM_AMD_FIND_GRIDS_STATS 9
int mrgingham_amd_find_grids_stats(mrgingham_amd_ctx* ctx, double* out, int n, int reset);

/* find_blobs_from_image_array (find_blobs.cc:14-46) for every frame of a device-resident batch.
 * HOST outputs (the last stage of the detector runs on the host): h_xy = nframes blocks of capacity_per_frame
 * interleaved (x,y)*1000 int pairs in SimpleBlobDetector's output order, h_counts[f] = keypoints of frame f
 * (may exceed capacity_per_frame: then only the first capacity_per_frame were stored; -1: see ERR_CAPACITY).
 * Synchronous.  Same integers as find_chessboard_corners_from_image_array_C(.., doblobs = true) per frame.
 * Frames up to 32767 x 65535; h_xy may be NULL only with capacity 0; nthreads: host threads of the per-contour filters
 * (<= 0: all cores, at most 32).  The device follows the borders of all 17 thresholds of a CHUNK of frames at once
 * (one launch of every kernel and three round trips per chunk, whatever its frame count); a batch is worked through in
 * chunks whose bit planes stay within 1 GiB of context scratch.  A frame with more than 2^27 border starts (pure noise
 * at tens of megapixels) has no result: its count is -1, the other frames are delivered, and the call returns
 * MRGINGHAM_AMD_ERR_CAPACITY.  Completes find_boards jobs in flight first; restores the caller's current HIP device. */
int mrgingham_amd_blobs_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* frames, int32_t* h_xy,
                              int capacity_per_frame, int32_t* h_counts, int nthreads);

/* find_circle_grid_from_image_array (bridge.cc:104-113) for every frame: blobs, then the host grid finder on the
 * context's host threads, no refinement.  h_boards / h_found as mrgingham_amd_find_boards_batch; h_found[f] is 0
 * or -1.  The grid finder sees ALL keypoints of a frame (no capacity). */
int mrgingham_amd_find_circle_grids_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* frames, int gridn,
                                          double* h_boards, signed char* h_found, int nthreads);

/* What the two calls above did on this context since the last reset: out[0 .. n) receives up to
 * MRGINGHAM_AMD_BLOBS_STATS doubles:
 *   [0] calls   [1] chunks   [2] nodes (border starts) followed   [3] contours downloaded   [4] contour points downloaded
 *   [5] device milliseconds of the chunks' kernels (hipEvents; counted only while mrgingham_amd_set_kernel_timing is on)
 *   [6] host milliseconds of the filters and the grouping   [7] frames
 * (the one-image blob path of the reference symbols counts too, on the calling thread's context).  Returns
 * MRGINGHAM_AMD_BLOBS_STATS, or an error code. */
#define MRGINGHAM_AMD_BLOBS_STATS 8
int mrgingham_amd_blobs_stats(mrgingham_amd_ctx* ctx, double* out, int n, int reset);

/* TEST HOOK: which implementation of the component search handled each frame of the most recent call at
 * `level`: h_paths[f] = 1 out of LDS, 0 the global-memory kernels (hot pixels that cannot be cut into bands
 * of at most 2048, more than 512 multi-pixel components per band / points, or more LIFO demand than the LDS
 * tables hold), 2 = a refinement the LDS kernel began band by band and the global-memory kernel finished.
 * Synchronises. */
int mrgingham_amd_debug_paths(mrgingham_amd_ctx* ctx, int level, int nframes, int32_t* h_paths);

/* TEST HOOK: with option "cc_lds" = 1 | 512 the LDS refinement kernel leaves a phase clock of the first frame of
 * the call: h_ticks12[0..7] = 100 MHz ticks at start, bands planned, hot list loaded + labelled, seeds found,
 * groups formed, LIFO demand known + neighbour table built, fills done (all of the first band), end;
 * [8..11] = hot pixels, points, bands, level.  Synchronises.  (tools/cc_phases.py) */
int mrgingham_amd_debug_refine_clock(mrgingham_amd_ctx* ctx, long long* h_ticks12);

/* TEST HOOK: the PIXEL STAGE of a call alone.  Queues on the pixel stream exactly what the named entry point queues
 * there under the context's current options -- level images, clamped responses, hot lists and pixel -> index maps --
 * launches NO kernel of the component search, ends the call and synchronises (returns what mrgingham_amd_sync would).
 * The products stay in the context's scratch for mrgingham_amd_debug_pixel_products until the next call that computes.
 *   MRGINGHAM_AMD_PIXELS_CHAIN     mrgingham_amd_chain_batch(frames, level = start level, points_pitch);
 *                                  mrgingham_amd_chain_info reports the launch as after that call.  Products: levels
 *                                  0 .. level -- with the sparse schedule the level images of all of them, and the
 *                                  response, list and map of the start level only (the levels below it are computed on
 *                                  the component stream);
 *   MRGINGHAM_AMD_PIXELS_LEVEL     mrgingham_amd_detect_batch(frames, level).  Products: that level;
 *   MRGINGHAM_AMD_PIXELS_RESPONSE  mrgingham_amd_cc_on_response_batch: d_response = dense int16 responses, frames->nframes
 *                                  of frames->width x frames->height (no other field of `frames` is read).  Products:
 *                                  "level" 0 without a level image.
 * d_response is NULL in the other two modes; points_pitch only sizes scratch (as in the calls themselves; >= 1 for a chain). */
#define MRGINGHAM_AMD_PIXELS_CHAIN 0
#define MRGINGHAM_AMD_PIXELS_LEVEL 1
#define MRGINGHAM_AMD_PIXELS_RESPONSE 2
int mrgingham_amd_debug_pixel_stage(mrgingham_amd_ctx* ctx, int mode, const mrgingham_amd_frames* frames, int level,
                                    int points_pitch, const int16_t* d_response);

/* TEST HOOK: what mrgingham_amd_debug_pixel_stage left for frame `frame` at `level` (w x h = mrgingham_amd_level_dims of
 * the frames; gw = (w + 7) / 8), copied to the host; a NULL pointer skips that product:
 *   h_image     w * h bytes, the level image (levels >= 1)            h_response  w * h int16, the clamped response
 *   h_hot_cnt   1: hot-list entries MADE (may exceed the capacity)    h_cap       1: the list's capacity per frame
 *   h_hot_xy    min(*h_hot_cnt, *h_cap) entries (y << 16) | x         h_gidx      gw * h pairs (first index, 8-bit mask);
 *                                                                                 pairs of groups without a hot pixel are
 *                                                                                 never written and hold anything
 * MRGINGHAM_AMD_ERR_ARG when there is no pixel stage to read (another call has computed since) or the product asked for
 * is not one of that stage's. */
int mrgingham_amd_debug_pixel_products(mrgingham_amd_ctx* ctx, int level, int frame, uint8_t* h_image, int16_t* h_response,
                                       int32_t* h_hot_cnt, int32_t* h_cap, uint32_t* h_hot_xy, uint32_t* h_gidx);

/* Device memory the context currently holds (level scratch of both sets, point scratch, staging). */
long long mrgingham_amd_scratch_bytes(const mrgingham_amd_ctx* ctx);

/* How the most recent mrgingham_amd_chain_batch call was launched (for benchmarks that price the level-0
 * kernel): *fused_pyramid = 1 when the level-0 response kernel also wrote the level images 1..3 (frames of
 * whole 16 x 8 blocks, option "fuse_pyramid"), 0 when a separate pyramid kernel did; *merged_levels = number
 * of levels whose responses shared one launch (0 = one launch per level; -1 = the call ran with option
 * "sparse_refine", where the timed launch is the one that writes the level images).  Either pointer may be NULL. */
int mrgingham_amd_chain_info(const mrgingham_amd_ctx* ctx, int* fused_pyramid, int* merged_levels);

/* Tunables outside the reference's surface.  Known names:
 *   "fuse_pyramid"        1 (default): chain calls on frames of whole 16 x 8 blocks take the level images
 *                         1..3 out of the level-0 response kernel; 0: separate pyramid kernel
 *   "scratch_sets"        how many calls' component searches may be in flight while the pixel kernels of the next call
 *                         run (each set is a full copy of the level scratch): 0 (default) = chosen per batch shape --
 *                         three while three sets stay below 8 GB (small frames, whose search chain is longer than two
 *                         steps of the pixel kernels; 16 GB once option "sparse_refine" has been on), two otherwise --,
 *                         2 or 3 = fixed.  Synchronises.
 *   "hot_capacity_shift"  per-frame capacity of the hot-pixel / component tables of a pyramid level is
 *                         (level width * height) >> shift entries, at least 4096 (default 7: 0.35 bytes of tables per
 *                         pixel; 0 = one entry per pixel).  Derived limits at shift > 0: candidates per frame
 *                         capacity / 16 + 1024, LIFO words 1.25 * capacity + 16384.  A frame that exceeds one of
 *                         them makes the call fail with MRGINGHAM_AMD_ERR_CAPACITY at the next mrgingham_amd_sync --
 *                         nothing is written for that frame (detect: count -1; refine: its points keep their values
 *                         and levels, except on a LIFO overflow in the middle of a frame, where the points refined so
 *                         far stay refined) -- and the tables of that level GROW to what the frame asked for, so
 *                         the same call succeeds when it is made again (refinement is idempotent: points already at
 *                         the level are skipped).  Setting the option resets what has grown
 *                         ("hot_capacity_shift_temporary": the same without that reset -- for a caller's own last-resort
 *                         retry at shift 0 and the way back).
 *   "multi_level_launch"  chain_batch: 0 = one ChESS launch per pyramid level, 1 (default) = levels 3..1 in one
 *                         launch, 2 = all levels in one launch
 *   "cc_lds"              1 (default) = component search out of LDS: frames with at most 2048 hot pixels in one
 *                         pass, frames with up to 16384 in bands of rows separated by three rows without a hot
 *                         pixel, refinement of frames with more than that on the hot pixels in the cells around
 *                         the points (the global-memory kernels take what is left), 0 = global-memory kernels only;
 *                         1 | 256 = neither bands nor cells (test hook; results are the same).  Any other value is
 *                         refused.
 *   "sparse_subsets"      1 .. 4 (default 2): workgroups per frame of the refinement kernel of a sparse level.  A frame with
 *                         at least 128 points to refine at a level (a 14x14 board) is cut into that many subsets of points
 *                         that are at least 64 pixels apart, refined side by side (64 x 4096x3072, 14x14: 0.55 -> 0.46 ms per
 *                         sparse step; a 10x10 board stays with one workgroup, which is faster there).  Results do not depend on it.
 *   "sparse_refine"       1 (default), 0, 2: chain_batch computes the response of the levels BELOW the start level only in
 *                         the 16 x 16 cells around the points it refines there (all level images and the start level's
 *                         response stay whole-frame): 2 = always, 1 = for calls of at least 96 Mi frame pixels (smaller
 *                         calls are faster dense), 0 = never (the dense per-level response of the reference, what bench.py's
 *                         `value` is measured with).  Same outputs on every frame: a frame the sparse kernels cannot take
 *                         -- a component that leaves the cells around its point, more than 512 points -- is repeated densely
 *                         by the library, on the device, inside the same call (mrgingham_amd_sparse_fallbacks counts them).
 *   "blob_chunk_frames"   test hook: 0 (default) = mrgingham_amd_blobs_batch / _find_circle_grids_batch cut a batch into chunks
 *                         by their scratch budget; n > 0 = at most n frames per chunk.  Results never depend on it.
 *   "jpeg_chunk_frames"   test hook: 0 (default) = mrgingham_amd_read_jpegs_batch cuts its files into chunks by its scratch
 *                         budget; n > 0 = at most n files per chunk.  Results never depend on it.
 *   "png_chunk_frames"    test hook: the same for mrgingham_amd_read_pngs_batch.
 *   "pgm_chunk_frames"    test hook: the same for mrgingham_amd_read_pgms_batch.
 *   "tiff_chunk_frames"   test hook: the same for mrgingham_amd_read_tiffs_batch.
 *   "bmp_chunk_frames"    test hook: the same for mrgingham_amd_read_bmps_batch.
 *   "bmp_unpack"          1 (default): mrgingham_amd_read_bmps_batch sends the files' pixel arrays through
 *                         mrgingham_amd_bmp_unpack_batch; 0: its host threads decode every file (the leg to compare
 *                         against).  Same frames and statuses.
 *   "pnm_chunk_frames"    test hook: the same for mrgingham_amd_read_pnms_batch.
 *   "pnm_unpack"          1 (default): mrgingham_amd_read_pnms_batch sends the files' rasters through
 *                         mrgingham_amd_pnm_unpack_batch; 0: its host threads decode every file with
 *                         mrgingham_amd_read_image (the leg to compare against).  Same frames and statuses.
 *   "tiff_lzw_max_strip"  decoded bytes of an LZW strip, 1 .. 1048576 (the limit of the kernel's table entries; default
 *                         65536): a file with a larger strip keeps the host threads in mrgingham_amd_read_tiffs_batch.  It
 *                         bounds the serial work of one lane: on 64 12 MP files mrgingham_amd_read_tiffs_batch was measured
 *                         faster through the device than on 16 host threads at 8 KiB and 64 KiB strips and slower at 1 MiB
 *                         (the sizes between were not measured).
 *   "tiff_deflate"        0 (default): mrgingham_amd_read_tiffs_batch leaves Deflate files to its host threads; 1: it sends
 *                         them through the device (mrgingham_amd_tiff_layout_ex), a strip per lane.
 *   "tiff_deflate_max_strip" decoded bytes of a Deflate strip, 0 .. 1048576 (default 8192): with "tiff_deflate" 1, a file
 *                         with a larger strip keeps the host threads.  Together with the limit on a strip's bytes in the
 *                         file (mrgingham_amd_tiff_layout_ex) it bounds the serial work of one lane: on 64 12 MP
 *                         files mrgingham_amd_read_tiffs_batch was measured against 16 host threads at 8 KiB, 64 KiB and
 *                         1 MiB per strip and won at 8 KiB only.
 *   "tiff_deflate_lanes"  test hook: lanes in flight of the Deflate launch, a multiple of 64 up to 131072; 0 (default) = 131072.
 *   "tiff_lzw_lanes"      test hook: lanes in flight of the LZW launch, a multiple of 64 up to 16384; 0 (default) = 16384.
 *                         Results never depend on it.
 *   "jpeg_entropy"        0 (default): mrgingham_amd_read_jpegs_batch entropy-decodes on its host threads; 1: files with
 *                         restart intervals are Huffman-decoded on the device, one lane per interval.  Same frames and statuses.
 *   "jpeg_entropy_max_interval"  MCUs per restart interval the device accepts (default 1024, at least 1; files above it go
 *                         to the host threads / get status -3).  A condition, not a tuning result: it bounds the serial
 *                         work of one lane, so a 12 MP file of a single interval is never handed to one lane.
 *   "jpeg_entropy_memset" how the device decoder fills the blocks (same coefficients): 0 (default) = every lane writes its
 *                         blocks in full, zeros included; 1 = the area is zeroed in front and lanes store non-zero values
 *   "jpeg_sync"           0 (default): files without restart intervals keep the host decoder (status -3 from
 *                         mrgingham_amd_jpeg_entropy_batch); 1: they are Huffman-decoded on the device by subsequences that
 *                         synchronise themselves (mrgingham_amd_jpeg_sync_rounds).  The loader looks at it only under
 *                         "jpeg_entropy" 1.  Same coefficients, frames and statuses.
 *   "jpeg_sync_subsequence"  raw bytes of entropy-coded data per lane: a multiple of 4 in 8..1024 (default 128, the size with the best
 *                         loader rate measured at 12 MP: DESIGN.md section 4.10).  Results never depend on it; the rounds a
 *                         file needs do.
 *   "jpeg_sync_max_rounds"  0..4096, the update rounds within which a file has to converge to be decoded on the device;
 *                         0 (default) = 8192 / "jpeg_sync_subsequence".  A condition, not a tuning result: it bounds the
 *                         launches queued per chunk (this many + 1) at 8 KB of synchronisation distance.
 *   "jpeg_sync_time_phase"  internal hook of tools/jpeg_huff_bench.py, not part of the interface and free to change: what
 *                         kernel timing brackets on that path: 0 (default) all its launches, 1 round 0, 2 the update
 *                         rounds, 3 the scan, 4 the write pass.  Results never depend on it.
 *   "find_boards_pipeline" 1 (default): mrgingham_amd_find_boards_batch / _submit / _collect as described there; 0: the
 *                         synchronous schedule (one level at a time for the whole batch, dense refinement) -- same results
 *   "find_boards_grid"    0 (default): the grid finder of find_boards runs on the context's host threads; 1: the pipelined
 *                         schedule orders the candidate lists of levels 3, 2 and 1 on the device, right behind their
 *                         detection (mrgingham_amd_find_grids_batch), and the host threads take, per frame and level in the
 *                         reference's order, the board from the indices (status 1), go on to the next level (0), or run
 *                         the host finder on a list the device declined.  Frames re-detected at full capacity and the
 *                         synchronous schedule ("find_boards_pipeline" 0) keep the host finder.  Under 1 EVERY host finder
 *                         call of the job starts its neighbour rings at the canonical neighbour (the first one
 *                         counter-clockwise from +x), so that one call has one ring rule: on clean candidate sets this
 *                         changes no board (tests/test_grid.py), on ambiguous ones the ring start was never pinned.
 *   "find_grids_guard_bits"  8 .. 45 (default 33): the guard band of the device grid finder is 2^-bits
 *                         (mrgingham_amd_find_grids_batch); a wider band declines more lists and changes no answer.
 *   "chess_seg", "chess16_seg"  rows per workgroup of the ChESS kernels of THIS context (chess_v1* / chess_v16; 0 = cost model,
 *                         the default): the frame is cut into ceil(height / value) row segments of equal height (whole
 *                         8- / 16-row groups); results do not depend on it
 *   "chess_variant"       the response without a hot list: 0 (default) = chess_v16_kernel where it pays, 1 = chess_v1 always,
 *                         16 = chess_v16 wherever it can run (widths that are multiples of 16); same results
 *   "preprocess_fused"    1 (default): mrgingham_amd_preprocess_batch(do_clahe, blur_radius 1) -- the reference tool's default
 *                         chain -- blends the CLAHE tile LUTs and blurs in ONE pass over the frame where the geometry allows
 *                         (rows of 16-byte multiples, tiles at least 34 rows high); 0: always two kernels.  Same bytes.
 *                         Also mrgingham_amd_preprocess16_batch (and the 16-bit images of _preprocess_image16 /
 *                         _process_image_ex): 1 = three passes over the pixels (extrema, raw-value tile histograms,
 *                         blend + blur), 0 = the one-image kernels (normalised 16-bit copy, 65 536-bin tables per tile,
 *                         then the box blur as its own kernel).  Same bytes.
 *   "scratch_fill"        test hook: -1 (default) = off; 0..255: every new allocation of context memory (device and page-locked)
 *                         is filled with that byte before it is used.  A context starts with the value of the environment
 *                         variable MRGINGHAM_AMD_SCRATCH_FILL (decimal or 0x..; unset, empty or no byte: off) -- the way to
 *                         reach the contexts behind the reference's own names and inside mrgingham_amd_find_boards_files.
 *                         Results never depend on it: no call reads scratch it has not written.
 *   "scratch_fill_now"    test hook, a one-shot: completes what is in flight, then fills every scratch buffer the context
 *                         owns with the byte given (0..255) -- not the few words that are state between calls (status
 *                         and hot-count words, the sparse-fallback counter, the clock probe's sums, the grid finder's counters).  Results never depend on it.
 * Builds made with -DMRG_EXPERIMENT (make -C mrgingham_amd/csrc EXPERIMENT=1 -> libmrgingham_amd_experiment.so)
 * additionally accept the timing ablations and phase clocks of tools/ ("cc_lds" bits 2, 4, 8, 16, 128, 512,
 * "cc_schedule", "chess_stage", "chess_multi_min_blocks", "chess_v0" = the reference-shaped ChESS kernel as an on-device
 * cross-check, the MRGINGHAM_AMD_PYR_SKIP / _CC_LDS_PAD / _CC_CUS /
 * _PIX_COMPLEMENT / _CHESS_V0 environment variables): some of them produce wrong results on purpose, which is why the
 * shipped library has none of them and reads no environment variable except MRGINGHAM_AMD_DEVICE and the test hook
 * MRGINGHAM_AMD_SCRATCH_FILL, which changes no result. */
int mrgingham_amd_set_option(mrgingham_amd_ctx* ctx, const char* name, int value);

/* Wait for everything queued on the context's streams; returns the first
 * asynchronous error.  MRGINGHAM_AMD_ERR_CAPACITY here means a frame had more
 * hot pixels (or candidates) than the component tables of its level hold (dense
 * texture): the tables have grown by the time this returns, make the same call
 * again (see "hot_capacity_shift").  The reference-symbol wrappers in section (1)
 * and mrgingham_amd_find_boards_batch do that themselves. */
int mrgingham_amd_sync(mrgingham_amd_ctx* ctx);

/* Device-side alternative to mrgingham_amd_sync for pipelines: makes `stream` (a hipStream_t,
 * NULL = the default stream) wait for EVERY detect / refine / chain call queued so far and not yet
 * waited for by mrgingham_amd_sync -- consecutive calls finish on different component streams, so the
 * wait is for each scratch set with a call in flight, not for the last call alone -- without
 * blocking the host.  Consecutive calls overlap (the pixel kernels of call N+1 run while
 * the component kernels of call N finish, on alternating scratch sets), so give each call in
 * flight its own output buffers. */
int mrgingham_amd_stream_wait(mrgingham_amd_ctx* ctx, void* stream);

/* The other direction: the NEXT detect / refine / chain call queued on the context starts only after
 * everything queued so far on `stream` (e.g. the host-to-device copy of its frames on a copy stream)
 * has completed.  Does not block the host. */
int mrgingham_amd_after_stream(mrgingham_amd_ctx* ctx, void* stream);

/* Average duration in milliseconds of the dominant kernel (the level-0 ChESS
 * response kernel) over the launches issued since the last call, measured with
 * hipEvents on the streams the kernel ran on; the number of launches is stored
 * in *nlaunches.  Timing is off by default: enable with
 * mrgingham_amd_set_kernel_timing(ctx, 1); 2 = only the engine-clock probe below (no events on the streams), 0 = off.
 * While timing is on, the Huffman launches of mrgingham_amd_jpeg_entropy_batch / of the loader under "jpeg_entropy" are
 * bracketed and counted the same way (one pair per chunk; tools/jpeg_huff_bench.py). */
void mrgingham_amd_set_kernel_timing(mrgingham_amd_ctx* ctx, int enable);
double mrgingham_amd_chess_kernel_ms(mrgingham_amd_ctx* ctx, int* nlaunches);

/* The engine clock the level-0 response kernels (and the fused blend + blur kernels of mrgingham_amd_preprocess_batch / _preprocess16_batch) ACTUALLY ran at, in MHz, averaged over the launches issued since the last
 * call while kernel timing was enabled (1 or 2): workgroup 0 of each launch reads the shader-cycle counter (s_memtime) and the
 * constant-rate counter (s_memrealtime, hipDeviceAttributeWallClockRate) at its start and end and adds the two differences
 * to a pair of device counters -- four scalar instructions in one workgroup of the launch.  A VALU-bound kernel scales with
 * this clock, so a benchmark line that carries it can tell a slow box from a regression.  0 when nothing was probed.
 * Synchronises the device. */
double mrgingham_amd_sclk_mhz(mrgingham_amd_ctx* ctx);

#ifdef __cplusplus
}
#endif
