// How many files the file-list loaders (mrgingham_amd_read_jpegs_batch, _read_pngs_batch, _read_pgms_batch,
// _read_tiffs_batch, _read_bmps_batch, _read_pnms_batch) take per chunk, host only and free of every other header of the
// library, so that a stand-alone program can include it (tests/boundary/loader_plan_main.cpp).  The rest of what the loaders share is loader.hip (declared in ctx.h).
#pragma once
#include <stddef.h>

namespace mrg {

// Two chunks are in flight, so one gets half of budget_bytes: as many files of bytes_per_frame (> 0) as fit into that, at
// least 1 and at most nfiles (>= 1); above nthreads (>= 1) whole rounds of the host threads; at most `cap` if cap > 0
// (the test hooks "jpeg_chunk_frames", "png_", "pgm_", "tiff_", "bmp_" and "pnm_chunk_frames").
inline int loader_chunk_frames(size_t budget_bytes, size_t bytes_per_frame, int nfiles, int nthreads, int cap) {
    const size_t fit = budget_bytes / 2 / bytes_per_frame;
    int chunk = fit < 1 ? 1 : fit > (size_t)nfiles ? nfiles : (int)fit;
    if (chunk > nthreads) chunk -= chunk % nthreads;
    if (cap > 0 && chunk > cap) chunk = cap;
    return chunk;
}

}  // namespace mrg
