// Host side of libmrgingham_amd.so, the blob path over a batch of device-resident frames: mrgingham_amd_blobs_batch
// (find_blobs_from_image_array per frame), mrgingham_amd_find_circle_grids_batch (find_circle_grid_from_image_array per
// frame) and their statistics.  The detector itself is blobs.hip; see include/mrgingham_amd.h for the contract.
#include <string.h>

#include <atomic>

#include "ctx.h"

using namespace mrg;

// the checks the two entry points share: MRGINGHAM_AMD_ERR_ARG and nothing written
static int check_blob_frames(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* f) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (!f || (!f->frames && f->nframes > 0) || f->nframes < 0 || f->width < 0 || f->height < 0 || f->stride < f->width)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad frame batch descriptor");
    if (f->width > 32767 || f->height > 65535)  // the node keys: 15 bits of x, 16 bits of y
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "blob detector: frames up to 32767 x 65535");
    return 0;
}

extern "C" {

int mrgingham_amd_blobs_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int32_t* h_xy, int capacity_per_frame,
                              int32_t* h_counts, int nthreads) {
    int rc = check_blob_frames(ctx, fr);
    if (rc) return rc;
    if (!h_counts || capacity_per_frame < 0 || (!h_xy && capacity_per_frame > 0))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "NULL outputs or a negative capacity");
    fb_drain(ctx);
    const CallerDevice caller_device_;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<std::vector<int32_t>> xy;
    std::vector<char> bad;
    rc = blob_detect_batch(ctx, fr, host_threads(nthreads), xy, bad);
    if (rc && rc != MRGINGHAM_AMD_ERR_CAPACITY) return rc;
    for (int f = 0; f < fr->nframes; ++f) {
        const size_t n = xy[f].size() / 2;
        h_counts[f] = bad[f] ? -1 : (int32_t)n;
        const size_t keep = bad[f] ? 0 : n < (size_t)capacity_per_frame ? n : (size_t)capacity_per_frame;
        if (keep) memcpy(h_xy + (size_t)f * capacity_per_frame * 2, xy[f].data(), keep * 2 * sizeof(int32_t));
    }
    return rc;
}

int mrgingham_amd_find_circle_grids_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int gridn, double* h_boards,
                                          signed char* h_found, int nthreads) {
    int rc = check_blob_frames(ctx, fr);
    if (rc) return rc;
    if (gridn < 2 || !h_boards || !h_found) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad gridn / NULL outputs");
    fb_drain(ctx);
    const CallerDevice caller_device_;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    const int B = fr->nframes, N = gridn * gridn;
    nthreads = host_threads(nthreads);
    std::vector<std::vector<int32_t>> xy;
    std::vector<char> bad;
    rc = blob_detect_batch(ctx, fr, nthreads, xy, bad);
    if (rc && rc != MRGINGHAM_AMD_ERR_CAPACITY) return rc;
    // the grid finder on all keypoints of a frame (bridge.cc:104-113: no refinement), frames side by side
    std::atomic<int> next{0};
    auto worker = [&]() {
        GridScratch scratch;
        for (int f; (f = next.fetch_add(1)) < B;) {
            const int n = (int)(xy[f].size() / 2);
            h_found[f] = !bad[f] && n >= N && grid_of_candidates(xy[f].data(), n, gridn, h_boards + (size_t)f * N * 2, &scratch) ? 0 : -1;
        }
    };
    ctx->pool.run(nthreads < B ? nthreads : B, worker);
    return rc;
}

int mrgingham_amd_blobs_stats(mrgingham_amd_ctx* ctx, double* out, int n, int reset) {
    if (!ctx || !out || n < 0) return MRGINGHAM_AMD_ERR_ARG;
    for (int i = 0; i < n && i < MRGINGHAM_AMD_BLOBS_STATS; ++i) out[i] = ctx->blob_stat[i];
    if (reset)
        for (double& v : ctx->blob_stat) v = 0;
    return MRGINGHAM_AMD_BLOBS_STATS;
}

}  // extern "C"
