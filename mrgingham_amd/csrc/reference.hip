// Host side of libmrgingham_amd.so, the reference's own C symbols over ONE frame: the per-thread contexts and their
// devices, host allocation and the wait policy, mrgingham_ChESS_response_5, the *_C functions of the reference's Python
// bridge, the grid finder's C entries, the file entry points, and the command-line tool's preprocess / process_image.
// The board search itself is boards.hip's (find_board_on_device).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ctx.h"
#include "image_io.h"

namespace mrg {

// Which device the k-th thread that calls a reference symbol gets when nobody said otherwise: MRGINGHAM_AMD_DEVICE
// (every thread on that device) or, with the variable unset, k modulo the number of devices -- the reference's own
// parallelism is N worker threads with image i on worker i % N (mrgingham-from-image.cc:50, :374-379), and mapped this
// way its workers spread over the GPUs of a node by themselves.
static std::atomic<int> g_thread_counter{0};
struct ThreadCtxHolder {
    mrgingham_amd_ctx* ctx = nullptr;
    int requested = -1;  // mrgingham_amd_set_thread_device
    ~ThreadCtxHolder() { /* leaked on purpose: HIP may already be torn down at thread exit */ }
};
static thread_local ThreadCtxHolder t_holder;

static mrgingham_amd_ctx* thread_ctx() {
    // One context per calling thread: the reference is called from N worker
    // pthreads at once (mrgingham-from-image.cc:374-379).
    ThreadCtxHolder& h = t_holder;
    if (!h.ctx) {
        int dev = h.requested;
        const bool counted = dev < 0;
        if (counted) dev = mrgingham_amd_device_for_thread(g_thread_counter.fetch_add(1), mrgingham_amd_device_count(),
                                                           getenv("MRGINGHAM_AMD_DEVICE"));
        h.ctx = mrgingham_amd_create(dev);
        if (!h.ctx && counted) g_thread_counter.fetch_sub(1);  // a slot of the round-robin is used by a context, not by an attempt
    }
    return h.ctx;
}
// The calling thread's context with its device current (the caller holds a CallerDevice); NULL when there is none.
static mrgingham_amd_ctx* device_ctx() {
    mrgingham_amd_ctx* ctx = thread_ctx();
    if (ctx) hipSetDevice(ctx->device);
    return ctx;
}

// Upload one host frame as a dense device image; fills `fr`.
static int upload_frame(mrgingham_amd_ctx* ctx, const void* host, int rows, int cols, int stride,
                        mrgingham_amd_frames* fr) {
    int rc;
    if ((rc = ensure(ctx, ctx->io_frame, (size_t)rows * cols + 64))) return rc;
    // stream-ordered on streams[0]: the kernels that read it are queued on the same stream
    // (a dense frame as ONE copy: the 2-D form goes through a slower path of the runtime even when the rows are contiguous)
    if (rows > 0 && cols > 0) {
        if (stride == cols)
            MRG_HIP_CHECK(hipMemcpyAsync(ctx->io_frame.p, host, (size_t)rows * cols, hipMemcpyHostToDevice, ctx->pix));
        else
            MRG_HIP_CHECK(copy_rows_async(ctx->io_frame.p, cols, host, stride, cols, rows, hipMemcpyHostToDevice,
                                           ctx->pix));
    }
    fr->frames = (const uint8_t*)ctx->io_frame.p;
    fr->frame_pitch = (int64_t)rows * cols;
    fr->nframes = 1;
    fr->width = cols;
    fr->height = rows;
    fr->stride = cols;
    return 0;
}

// The reference's --debug dumps of one detector / refinement pass (find_chessboard_corners.cc:282-315,
// :453-459, :513-541): the level image, the ChESS response normalised to 0..255 (raw, and with the
// negatives clamped), and a self-plotting vnlog of the corners.  Same file names, same messages.  The
// response PNGs follow cv::normalize(.., 0, 255, NORM_MINMAX) on CV_16S (single-precision scale and
// shift, round half to even) and imwrite's saturating conversion to 8 bit.
static void write_debug_dumps(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr1, int level, bool refinement,
                              const char* debug_image_filename, const double* pts_xy, int npts) {
    int w, h;
    if (level_dims(fr1->width, fr1->height, level, &w, &h) || w <= 0 || h <= 0) return;
    const size_t n = (size_t)w * h;
    char name[300];
    std::vector<uint8_t> img8(n);
    std::vector<int16_t> resp(n);
    if (ensure(ctx, ctx->dbg_img, n + 64) || ensure(ctx, ctx->dbg_resp, n * 2 + 64)) return;
    if (!refinement) {  // apply_image_pyramid_scaling dumps once per detector call (:453-459)
        if (mrgingham_amd_decimate_batch(ctx, fr1, level, (uint8_t*)ctx->dbg_img.p, ctx->pix) ||
            hipMemcpyAsync(img8.data(), ctx->dbg_img.p, n, hipMemcpyDeviceToHost, ctx->pix) != hipSuccess ||
            hipStreamSynchronize(ctx->pix) != hipSuccess)
            return;
        snprintf(name, sizeof(name), "/tmp/mrgingham-scaled-processed-level%d.png", level);
        if (write_png_gray8(name, img8.data(), w, h)) fprintf(stderr, "Wrote scaled,processed image to %s\n", name);
    }
    for (int positive = 0; positive < 2; ++positive) {
        if (mrgingham_amd_chess_response_batch(ctx, fr1, level, positive, (int16_t*)ctx->dbg_resp.p, ctx->pix) ||
            hipMemcpyAsync(resp.data(), ctx->dbg_resp.p, n * 2, hipMemcpyDeviceToHost, ctx->pix) != hipSuccess ||
            hipStreamSynchronize(ctx->pix) != hipSuccess)
            return;
        int lo = 32767, hi = -32768;
        for (int16_t v : resp) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
        const double scale = 255.0 * (hi - lo > 2.220446049250313e-16 ? 1.0 / (double)(hi - lo) : 0.0);
        const double shift = 0.0 - (double)lo * scale;
        const float a = (float)scale, b = (float)shift;
        for (size_t i = 0; i < n; ++i) {
            const float prod = (float)resp[i] * a;
            const float r = rintf(prod + b);
            img8[i] = (uint8_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
        }
        snprintf(name, sizeof(name), "/tmp/mrgingham-chess-response%s-level%d%s.png", refinement ? "-refinement" : "", level,
                 positive ? "-positive" : "");
        if (write_png_gray8(name, img8.data(), w, h))
            fprintf(stderr, positive ? "Wrote positive-only, normalized ChESS response to %s\n"
                                     : "Wrote a normalized ChESS response to %s\n", name);
    }
    if (refinement) snprintf(name, sizeof(name), "/tmp/mrgingham-1-corners-refinement-level%d.vnl", level);
    else snprintf(name, sizeof(name), "/tmp/mrgingham-1-corners.vnl");
    fprintf(stderr, "Writing self-plotting corner dump to %s\n", name);
    FILE* fp = fopen(name, "w");
    if (!fp) return;
    if (debug_image_filename)
        fprintf(fp, "#!/usr/bin/feedgnuplot --dom --with 'points pt 7 ps 2' --square --image %s\n", debug_image_filename);
    else
        fprintf(fp, "#!/usr/bin/feedgnuplot --dom --square --set 'yr [:] rev'\n");
    fprintf(fp, "# x y\n");
    for (int i = 0; i < npts; ++i) fprintf(fp, "%f %f\n", pts_xy[2 * i], pts_xy[2 * i + 1]);
    fclose(fp);
}

// Every candidate of ONE frame that already lives on the device (dense or strided), with the retry of
// the reference-symbol wrappers: a frame whose hot list or candidate table overflows the default
// capacity is re-run with one table entry per pixel.  Returns false on a device / argument error.
bool detect_one_frame_all(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr1, int level, std::vector<int32_t>& xy,
                          int32_t* count_out, bool debug, const char* debug_image_filename) {
    const int saved_shift = ctx->cap_shift;
    bool ok = false;
    int32_t count = 0;
    for (int attempt = 0; attempt < 4 && !ok; ++attempt) {
        if (ensure_level(ctx, level, 1, fr1->width, fr1->height, 0) || ensure_points(ctx, 1, 1)) break;
        const int cap = ctx->lvs[0][level].cand_cap;
        if (ensure(ctx, ctx->io_out, (size_t)cap * 8 + 64) || ensure(ctx, ctx->io_counts, 64)) break;
        if (mrgingham_amd_detect_batch(ctx, fr1, level, (int32_t*)ctx->io_out.p, cap, (int32_t*)ctx->io_counts.p)) break;
        // The count and the first candidates follow the search on its own stream into page-locked memory: one wait for
        // that stream instead of a full synchronisation with its status read-back and two blocking copies (3 x 15-20 us
        // of a 0.4 ms call).  A frame whose tables overflowed says so in its count (-1): only then the status words are
        // read, the tables grow and the call is made again.
        constexpr int kFast = 4000;  // candidates that travel with the count
        if (ensure_pinned(ctx, ctx->io_res_pin, 64 + (size_t)kFast * 8, 0, false)) break;
        int32_t* pin_count = (int32_t*)ctx->io_res_pin.p;
        int32_t* pin_xy = pin_count + 16;
        hipStream_t cc = ctx->ccs[ctx->cur];
        const int nfast = cap < kFast ? cap : kFast;
        if (hipMemcpyAsync(pin_count, ctx->io_counts.p, sizeof(int32_t), hipMemcpyDeviceToHost, cc) != hipSuccess ||
            hipMemcpyAsync(pin_xy, ctx->io_out.p, (size_t)nfast * 8, hipMemcpyDeviceToHost, cc) != hipSuccess ||
            hipStreamSynchronize(cc) != hipSuccess)
            break;
        count = *pin_count;
        if (count < 0) {
            const int rc = mrgingham_amd_sync(ctx);
            if (rc == MRGINGHAM_AMD_ERR_CAPACITY && attempt < 3) {
                // the tables have grown to what the frame asked for (mrgingham_amd_sync); the last retry takes a
                // table entry for every pixel (adversarial texture)
                if (attempt == 2) ctx->cap_shift = 0;
                continue;
            }
            break;  // (a count of -1 with nothing to grow: a device error)
        }
        xy.resize((size_t)count * 2);
        if (count > 0) memcpy(xy.data(), pin_xy, (size_t)(count < nfast ? count : nfast) * 8);
        if (count > nfast &&
            hipMemcpy(xy.data() + (size_t)nfast * 2, (const int32_t*)ctx->io_out.p + (size_t)nfast * 2, (size_t)(count - nfast) * 8,
                      hipMemcpyDeviceToHost) != hipSuccess)
            break;
        ok = true;
    }
    ctx->cap_shift = saved_shift;
    *count_out = count;
    if (ok && debug) {
        // the dump lists the corners in full-resolution pixels (:346-348); from the *1000 integers here,
        // i.e. to three decimals
        std::vector<double> p((size_t)(count > 0 ? count : 0) * 2);
        for (size_t i = 0; i < p.size(); ++i) p[i] = (double)xy[i] / kGridScale;
        write_debug_dumps(ctx, fr1, level, false, debug_image_filename, p.data(), count > 0 ? count : 0);
    }
    return ok;
}

// Common checks of apply_image_pyramid_scaling (find_chessboard_corners.cc:433-473).
bool check_level_and_layout(const char* fn, int Nrows, int Ncols, int stride, int level) {
    if (level < 0 || level > 10) {
        fprintf(stderr, "mrgingham_amd: %s(): Got an unreasonable image_pyramid_level = %d. Sorry.\n", fn, level);
        return false;
    }
    if (level == 0 && stride != Ncols && Nrows != 1) {
        fprintf(stderr, "mrgingham_amd: %s(): I can only handle continuous arrays (stride == width) currently."
                        " Sorry.\n", fn);
        return false;
    }
    return true;
}

// find_blobs_from_image_array (find_blobs.cc:14-46) on a frame that lives on the device as `fr` (one frame): candidates
// as (x, y) * 1000 ints.  The batch detector with a batch of one; a few host threads for the filters, as ever.
static bool blobs_on_device(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, std::vector<int32_t>& xy) {
    if (fr->width > 32767 || fr->height > 65535) {
        fail(ctx, MRGINGHAM_AMD_ERR_CAPACITY, "blob detector: frames up to 32767 x 65535");
        return false;
    }
    std::vector<std::vector<int32_t>> per_frame;
    std::vector<char> bad;
    const unsigned hw = std::thread::hardware_concurrency();
    if (blob_detect_batch(ctx, fr, (int)std::min(hw ? hw : 1u, 16u), per_frame, bad)) return false;
    xy.insert(xy.end(), per_frame[0].begin(), per_frame[0].end());
    return true;
}

// The blob path of the reference's *_C functions: one host frame onto the calling thread's device, its blobs.  (The
// caller keeps its CallerDevice: add_points runs on the context's device, as it always has.)
static bool blobs_of_host_frame(int Nrows, int Ncols, int stride, const char* imagebuffer, std::vector<int32_t>& xy) {
    mrgingham_amd_ctx* ctx = device_ctx();
    if (!ctx) return false;
    mrgingham_amd_frames fr;
    return upload_frame(ctx, imagebuffer, Nrows, Ncols, stride, &fr) == 0 &&
           blobs_on_device(ctx, &fr, xy);
}

// The 16-bit preprocessing of one host frame, mrgingham-from-image.cc:85-92 ([normalize to 0..65535 + CLAHE on 16 bits]
// -> convertTo(CV_8U, 255/65535)), then the box blur: `fr` is the 8-bit result on the device.
static bool preprocess16_on_device(mrgingham_amd_ctx* ctx, const uint16_t* image, int width, int height, int stride,
                                   int do_clahe, int blur_radius, mrgingham_amd_frames* fr) {
    const size_t npx = (size_t)width * height;
    if (ensure(ctx, ctx->io_frame16, npx * 2 + 64) || ensure(ctx, ctx->pre_out, npx + 64)) return false;
    if (copy_rows_async(ctx->io_frame16.p, (size_t)width * 2, image, (size_t)stride * 2, (size_t)width * 2, height,
                        hipMemcpyHostToDevice, ctx->pix) != hipSuccess)
        return false;
    if (queue_preprocess16(ctx, (const uint16_t*)ctx->io_frame16.p, (int64_t)npx, 1, width, height, width, do_clahe, blur_radius,
                           (uint8_t*)ctx->pre_out.p, ctx->pix))
        return false;
    *fr = mrgingham_amd_frames{(const uint8_t*)ctx->pre_out.p, (int64_t)npx, 1, width, height, width};
    return true;
}

// The level check of the board searches (find_chessboard_corners.cc:433-436), before anything runs.
static bool level_reasonable(const char* fn, int level) {
    if (level <= kMaxLevel) return true;
    fprintf(stderr, "mrgingham_amd: %s(): Got an unreasonable image_pyramid_level = %d. Sorry.\n", fn, level);
    return false;
}

// The grid finder's --debug-sequence trace for one call (bridge.cc:97-104, mrgingham-from-image.cc:262-276): both
// coordinates >= 0 switch it on (stderr).
struct TraceScope {
    TraceScope(int x, int y) { g_grid_debug_sequence = {x >= 0 && y >= 0, x, y}; }
    ~TraceScope() { g_grid_debug_sequence = {false, 0, 0}; }
};


// Refinement of host-side points against a frame that already lives on the device (one frame).
int refine_on_device(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, double* points_xy, signed char* level,
                     int Npoints, int image_pyramid_level, bool debug, const char* debug_image_filename) {
    std::vector<signed char> level_before;
    if (debug) level_before.assign(level, level + Npoints);
    const int saved_shift = ctx->cap_shift;
    int32_t nrefined = 0;
    bool ok = false;
    for (int attempt = 0; attempt < 4; ++attempt) {
        // layout of io_out: points | levels | npoints | nrefined
        const size_t o_lv = (size_t)Npoints * 16, o_np = o_lv + (((size_t)Npoints + 7) & ~(size_t)7), o_nr = o_np + 8;
        if (ensure(ctx, ctx->io_out, o_nr + 8)) break;
        char* base = (char*)ctx->io_out.p;
        // ONE block up and ONE block down (points | levels | npoints | nrefined through a host copy of the same layout):
        // every blocking copy of a few hundred bytes costs 15-20 us, and there were three each way
        std::vector<char>& blk = ctx->io_host_block;
        blk.assign(o_nr + 8, 0);
        memcpy(blk.data(), points_xy, (size_t)Npoints * 16);
        memcpy(blk.data() + o_lv, level, (size_t)Npoints);
        const int32_t np = Npoints;
        memcpy(blk.data() + o_np, &np, 4);
        if (hipMemcpy(base, blk.data(), o_nr + 8, hipMemcpyHostToDevice) != hipSuccess) break;
        if (mrgingham_amd_refine_batch(ctx, fr, image_pyramid_level, (double*)base, (signed char*)(base + o_lv),
                                       (const int32_t*)(base + o_np), Npoints, (int32_t*)(base + o_nr)))
            break;
        const int rc = mrgingham_amd_sync(ctx);
        if (rc == MRGINGHAM_AMD_ERR_CAPACITY && attempt < 3) {  // (the upload above restores the points)
            if (attempt == 2) ctx->cap_shift = 0;
            continue;
        }
        if (rc) break;
        if (hipMemcpy(blk.data(), base, o_nr + 8, hipMemcpyDeviceToHost) != hipSuccess) break;
        memcpy(&nrefined, blk.data() + o_nr, 4);
        memcpy(points_xy, blk.data(), (size_t)Npoints * 16);
        memcpy(level, blk.data() + o_lv, (size_t)Npoints);
        ok = true;
        break;
    }
    ctx->cap_shift = saved_shift;
    if (ok && debug) {  // the points refined by this pass, in index order (:390-392)
        std::vector<double> p;
        for (int i = 0; i < Npoints; ++i)
            if (level[i] != level_before[i]) { p.push_back(points_xy[2 * i]); p.push_back(points_xy[2 * i + 1]); }
        write_debug_dumps(ctx, fr, image_pyramid_level, true, debug_image_filename, p.data(), (int)(p.size() / 2));
    }
    return ok && nrefined > 0 ? nrefined : 0;
}

/* The reference's file entry points: find_chessboard_corners_from_image_file
 * (find_chessboard_corners.cc:623-648) and find_chessboard_from_image_file (mrgingham.cc:145-170) are
 * cv::imread(GRAYSCALE) followed by the array functions.  Here the file is decoded by csrc/image_io
 * (binary PGM, non-interlaced PNG; 16-bit samples are reduced to their high byte, as cv::imread without
 * IMREAD_ANYDEPTH does) -- same results as the array
 * functions on the decoded pixels, same "Couldn't open image" failure. */
static bool load_gray8(const char* who, const char* filename, mrg::Image& im, std::vector<uint8_t>& tmp,
                       const uint8_t** px) {
    if (!filename || !mrg::read_image(filename, im)) {
        fprintf(stderr, "mrgingham_amd: %s(): Couldn't open image '%s'. Sorry.\n", who, filename ? filename : "(null)");
        return false;
    }
    if (im.depth == 16) {
        mrg::to_8bit_imread(im, tmp);  // cv::imread(GRAYSCALE) keeps the high byte; the CLI's own path rescales
        *px = tmp.data();
    } else {
        *px = im.px8.data();
    }
    return true;
}

}  // namespace mrg

using namespace mrg;

extern "C" {

int mrgingham_amd_device_for_thread(int thread_index, int ndevices, const char* env_value) {
    if (env_value && *env_value) return atoi(env_value);
    if (ndevices <= 0) return 0;
    return (int)((unsigned)(thread_index < 0 ? 0 : thread_index) % (unsigned)ndevices);
}

int mrgingham_amd_set_thread_device(int device_ordinal) {
    const int ndev = mrgingham_amd_device_count();
    if (device_ordinal < 0 || device_ordinal >= ndev) {
        fprintf(stderr, "mrgingham_amd: device ordinal %d out of range (%d device(s))\n", device_ordinal, ndev);
        return MRGINGHAM_AMD_ERR_ARG;
    }
    ThreadCtxHolder& h = t_holder;
    h.requested = device_ordinal;
    if (h.ctx && h.ctx->device != device_ordinal) {
        mrgingham_amd_destroy(h.ctx);
        h.ctx = nullptr;
    }
    return MRGINGHAM_AMD_OK;
}

int mrgingham_amd_thread_device(void) {
    CallerDevice caller_device_;
    mrgingham_amd_ctx* ctx = thread_ctx();
    return ctx ? ctx->device : -1;
}

void* mrgingham_amd_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) return nullptr;
    static const int fill = scratch_fill_from_env();  // test hook (ctx.h, scratch_fill): no context here, the variable alone
    if (fill >= 0) memset(p, fill, bytes);
    return p;
}
void mrgingham_amd_host_free(void* p) {
    if (p) hipHostFree(p);
}
int mrgingham_amd_host_register(void* p, size_t bytes) {
    if (!p || bytes == 0) return MRGINGHAM_AMD_ERR_ARG;
    return hipHostRegister(p, bytes, hipHostRegisterPortable) == hipSuccess ? MRGINGHAM_AMD_OK : MRGINGHAM_AMD_ERR_DEVICE;
}
int mrgingham_amd_host_unregister(void* p) {
    if (!p) return MRGINGHAM_AMD_ERR_ARG;
    return hipHostUnregister(p) == hipSuccess ? MRGINGHAM_AMD_OK : MRGINGHAM_AMD_ERR_DEVICE;
}

int mrgingham_amd_set_wait_policy(int policy) {
    unsigned flag;
    switch (policy) {
        case 0: flag = hipDeviceScheduleAuto; break;
        case 1: flag = hipDeviceScheduleSpin; break;
        case 2: flag = hipDeviceScheduleYield; break;
        case 3: flag = hipDeviceScheduleBlockingSync; break;
        default: return MRGINGHAM_AMD_ERR_ARG;
    }
    int ndev = 0, prev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MRGINGHAM_AMD_ERR_DEVICE;
    hipGetDevice(&prev);
    int rc = MRGINGHAM_AMD_OK;
    for (int d = 0; d < ndev; ++d)
        if (hipSetDevice(d) != hipSuccess || hipSetDeviceFlags(flag) != hipSuccess) rc = MRGINGHAM_AMD_ERR_DEVICE;
    hipSetDevice(prev);
    (void)hipGetLastError();
    return rc;
}

void mrgingham_ChESS_response_5(int16_t* response, const uint8_t* image, int w, int h, int stride) {
    if (w < 15 || h < 15) return;  // no interior: the reference's loops do not execute (ChESS.c:62-63)
    CallerDevice caller_device_;
    mrgingham_amd_ctx* ctx = thread_ctx();
    if (!ctx || !response || !image) {
        fprintf(stderr, "mrgingham_amd: mrgingham_ChESS_response_5: no device context; response not written\n");
        return;
    }
    hipSetDevice(ctx->device);
    mrgingham_amd_frames fr;
    if (upload_frame(ctx, image, h, w, stride, &fr)) return;
    if (ensure(ctx, ctx->io_out, (size_t)w * h * 2 + 64)) return;
    if (mrgingham_amd_chess_response_batch(ctx, &fr, 0, 0, (int16_t*)ctx->io_out.p, ctx->pix)) return;
    // interior only, like the reference: the 7-pixel frame of `response` is not touched
    hipError_t e = hipSuccess;
    const size_t bytes = (size_t)w * h * 2;
    {
        // The strided copy of the interior into pageable memory goes through a slow path of the runtime (2.4 ms per 12 MP
        // frame, all of it this copy) that also serialises the threads of a process (hipMemcpy2DAsync: sixteen workers
        // of the command-line tool ran at an eighth of their rate behind one such copy per image).  Instead: whole rows
        // in plain copies into page-locked staging of the context, at the speed of the link, and -- for large frames
        // (12 MP: 25 MB back) in four chunks -- a few host threads that move the interior of each row block into the
        // caller's array as soon as the copy that carries it has landed.
        const bool small = bytes < (4u << 20);
        const int kChunks = small ? 1 : 4;
        (void)ensure_pinned(ctx, ctx->io_pin, bytes, 8, false);  // (without it: the message below)
        for (int c = 0; c < kChunks; ++c)
            (void)ctx->io_ev[c].create(hipEventDisableTiming);
        if (!ctx->io_pin.p || !ctx->io_ev[kChunks - 1]) {
            fprintf(stderr, "mrgingham_amd: ChESS response failed: no page-locked staging\n");
            return;
        }
        const int rows_per = (h + kChunks - 1) / kChunks;
        for (int c = 0; c < kChunks && e == hipSuccess; ++c) {
            const int y0 = c * rows_per, y1 = y0 + rows_per < h ? y0 + rows_per : h;
            if (y1 > y0)
                e = hipMemcpyAsync((char*)ctx->io_pin.p + (size_t)y0 * w * 2, (const char*)ctx->io_out.p + (size_t)y0 * w * 2,
                                   (size_t)(y1 - y0) * w * 2, hipMemcpyDeviceToHost, ctx->pix);
            if (e == hipSuccess) e = hipEventRecord(ctx->io_ev[c], ctx->pix);
        }
        if (e == hipSuccess) {
            std::atomic<int> next{0};
            std::atomic<int> failed{0};
            const int16_t* pin = (const int16_t*)ctx->io_pin.p;
            const int device = ctx->device;
            const Event* evs = ctx->io_ev;
            constexpr int kBlock = 32;  // rows per work item
            const int nblocks = (h - 2 * kMargin + kBlock - 1) / kBlock;
            auto mover = [&]() {
                hipSetDevice(device);
                int waited = -1;  // chunks known to have landed
                for (int b; (b = next.fetch_add(1)) < nblocks;) {
                    const int ya = kMargin + b * kBlock, yb = ya + kBlock < h - kMargin ? ya + kBlock : h - kMargin;
                    const int need = (yb - 1) / rows_per;
                    while (waited < need) {
                        if (hipEventSynchronize(evs[waited + 1]) != hipSuccess) { failed.store(1); return; }
                        ++waited;
                    }
                    for (int y = ya; y < yb; ++y)
                        memcpy(response + (size_t)y * w + kMargin, pin + (size_t)y * w + kMargin, (size_t)(w - 2 * kMargin) * 2);
                }
            };
            int nthreads = (int)std::thread::hardware_concurrency();
            nthreads = nthreads > 8 ? 8 : (nthreads < 1 ? 1 : nthreads);
            if (small) mover();  // (a few hundred KB: the calling thread)
            else ctx->pool.run(nthreads, mover);
            if (failed.load()) e = hipErrorUnknown;
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->pix);
        }
    }
    if (e != hipSuccess) fprintf(stderr, "mrgingham_amd: ChESS response failed: %s\n", hipGetErrorString(e));
}


bool find_chessboard_corners_from_image_array_C(int Nrows, int Ncols, int stride, char* imagebuffer,
                                                int image_pyramid_level, bool doblobs, bool debug,
                                                bool (*add_points)(int* xy, int N, double scale, void* cookie),
                                                void* cookie) {
    if (Nrows < 0 || Ncols < 0 || stride < Ncols || !imagebuffer || !add_points) return false;
    if (doblobs) {  // bridge.cc:50-55: the blob detector, level 0 only; always "found", possibly with 0 points
        if (image_pyramid_level != 0) return false;
        CallerDevice caller_device_;
        std::vector<int32_t> bxy;
        if (!blobs_of_host_frame(Nrows, Ncols, stride, imagebuffer, bxy)) return false;
        int32_t none[2] = {0, 0};
        return (*add_points)(bxy.empty() ? none : bxy.data(), (int)(bxy.size() / 2), 1. / kGridScale, cookie);
    }
    if (!check_level_and_layout(__func__, Nrows, Ncols, stride, image_pyramid_level)) return false;
    CallerDevice caller_device_;
    mrgingham_amd_ctx* ctx = device_ctx();
    if (!ctx) return false;
    std::vector<int32_t> xy;
    int32_t count = 0;
    mrgingham_amd_frames fr;
    const bool ok = upload_frame(ctx, imagebuffer, Nrows, Ncols, stride, &fr) == 0 &&
                    detect_one_frame_all(ctx, &fr, image_pyramid_level, xy, &count, debug, nullptr);
    if (!ok || count <= 0) return false;  // bridge.cc:61: nothing found -> false, add_points not called
    return (*add_points)(xy.data(), (int)count, 1. / kGridScale, cookie);  // bridge.cc:66-69
}

int refine_chessboard_corners_from_image_array_C(int Nrows, int Ncols, int stride, char* imagebuffer,
                                                 double* points_xy, signed char* level, int Npoints,
                                                 int image_pyramid_level, bool debug) {
    if (Nrows < 0 || Ncols < 0 || stride < Ncols || !imagebuffer || Npoints < 0) return 0;
    if (Npoints > 0 && (!points_xy || !level)) return 0;
    if (!check_level_and_layout(__func__, Nrows, Ncols, stride, image_pyramid_level)) return 0;
    if (Npoints == 0) return 0;
    CallerDevice caller_device_;
    mrgingham_amd_ctx* ctx = device_ctx();
    if (!ctx) return 0;
    mrgingham_amd_frames fr;
    if (upload_frame(ctx, imagebuffer, Nrows, Ncols, stride, &fr)) return 0;
    return refine_on_device(ctx, &fr, points_xy, level, Npoints, image_pyramid_level, debug, nullptr);
}

/* C face of mrgingham::find_grid_from_points (mrgingham.hh:83-87; find_grid.cc:1216-1445): host only. */
bool mrgingham_amd_find_grid_from_points(const int* xy_scaled, int npoints, int gridn, double* xy_out) {
    if (!xy_scaled || !xy_out || npoints < 0 || gridn < 2) return false;
    return grid_of_candidates(xy_scaled, npoints, gridn, xy_out);
}

bool mrgingham_amd_find_grid_from_points_traced(const int* xy_scaled, int npoints, int gridn, double* xy_out,
                                                int debug, int debug_sequence_x, int debug_sequence_y) {
    mrg::g_grid_debug = debug != 0;
    mrg::g_grid_debug_sequence = {debug_sequence_x >= 0 && debug_sequence_y >= 0, debug_sequence_x, debug_sequence_y};
    const bool ok = mrgingham_amd_find_grid_from_points(xy_scaled, npoints, gridn, xy_out);
    mrg::g_grid_debug_sequence = {false, 0, 0};
    mrg::g_grid_debug = false;
    return ok;
}

/* Test hook: the same with the visiting order perturbed (grid.h, GridPerturbation). */
bool mrgingham_amd_find_grid_from_points_perturbed(const int* xy_scaled, int npoints, int gridn, double* xy_out,
                                                   unsigned ring_seed, int last_match) {
    g_grid_perturbation = GridPerturbation{ring_seed, (last_match & 1) != 0, (last_match & 2) != 0};
    const bool ok = mrgingham_amd_find_grid_from_points(xy_scaled, npoints, gridn, xy_out);
    g_grid_perturbation = GridPerturbation{0u, false, false};
    return ok;
}

/* Replaces find_chessboard_from_image_array_C (mrgingham_pywrap_cplusplus_bridge.h:25-42, .cc:72-138),
 * i.e. mrgingham::find_chessboard_from_image_array with refinement on (mrgingham.cc:38-140): detector
 * and refinement on the GPU, grid finder on the host. */
bool find_chessboard_from_image_array_C(int Nrows, int Ncols, int stride, char* imagebuffer, const int gridn,
                                        int image_pyramid_level, bool doblobs, bool debug, int debug_sequence_x,
                                        int debug_sequence_y,
                                        bool (*add_points)(double* xy, int N, void* cookie), void* cookie) {
    const TraceScope trace_scope(debug_sequence_x, debug_sequence_y);
    if (Nrows < 0 || Ncols < 0 || stride < Ncols || !imagebuffer || !add_points || gridn < 2) return false;
    if (doblobs) {  // bridge.cc:104-113: find_circle_grid_from_image_array = blobs + grid finder, no refinement
        if (image_pyramid_level != 0) return false;
        CallerDevice caller_device_;
        std::vector<int32_t> bxy;
        if (!blobs_of_host_frame(Nrows, Ncols, stride, imagebuffer, bxy)) return false;
        std::vector<double> grid((size_t)gridn * gridn * 2);
        if (!grid_of_candidates(bxy.data(), (int)(bxy.size() / 2), gridn, grid.data())) return false;
        return (*add_points)(grid.data(), gridn * gridn, cookie);
    }
    if (!level_reasonable(__func__, image_pyramid_level)) return false;
    CallerDevice caller_device_;
    mrgingham_amd_ctx* ctx = device_ctx();
    if (!ctx) return false;
    mrgingham_amd_frames fr;
    if (upload_frame(ctx, imagebuffer, Nrows, Ncols, stride, &fr)) return false;
    std::vector<PointD> board;
    std::vector<signed char> lv;
    if (find_board_on_device(ctx, __func__, &fr, gridn, image_pyramid_level, true, board, lv, debug, nullptr) < 0)
        return false;
    static_assert(sizeof(PointD) == 2 * sizeof(double), "add_points() takes interleaved doubles");
    return (*add_points)(&board[0].x, gridn * gridn, cookie);  // bridge.cc:133-137
}

int mrgingham_amd_read_image(const char* filename, int cli_scaling, uint8_t* out, size_t out_capacity, int* width,
                             int* height, int* depth) {
    mrg::Image im;
    if (!filename || !mrg::read_image(filename, im)) return -1;
    if (width) *width = im.w;
    if (height) *height = im.h;
    if (depth) *depth = im.depth;
    const size_t n = (size_t)im.w * im.h;
    if (!out) return 0;
    if (out_capacity < n) return -2;
    if (im.depth == 16) {
        std::vector<uint8_t> tmp;
        if (cli_scaling) mrg::to_8bit(im, tmp);
        else mrg::to_8bit_imread(im, tmp);
        memcpy(out, tmp.data(), n);
    } else {
        memcpy(out, im.px8.data(), n);
    }
    return 0;
}

bool find_chessboard_corners_from_image_file_C(const char* filename, int image_pyramid_level, bool debug,
                                               bool (*add_points)(int* xy, int N, double scale, void* cookie),
                                               void* cookie) {
    mrg::Image im;
    std::vector<uint8_t> tmp;
    const uint8_t* px = nullptr;
    if (!load_gray8(__func__, filename, im, tmp, &px)) return false;
    return find_chessboard_corners_from_image_array_C(im.h, im.w, im.w, (char*)px, image_pyramid_level, false, debug,
                                                      add_points, cookie);
}

bool find_chessboard_from_image_file_C(const char* filename, const int gridn, int image_pyramid_level, bool debug,
                                       bool (*add_points)(double* xy, int N, void* cookie), void* cookie) {
    mrg::Image im;
    std::vector<uint8_t> tmp;
    const uint8_t* px = nullptr;
    if (!load_gray8(__func__, filename, im, tmp, &px)) return false;
    return find_chessboard_from_image_array_C(im.h, im.w, im.w, (char*)px, gridn, image_pyramid_level, false, debug, -1,
                                              -1, add_points, cookie);
}

/* The preprocessing alone, host image in, host image out (dense width x height bytes): what the
 * Python recipe in find_board.docstring:8-10 does with cv2 before calling find_board.  Returns 0, or
 * -2 on an argument / device error. */
int mrgingham_amd_preprocess_image(const uint8_t* image, int width, int height, int stride, int do_clahe,
                                   int blur_radius, uint8_t* out) {
    if (!image || !out || width <= 0 || height <= 0 || stride < width || blur_radius < 0) return -2;
    CallerDevice caller_device_;
    mrgingham_amd_ctx* ctx = device_ctx();
    if (!ctx) return -2;
    mrgingham_amd_frames fr;
    if (upload_frame(ctx, image, height, width, stride, &fr)) return -2;
    if (ensure(ctx, ctx->pre_out, (size_t)width * height + 64)) return -2;
    if (mrgingham_amd_preprocess_batch(ctx, &fr, do_clahe, blur_radius, (uint8_t*)ctx->pre_out.p, ctx->pix)) return -2;
    if (hipMemcpyAsync(out, ctx->pre_out.p, (size_t)width * height, hipMemcpyDeviceToHost, ctx->pix) != hipSuccess ||
        hipStreamSynchronize(ctx->pix) != hipSuccess)
        return -2;
    return 0;
}

/* What one worker of the reference CLI does with one decoded 8-bit image
 * (mrgingham-from-image.cc:71-111 and :160-171): [normalize + CLAHE] -> box blur ->
 * find_chessboard_from_image_array.  The frame is uploaded once; preprocessing, detector and
 * refinement run on the device, the grid finder on the host.  Returns the level the board was found
 * at (>= 0), -1 when no board was found, -2 on an argument / device error. */
int mrgingham_amd_preprocess_image16(const uint16_t* image, int width, int height, int stride, int do_clahe,
                                     int blur_radius, uint8_t* out) {
    if (!image || !out || width <= 0 || height <= 0 || stride < width || blur_radius < 0 || width > 32767 || height > 32767)
        return -2;
    CallerDevice caller_device_;
    mrgingham_amd_ctx* ctx = device_ctx();
    mrgingham_amd_frames fr;
    if (!ctx || !preprocess16_on_device(ctx, image, width, height, stride, do_clahe, blur_radius, &fr)) return -2;
    if (hipMemcpyAsync(out, fr.frames, (size_t)width * height, hipMemcpyDeviceToHost, ctx->pix) != hipSuccess ||
        hipStreamSynchronize(ctx->pix) != hipSuccess)
        return -2;
    return 0;
}

int mrgingham_amd_process_image_ex(const void* image, int bits, int width, int height, int stride,
                                   const mrgingham_amd_cli_options* o, double* xy_out, signed char* levels_out) {
    if (!image || !o || (bits != 8 && bits != 16) || width <= 0 || height <= 0 || stride < width || o->gridn < 2 ||
        !xy_out || o->blur_radius < 0 || width > 32767 || height > 32767)
        return -2;
    if (!level_reasonable(__func__, o->image_pyramid_level)) return -2;
    const TraceScope trace_scope(o->debug_sequence_x, o->debug_sequence_y);  // --debug-sequence X,Y of the command-line tool
    CallerDevice caller_device_;
    mrgingham_amd_ctx* ctx = device_ctx();
    if (!ctx) return -2;
    const size_t npx = (size_t)width * height;
    mrgingham_amd_frames fr;
    if (bits == 8) {
        if (upload_frame(ctx, image, height, width, stride, &fr)) return -2;
        if (o->do_clahe || o->blur_radius > 0) {
            if (ensure(ctx, ctx->pre_out, npx + 64)) return -2;
            if (mrgingham_amd_preprocess_batch(ctx, &fr, o->do_clahe, o->blur_radius, (uint8_t*)ctx->pre_out.p, ctx->pix))
                return -2;
            fr.frames = (const uint8_t*)ctx->pre_out.p;  // same stream as the detector's pixel kernels
        }
    } else if (!preprocess16_on_device(ctx, (const uint16_t*)image, width, height, stride, o->do_clahe, o->blur_radius, &fr)) {
        return -2;  // mrgingham-from-image.cc:85-92
    }
    if (o->debug) {  // mrgingham-from-image.cc:113-148: /tmp/<basename without extension>_preprocessed.png
        const char* fn = o->filename ? o->filename : "image";
        const char* slash = strrchr(fn, '/');
        std::string base = slash ? slash + 1 : fn;
        const size_t dot = base.rfind('.');
        if (dot != std::string::npos) base.resize(dot);
        const std::string outname = "/tmp/" + base + "_preprocessed.png";
        std::vector<uint8_t> host(npx);
        if (copy_rows_async(host.data(), width, fr.frames, fr.stride, width, height, hipMemcpyDeviceToHost, ctx->pix) ==
                hipSuccess &&
            hipStreamSynchronize(ctx->pix) == hipSuccess && write_png_gray8(outname.c_str(), host.data(), width, height))
            fprintf(stderr, "Wrote preprocessed image to %s\n", outname.c_str());
    }
    std::vector<PointD> board;
    std::vector<signed char> lv;
    if (o->do_blobs) {
        // mrgingham-from-image.cc:153-160: find_circle_grid_from_image_array on the preprocessed image, "level" 0
        std::vector<int32_t> bxy;
        if (!blobs_on_device(ctx, &fr, bxy)) return -2;
        if (!grid_of_candidates(bxy.data(), (int)(bxy.size() / 2), o->gridn, xy_out)) return -1;
        if (levels_out) memset(levels_out, 0, (size_t)o->gridn * o->gridn);
        return 0;
    }
    const int level = find_board_on_device(ctx, __func__, &fr, o->gridn, o->image_pyramid_level, o->do_refine != 0,
                                           board, lv, o->debug != 0, o->filename);
    if (level < 0) return -1;
    memcpy(xy_out, &board[0].x, sizeof(double) * 2 * (size_t)o->gridn * o->gridn);
    if (levels_out) memcpy(levels_out, lv.data(), (size_t)o->gridn * o->gridn);
    return level;
}

int mrgingham_amd_process_image(const uint8_t* image, int width, int height, int stride, int do_clahe,
                                int blur_radius, int gridn, int image_pyramid_level, int do_refine, double* xy_out,
                                signed char* levels_out) {
    mrgingham_amd_cli_options o{};
    o.do_clahe = do_clahe;
    o.blur_radius = blur_radius;
    o.gridn = gridn;
    o.image_pyramid_level = image_pyramid_level;
    o.do_refine = do_refine;
    return mrgingham_amd_process_image_ex(image, 8, width, height, stride, &o, xy_out, levels_out);
}

}  // extern "C"
