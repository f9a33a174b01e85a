// What the file-list loaders share (ctx.h lists the seven of them by file): the check of their descriptor, the zeroing of
// a failed file's frame, the two-slot chunk ring, of which each loader is a stage, the stage of the loaders that send a
// file's raster to the device as it lies on disk (BMP, Netpbm), and the launch shape of the unpack kernels.  Host code
// only; the chunk size is loader.h, the shape's arithmetic unpack_rows.h.
#include <string.h>

#include "ctx.h"
#include "loader.h"

namespace mrg {

int check_file_batch(mrgingham_amd_ctx* ctx, const char* format, const char* const* filenames, int nfiles, int width, int height,
                     size_t elem, const void* d_out, int64_t frame_pitch, int stride, const int32_t* h_status) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (nfiles < 0 || width <= 0 || height <= 0 || (elem != 1 && elem != 2) || stride < width || frame_pitch < 0 ||
        (nfiles > 0 && (!filenames || !d_out || !h_status)) || ((uintptr_t)d_out & (elem - 1)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad %s file batch descriptor", format);
    if (width > 32767 || height > 32767)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "frames larger than 32767 pixels per side are not supported");
    for (int i = 0; i < nfiles; ++i)
        if (!filenames[i]) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad %s file batch descriptor", format);
    return 0;
}

hipError_t zero_frame(void* d_out, int64_t frame, int64_t frame_pitch, int stride, int width, int height, size_t elem, hipStream_t s) {
    return hipMemset2DAsync((char*)d_out + (size_t)frame * (size_t)frame_pitch * elem, (size_t)stride * elem, 0, (size_t)width * elem,
                            (size_t)height, s);
}

LoaderStage zero_failed_frames(mrgingham_amd_ctx* ctx, void* d_out, int64_t frame_pitch, int stride, int width, int height, size_t elem,
                               const int32_t* h_status) {
    return [=](int, int f0, int n) -> int {
        for (int i = f0; i < f0 + n; ++i)
            if (h_status[i] != 0) MRG_HIP_CHECK(zero_frame(d_out, i, frame_pitch, stride, width, height, elem, ctx->pix));
        return 0;
    };
}

int unpack_launch_shape(mrgingham_amd_ctx* ctx, const void* d_out, long long frame_pitch_b, long long stride_b, long long row_bytes_out,
                        long long nrows, UnpackShape* shape) {
    int cus = 0;
    MRG_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    const bool aligned = !((uintptr_t)d_out & 15) && !(frame_pitch_b & 15) && !(stride_b & 15);
    *shape = unpack_shape(cus, aligned, row_bytes_out, nrows);
    return 0;
}

int loader_ring(mrgingham_amd_ctx* ctx, int nfiles, int chunk, size_t dev_bytes, size_t pin_bytes, const LoaderStage& stage,
                const LoaderStage& after, const std::function<int(int k)>& finish) {
    const int nslots = nfiles > chunk ? 2 : 1;
    int rc;
    for (int k = 0; k < nslots; ++k) {
        auto& slot = ctx->loader_slot[k];
        if ((rc = ensure(ctx, slot.dev, dev_bytes))) return rc;
        if (pin_bytes && (rc = ensure_pinned(ctx, slot.pin, pin_bytes, 0, true))) return rc;
        MRG_HIP_CHECK(slot.ev.create(hipEventDisableTiming));
    }
    hipStream_t s = ctx->pix;
    bool busy[2] = {false, false};
    // the chunk in slot k has passed the stream: the upload out of its staging is done, what it downloads is on the host
    auto passed = [&](int k) -> int {
        MRG_HIP_CHECK(hipEventSynchronize(ctx->loader_slot[k].ev));
        busy[k] = false;
        return finish ? finish(k) : 0;
    };
    for (int f0 = 0, k = 0; f0 < nfiles; f0 += chunk, k ^= nslots - 1) {
        const int n = nfiles - f0 < chunk ? nfiles - f0 : chunk;
        if (busy[k] && (rc = passed(k))) return rc;
        if ((rc = stage(k, f0, n))) return rc;
        MRG_HIP_CHECK(hipEventRecord(ctx->loader_slot[k].ev, s));
        busy[k] = true;
        if (after && (rc = after(k, f0, n))) return rc;
    }
    for (int k = 0; finish && k < nslots; ++k)
        if (busy[k] && (rc = passed(k))) return rc;
    MRG_HIP_CHECK(hipStreamSynchronize(s));
    return MRGINGHAM_AMD_OK;
}

int read_staged_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height, int bits, void* d_out,
                      int64_t frame_pitch, int stride, int nthreads, int32_t* h_status, const StagedFormat& fmt) {
    if (nfiles == 0) return 0;
    fb_drain(ctx);
    const CallerDevice caller_device_;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    nthreads = host_threads(nthreads);
    hipStream_t s = ctx->pix;
    const size_t es = (size_t)bits / 8, npx = (size_t)width * height * es;  // bytes of a sample, of a frame's samples

    // the headers first: what every file is, and with that the one size of the staging areas
    struct File {
        int8_t route = 0;  // 0 failed (h_status says how), 1 its raster through the kernel, 2 decoded by a host thread
        size_t raster = 0;
    };
    std::vector<File> file((size_t)nfiles);
    try {
        for_files<StagedThread>(ctx->pool, nthreads, nfiles, [&](int i, StagedThread& t) {
            int32_t st = -1;
            try {
                int route = 0;
                st = fmt.header(i, t, &route, &file[(size_t)i].raster);
                if (st == 0) file[(size_t)i].route = (int8_t)route;
            } catch (...) {  // std::bad_alloc
                st = -1;
            }
            h_status[i] = st;
        });
    } catch (...) {
        return fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "out of host memory");
    }
    // every file of a chunk gets one area of the staging, a multiple of 16 bytes: its raster lies there as in the file (a
    // host-decoded file: its grey samples, dense); the front bytes of the chunk's files lie in front of the areas
    size_t area = 16;
    for (const File& f : file) {
        const size_t need = f.route == 1 ? f.raster : f.route == 2 ? npx : 0;
        if (((need + 15) & ~(size_t)15) > area) area = (need + 15) & ~(size_t)15;
    }
    const int chunk = loader_chunk_frames(ctx->jpeg_coef_budget, area + fmt.front, nfiles, nthreads, fmt.chunk_cap);
    const size_t front_bytes = (size_t)chunk * fmt.front;
    auto stage = [&](int k, int f0, int n) -> int {
        uint8_t* h_front = (uint8_t*)ctx->loader_slot[k].pin.p;
        uint8_t* h_pay = h_front + front_bytes;
        for_files<StagedThread>(ctx->pool, nthreads, n, [&](int i, StagedThread& t) {
            const File& f = file[(size_t)(f0 + i)];
            if (f.route == 0) return;
            bool ok = false;
            uint8_t* dst = h_pay + (size_t)i * area;
            try {
                if (f.route == 2) {
                    ok = read_image(filenames[f0 + i], t.im) && t.im.depth == bits && t.im.w == width && t.im.h == height;
                    if (ok) memcpy(dst, bits == 8 ? (const void*)t.im.px8.data() : (const void*)t.im.px16.data(), npx);
                } else {
                    ok = fmt.stage_raster(f0 + i, t, dst, h_front + fmt.front * (size_t)i);
                }
            } catch (...) {  // std::bad_alloc
                ok = false;
            }
            if (!ok) h_status[f0 + i] = -1;
        });
        uint8_t* d_front = (uint8_t*)ctx->loader_slot[k].dev.p;
        uint8_t* d_pay = d_front + front_bytes;
        MRG_HIP_CHECK(hipMemcpyAsync(d_front, h_front, front_bytes + (size_t)n * area, hipMemcpyHostToDevice, s));
        // one launch per run of files with the same layout
        for (int i = 0; i < n;) {
            uint8_t* frame = (uint8_t*)d_out + (size_t)(f0 + i) * (size_t)frame_pitch * es;
            if (h_status[f0 + i] != 0) { ++i; continue; }  // (zeroed behind the launches)
            if (file[(size_t)(f0 + i)].route == 2) {
                MRG_HIP_CHECK(hipMemcpy2DAsync(frame, (size_t)stride * es, d_pay + (size_t)i * area, (size_t)width * es, (size_t)width * es,
                                               (size_t)height, hipMemcpyDeviceToDevice, s));
                ++i;
                continue;
            }
            int e = i + 1;
            while (e < n && h_status[f0 + e] == 0 && file[(size_t)(f0 + e)].route == 1 && fmt.same_launch(f0 + i, f0 + e)) ++e;
            const int lrc = fmt.launch(f0 + i, e - i, d_pay + (size_t)i * area, (int64_t)area, d_front + fmt.front * (size_t)i, frame);
            if (lrc) return lrc;
            i = e;
        }
        return 0;
    };
    // a failed file's area holds whatever the slot held before: its frame is zeroed behind the launches
    const size_t slot_bytes = front_bytes + (size_t)chunk * area;
    return loader_ring(ctx, nfiles, chunk, slot_bytes, slot_bytes, stage,
                       zero_failed_frames(ctx, d_out, frame_pitch, stride, width, height, es, h_status), nullptr);
}

}  // namespace mrg
