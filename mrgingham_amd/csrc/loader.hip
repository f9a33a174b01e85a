// What the file-list loaders share (mrgingham_amd_read_jpegs_batch in jpeg_idct.hip, its device-entropy route in
// jpeg_huff.hip, mrgingham_amd_read_pngs_batch in png_recon.hip, _read_pgms_batch in pgm_unpack.hip, _read_tiffs_batch in
// tiff_decode.hip): the check of their descriptor, the zeroing of a failed
// file's frame and the two-slot chunk ring, of which each loader is a stage.  Host code only; the chunk size is loader.h.
#include "ctx.h"

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

LoaderStage zero_failed_frames(mrgingham_amd_ctx* ctx, uint8_t* d_out, int64_t frame_pitch, int stride, int width, int height,
                               const int32_t* h_status) {
    return [=](int, int f0, int n) -> int {
        for (int i = f0; i < f0 + n; ++i)
            if (h_status[i] != 0) MRG_HIP_CHECK(zero_frame(d_out, i, frame_pitch, stride, width, height, 1, ctx->pix));
        return 0;
    };
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

}  // namespace mrg
