// Packed camera frames on the device: rows of 10 / 12 / 14-bit samples as a camera or a frame grabber delivers them --
// an LSB-first bit stream (Mono10p, Mono12p, Mono14p) or 3-byte pixel pairs (Mono10Packed, Mono12Packed), rows of
// row_bytes bytes -- to native uint16 frames with a row stride.  The samples themselves are raw_pixels.h, the text the host
// entry (image_io.cpp: mrgingham_amd_raw_unpack_image) runs.  See include/mrgingham_amd.h for the contract of the entry
// points and DESIGN.md section 4.20 for the byte model and the numbers.
#include "ctx.h"
#include "raw_pixels.h"
#include "unpack_rows.h"

using namespace mrg;

namespace {

// a row of a packed frame: it begins at byte y * rowb of the frame's payload, at any phase; a word begins at any bit
// (streams) or at either sample of a pair
template <int FMT>
struct RawRows {
    const uint8_t* __restrict__ payload;
    long long payload_pitch, rowb;
    struct Row {
        const uint8_t* __restrict__ base;
        long long limit, row_off;
        __device__ __forceinline__ void pixels(int x0, int n, uint32_t d[4]) const { raw_pixels<FMT>(base, limit, row_off, x0, n, d); }
    };
    __device__ __forceinline__ Row row(long long f, int y) const { return Row{payload + f * payload_pitch, payload_pitch, (long long)y * rowb}; }
};

// unpack_rows.h has the schedule
template <int FMT>
__global__ __launch_bounds__(kUnpackLanes) void raw_unpack_kernel(const uint8_t* __restrict__ payload, long long payload_pitch, long long rowb,
                                                                  int width, int height, long long nrows, uint8_t* __restrict__ out,
                                                                  long long frame_pitch_b, long long stride_b, int lpr_shift) {
    unpack_rows<2>(RawRows<FMT>{payload, payload_pitch, rowb}, width, height, nrows, out, frame_pitch_b, stride_b, lpr_shift);
}

// checked arguments -> the launch (frame_pitch and stride in samples)
int launch_raw_unpack(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, int nframes, int width, int height, int64_t row_bytes,
                      int format, uint16_t* d_out, int64_t frame_pitch, int stride, hipStream_t s) {
    const long long nrows = (long long)nframes * height;
    UnpackShape sh;
    if (int rc = unpack_launch_shape(ctx, d_out, (long long)frame_pitch * 2, (long long)stride * 2, (long long)width * 2, nrows, &sh)) return rc;
#define MRG_RAW_LAUNCH(F)                                                                                                                    \
    case F:                                                                                                                                  \
        hipLaunchKernelGGL((raw_unpack_kernel<F>), dim3((unsigned)sh.blocks), dim3(kUnpackLanes), 0, s, d_payload, (long long)payload_pitch, \
                           (long long)row_bytes, width, height, nrows, (uint8_t*)d_out, (long long)frame_pitch * 2, (long long)stride * 2,   \
                           sh.lpr_shift);                                                                                                    \
        break
    switch (format) {
        MRG_RAW_LAUNCH(MRGINGHAM_AMD_RAW_P10);
        MRG_RAW_LAUNCH(MRGINGHAM_AMD_RAW_P12);
        MRG_RAW_LAUNCH(MRGINGHAM_AMD_RAW_P14);
        MRG_RAW_LAUNCH(MRGINGHAM_AMD_RAW_GEV10);
        MRG_RAW_LAUNCH(MRGINGHAM_AMD_RAW_GEV12);
    }
#undef MRG_RAW_LAUNCH
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

void mrgingham_amd_raw_unpack_geometry(int* lanes_per_workgroup, int* max_workgroups_per_cu) {
    if (lanes_per_workgroup) *lanes_per_workgroup = kUnpackLanes;
    if (max_workgroups_per_cu) *max_workgroups_per_cu = kUnpackWorkgroupsPerCu;
}

int mrgingham_amd_raw_unpack_batch(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, int nframes, int width, int height,
                                   int64_t row_bytes, int format, uint16_t* d_out, int64_t frame_pitch, int stride, void* stream) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (!raw_format_ok(format)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "packed frames: format is one of MRGINGHAM_AMD_RAW_P10, _P12, _P14, _GEV10, _GEV12");
    if (width < 1 || height < 1 || width > 32767 || height > 32767)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "packed frames: sides 1 .. 32767");
    if (nframes < 0 || stride < width || frame_pitch < 0 || payload_pitch < 0 || (nframes > 0 && (!d_payload || !d_out)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad packed frame batch descriptor");
    const int64_t rmin = raw_min_row_bytes(width, format);
    // (row_bytes bounded so that no product below leaves 64 bits; a real row is a few ten thousand bytes)
    if (row_bytes < rmin || row_bytes > ((int64_t)1 << 40))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "packed frames: row_bytes is at least mrgingham_amd_raw_row_bytes(width, format)");
    if ((payload_pitch & 15) || payload_pitch < (int64_t)(height - 1) * row_bytes + rmin || ((uintptr_t)d_payload & 15) || ((uintptr_t)d_out & 1))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "packed frames: 16-byte aligned, payload_pitch a multiple of 16 and at least (height-1)*row_bytes + the minimum row; frames 2-byte aligned");
    if (nframes == 0) return 0;
    if (nframes > 1 && frame_pitch > ((int64_t)1 << 40)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad packed frame batch descriptor");
    // what the launch reads and what it writes, as byte ranges
    const uintptr_t in0 = (uintptr_t)d_payload, in1 = in0 + (uintptr_t)nframes * (uintptr_t)payload_pitch;
    const uintptr_t out0 = (uintptr_t)d_out,
                    out1 = out0 + 2 * ((uintptr_t)(nframes - 1) * (uintptr_t)frame_pitch + (uintptr_t)(height - 1) * (uintptr_t)stride + (uintptr_t)width);
    if (in0 < out1 && out0 < in1) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "packed frames: input and output must not overlap");
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    return launch_raw_unpack(ctx, d_payload, payload_pitch, nframes, width, height, row_bytes, format, d_out, frame_pitch, stride,
                             (hipStream_t)stream);  // (the stream used as given: NULL is HIP's default stream)
}

}  // extern "C"
