// Packed camera frames on the device: rows of 10 / 12 / 14-bit samples as a camera or a frame grabber delivers them --
// an LSB-first bit stream (Mono10p, Mono12p, Mono14p) or 3-byte pixel pairs (Mono10Packed, Mono12Packed), rows of
// row_bytes bytes -- to native uint16 frames with a row stride.  The samples themselves are raw_pixels.h, the text the host
// entry (image_io.cpp: mrgingham_amd_raw_unpack_image) runs.  See include/mrgingham_amd.h for the contract of the entry
// points and DESIGN.md section 4.20 for the byte model and the numbers.
#include "ctx.h"
#include "raw_pixels.h"

using namespace mrg;

namespace {

constexpr int kLanes = 256;
constexpr int kWorkgroupsPerCu = 8;  // eight workgroups of 256 lanes fill a CU

// pnm_unpack_kernel's schedule: a grid-stride loop over the rows of all frames; a row is taken by 2^lpr_shift lanes of a
// workgroup (256 >> lpr_shift rows side by side), lane l by the words l, l + lanes, ... of the DESTINATION row: consecutive
// lanes store consecutive 16-byte words.  Word k of a row whose destination begins `ph` bytes behind a 16-byte boundary
// holds the samples [(16k - ph) / 2, (16k - ph) / 2 + 8) that lie inside the row; a whole word is one 16-byte store (its
// address is a multiple of 16 by construction), the head and the tail of a row go out sample by sample.  The source row
// begins at byte y * rowb of the frame's payload, at any phase; word k begins at any bit (streams) or at either sample of
// a pair.
template <int FMT>
__global__ __launch_bounds__(kLanes) void raw_unpack_kernel(const uint8_t* __restrict__ payload, long long payload_pitch, long long rowb, int width,
                                                            int height, long long nrows, uint8_t* __restrict__ out,
                                                            long long frame_pitch_b, long long stride_b, int lpr_shift) {
    const int lanes = 1 << lpr_shift, l = (int)threadIdx.x & (lanes - 1), sub = (int)threadIdx.x >> lpr_shift;
    const long long rows_per_step = (long long)gridDim.x * (kLanes >> lpr_shift);
    for (long long row = (long long)blockIdx.x * (kLanes >> lpr_shift) + sub; row < nrows; row += rows_per_step) {
        const long long f = row / height;
        const int y = (int)(row - f * height);
        const uint8_t* base = payload + f * payload_pitch;
        const long long row_off = (long long)y * rowb;
        uint8_t* dst = out + f * frame_pitch_b + (long long)y * stride_b;
        const int ph = (int)((uintptr_t)dst & 15);  // (even)
        const int K = (ph + width * 2 + 15) >> 4;
        for (int k = l; k < K; k += lanes) {
            int x0 = (16 * k - ph) / 2, hi = x0 + 8;  // (16k - ph < 0 only with k == 0: x0 becomes 0 either way)
            if (x0 < 0) x0 = 0;
            if (hi > width) hi = width;
            const int n = hi - x0;
            uint32_t d[4];
            raw_pixels<FMT>(base, payload_pitch, row_off, x0, n, d);
            uint16_t* o = (uint16_t*)dst + x0;
            if (n == 8) {
                *(uint4*)o = make_uint4(d[0], d[1], d[2], d[3]);
            } else {
#pragma unroll
                for (int p = 0; p < 7; ++p)
                    if (p < n) o[p] = (uint16_t)(d[p >> 1] >> (16 * (p & 1)));
            }
        }
    }
}

// checked arguments -> the launch (frame_pitch and stride in samples)
int launch_raw_unpack(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, int nframes, int width, int height, int64_t row_bytes,
                      int format, uint16_t* d_out, int64_t frame_pitch, int stride, hipStream_t s) {
    const long long nrows = (long long)nframes * height;
    // the lanes of a row: the power of two that covers its words (one more where a row can begin inside a word)
    const bool aligned = !((uintptr_t)d_out & 15) && !((frame_pitch * 2) & 15) && !(((long long)stride * 2) & 15);
    const int kmax = (width * 2 + 15) / 16 + (aligned ? 0 : 1);
    int lpr_shift = 0;
    while ((1 << lpr_shift) < kmax && (1 << lpr_shift) < kLanes) ++lpr_shift;
    const int rows_per_block = kLanes >> lpr_shift;
    int cus = 0;
    MRG_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    long long blocks = (nrows + rows_per_block - 1) / rows_per_block;  // sized to the device
    if (blocks > (long long)cus * kWorkgroupsPerCu) blocks = (long long)cus * kWorkgroupsPerCu;
#define MRG_RAW_LAUNCH(F)                                                                                                                    \
    case F:                                                                                                                                  \
        hipLaunchKernelGGL((raw_unpack_kernel<F>), dim3((unsigned)blocks), dim3(kLanes), 0, s, d_payload, (long long)payload_pitch,          \
                           (long long)row_bytes, width, height, nrows, (uint8_t*)d_out, (long long)frame_pitch * 2, (long long)stride * 2,   \
                           lpr_shift);                                                                                                       \
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
    if (lanes_per_workgroup) *lanes_per_workgroup = kLanes;
    if (max_workgroups_per_cu) *max_workgroups_per_cu = kWorkgroupsPerCu;
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
