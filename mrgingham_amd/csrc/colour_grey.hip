// Colour frames on the device: interleaved RGB / BGR (3 or 4 samples per pixel), planar RGB / BGR and packed YUV 4:2:2,
// uint8 or native uint16, to grey frames of the same type, one streaming launch.  The pixels themselves are
// colour_pixels.h, the text the host entry (image_io.cpp: mrgingham_amd_colour_grey_image) runs; the schedule is
// unpack_rows.h.  See include/mrgingham_amd.h for the definition and the contract of the entry points, DESIGN.md section
// 4.24 for the byte model and the numbers.
#include "ctx.h"  // (first: colour_pixels.h uses the runtime's uint4 in its device half)

#include "colour_pixels.h"
#include "unpack_rows.h"

using namespace mrg;

namespace {

// a row of a frame view: it begins at any byte (any even byte at 16 bit), f * frame_pitch + y * stride behind `in`, 64-bit
// products both; the pixel text gets it as a 16-byte aligned base and the row's phase behind it, so that every dword it
// loads is an aligned one
template <int ES, int LAYOUT>
struct ColourRows {
    const uint8_t* __restrict__ in;
    long long frame_pitch_b, plane_pitch_b, stride_b;
    uint32_t ca, cb;
    int ybyte;
    struct Row {
        ColourRow<LAYOUT> r;
        uint32_t ca, cb;
        int ybyte;
        __device__ __forceinline__ void pixels(int x0, int n, uint32_t d[4]) const { colour_pixels<ES, LAYOUT>(r, ca, cb, ybyte, x0, n, d); }
    };
    __device__ __forceinline__ Row row(long long f, int y) const {
        Row w;
        const uint8_t* a = in + f * frame_pitch_b + (long long)y * stride_b;
#pragma unroll
        for (int k = 0; k < ColourRow<LAYOUT>::kPlanes; ++k) {
            const uint8_t* p = a + k * plane_pitch_b;
            const long long ph = (long long)((uintptr_t)p & 15);
            w.r.base[k] = p - ph, w.r.off[k] = ph;
        }
        w.r.limit = 0;  // (the device's pnm_dword does not look at it)
        w.ca = ca, w.cb = cb, w.ybyte = ybyte;
        return w;
    }
};

// unpack_rows.h has the schedule; pitches and strides in bytes
template <int ES, int LAYOUT>
__global__ __launch_bounds__(kUnpackLanes) void colour_grey_kernel(const uint8_t* __restrict__ in, long long in_pitch_b, long long plane_pitch_b,
                                                                   long long in_stride_b, uint32_t ca, uint32_t cb, int ybyte, int width, int height,
                                                                   long long nrows, uint8_t* __restrict__ out, long long out_pitch_b,
                                                                   long long out_stride_b, int lpr_shift) {
    unpack_rows<ES>(ColourRows<ES, LAYOUT>{in, in_pitch_b, plane_pitch_b, in_stride_b, ca, cb, ybyte}, width, height, nrows, out, out_pitch_b,
                    out_stride_b, lpr_shift);
}

}  // namespace

extern "C" {

void mrgingham_amd_colour_grey_geometry(int* lanes_per_workgroup, int* max_workgroups_per_cu) {
    if (lanes_per_workgroup) *lanes_per_workgroup = kUnpackLanes;
    if (max_workgroups_per_cu) *max_workgroups_per_cu = kUnpackWorkgroupsPerCu;
}

int mrgingham_amd_colour_grey_batch(mrgingham_amd_ctx* ctx, const void* d_in, int bits, int format, int nframes, int width, int height,
                                    int64_t in_frame_pitch, int64_t in_plane_pitch, int64_t in_stride, void* d_out, int64_t out_frame_pitch,
                                    int64_t out_stride, void* stream) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (bits != 8 && bits != 16) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "colour frames: 8 or 16 bits");
    if (!colour_format_ok(format, bits))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "colour frames: format is one of MRGINGHAM_AMD_COLOUR_RGB .. _UYVY, the 4:2:2 forms at 8 bits only");
    if (width < 1 || height < 1 || width > 32767 || height > 32767) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "colour frames: sides 1 .. 32767");
    const int es = bits / 8, layout = colour_layout(format);
    const int64_t big = (int64_t)1 << 40, plane_pitch = layout == kColourPlanar ? in_plane_pitch : 0;
    if (nframes < 0 || in_stride < (int64_t)colour_row_samples(layout) * width || out_stride < width || in_stride > big || out_stride > big ||
        plane_pitch < 0 || plane_pitch > big || in_frame_pitch < 0 || out_frame_pitch < 0 || (nframes > 0 && (!d_in || !d_out)) ||
        (((uintptr_t)d_in | (uintptr_t)d_out) & (uintptr_t)(es - 1)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad colour frame batch descriptor");
    const int64_t extent_in = colour_extent(layout, width, height, in_stride, plane_pitch), extent_out = (int64_t)(height - 1) * out_stride + width;
    if (nframes > 1 && (in_frame_pitch > big || out_frame_pitch > big || out_frame_pitch < extent_out))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "colour frames: the frames of the output must not overlap each other");
    if (nframes == 0) return 0;
    // what the launch reads and what it writes, as byte ranges
    const uintptr_t in0 = (uintptr_t)d_in, in1 = in0 + (uintptr_t)es * ((uintptr_t)(nframes - 1) * (uintptr_t)in_frame_pitch + (uintptr_t)extent_in);
    const uintptr_t out0 = (uintptr_t)d_out, out1 = out0 + (uintptr_t)es * ((uintptr_t)(nframes - 1) * (uintptr_t)out_frame_pitch + (uintptr_t)extent_out);
    if (in0 < out1 && out0 < in1) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "colour frames: input and output must not overlap");
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    const long long nrows = (long long)nframes * height;
    UnpackShape sh;
    if (int rc = unpack_launch_shape(ctx, d_out, (long long)out_frame_pitch * es, (long long)out_stride * es, (long long)width * es, nrows, &sh)) return rc;
#define MRG_COLOUR_LAUNCH(ES, L)                                                                                                                  \
    hipLaunchKernelGGL((colour_grey_kernel<ES, L>), dim3((unsigned)sh.blocks), dim3(kUnpackLanes), 0, (hipStream_t)stream, (const uint8_t*)d_in, \
                       (long long)in_frame_pitch * ES, (long long)plane_pitch * ES, (long long)in_stride * ES, colour_coef_first(format),         \
                       colour_coef_third(format), colour_y_byte(format), width, height, nrows, (uint8_t*)d_out, (long long)out_frame_pitch * ES,  \
                       (long long)out_stride * ES, sh.lpr_shift)
    if (es == 1) {
        switch (layout) {
            case kColourPacked3: MRG_COLOUR_LAUNCH(1, kColourPacked3); break;
            case kColourPacked4: MRG_COLOUR_LAUNCH(1, kColourPacked4); break;
            case kColourPlanar: MRG_COLOUR_LAUNCH(1, kColourPlanar); break;
            default: MRG_COLOUR_LAUNCH(1, kColour422); break;
        }
    } else {
        switch (layout) {
            case kColourPacked3: MRG_COLOUR_LAUNCH(2, kColourPacked3); break;
            case kColourPacked4: MRG_COLOUR_LAUNCH(2, kColourPacked4); break;
            default: MRG_COLOUR_LAUNCH(2, kColourPlanar); break;
        }
    }
#undef MRG_COLOUR_LAUNCH
    MRG_HIP_CHECK(hipGetLastError());  // (the stream used as given: NULL is HIP's default stream)
    return 0;
}

}  // extern "C"
