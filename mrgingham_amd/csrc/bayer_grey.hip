// Bayer mosaics on the device: uint8 or uint16 frames whose samples are a colour filter mosaic (RGGB, GRBG, GBRG, BGGR) to
// grey frames of the same type, one streaming 3x3 stencil launch.  The arithmetic is bayer_pixels.h, the text the host
// entry (image_io.cpp: mrgingham_amd_bayer_grey_image) runs.  See include/mrgingham_amd.h for the definition and the
// contract of the entry points, DESIGN.md section 4.22 for the byte model and the numbers.
//
// THE SCHEDULE (box_blur3_kernel's, decimate.hip, for any width, stride and address).  A lane owns one column of 16-byte
// destination words -- the NP = 16 / ES samples from x0 = xbase + NP * (its index along the row) -- and rolls down a slab of
// kBayerSlabRows rows with the windows of three source rows in registers: every source row is loaded once per slab (and the
// two rows around a slab once more), every destination row leaves as one 16-byte store.  xbase (-NP < xbase <= 0) is
// chosen by the launch so that the words of frame 0, row 0 are 16-byte aligned; where the strides are multiples of 16
// bytes that holds for every row, and in any other row the lane finds its address unaligned and stores sample by sample,
// as the words that hang over an end of the row always do.  NP is even, so x0 has the parity of xbase in every lane: with
// the row loop unrolled by two, which sites of a word are green is a template argument.  Rows are counted inside their
// frame (a slab never crosses one), so the parity of a row is that of its y.
#include "bayer_pixels.h"
#include "ctx.h"
#include "pnm_pixels.h"

using namespace mrg;

namespace {

constexpr int kBayerLanes = 256;    // of a workgroup, side by side along a row
constexpr int kBayerSlabRows = 32;  // even: a slab begins at an even row

// The window of the samples x0 - 1 .. x0 + NP of a row.  whole (0 <= x0, x0 + NP <= width): the word as one 16-byte load
// where it is aligned, else as the aligned dwords that hold it behind a funnel shift (pnm_pixels.h), and the two samples
// beside it by narrow loads of their own, reflected at the ends of the row.  Not whole: sample by sample.
template <int ES>
__device__ __forceinline__ BayerWindow<ES> bayer_window(const uint8_t* __restrict__ row, int x0, int width, bool whole) {
    constexpr int NP = 16 / ES;
    if (!whole) return bayer_window_edge<ES>(row, x0, width);
    BayerWindow<ES> w;
    w.lr = bayer_load<ES>(row, x0 > 0 ? x0 - 1 : 1) | (bayer_load<ES>(row, x0 + NP < width ? x0 + NP : width - 2) << 16);
    const uint8_t* p = row + (long long)x0 * ES;
    const int off = (int)((uintptr_t)p & 15);
    if (off == 0) {
        const uint4 g = *reinterpret_cast<const uint4*>(p);
        w.m[0] = g.x, w.m[1] = g.y, w.m[2] = g.z, w.m[3] = g.w;
    } else {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p - (off & 3));
        const int r = 8 * (off & 3);
        uint32_t d[5];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = q[i];
        d[4] = r ? q[4] : 0u;  // (with r == 0 the fifth dword holds nothing of the word and may lie behind the frame)
#pragma unroll
        for (int i = 0; i < 4; ++i) w.m[i] = pnm_funnel(d[i], d[i + 1], r);
    }
    return w;
}

template <int ES, bool G0>
__device__ __forceinline__ void bayer_emit(const BayerWindow<ES>& n, const BayerWindow<ES>& c, const BayerWindow<ES>& s, uint32_t ca, uint32_t cb,
                                           uint8_t* __restrict__ dst_row, int x0, int width, bool whole) {
    constexpr int NP = 16 / ES;
    uint32_t d[4];
    bayer_word<ES, G0>(n, c, s, ca, cb, d);
    uint8_t* o = dst_row + (long long)x0 * ES;  // (not dereferenced where x0 + p lies outside the row)
    if (whole && ((uintptr_t)o & 15) == 0) {
        *reinterpret_cast<uint4*>(o) = make_uint4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
        for (int p = 0; p < NP; ++p)
            if (x0 + p >= 0 && x0 + p < width) {
                if constexpr (ES == 2)
                    reinterpret_cast<uint16_t*>(o)[p] = (uint16_t)(d[p >> 1] >> (16 * (p & 1)));
                else
                    o[p] = (uint8_t)(d[p >> 2] >> (8 * (p & 3)));
            }
    }
}

// A lane's column of words down its slab, in every frame the lane takes.  G0E: the first sample of a word is a green
// site in the even rows of a frame; c0, c1: the coefficients of the colour that shares the even and the odd rows with
// green (bayer_pixels.h).  Pitches and strides in bytes.  WHOLE: the word lies inside the row.
template <int ES, bool G0E, bool WHOLE>
__device__ __forceinline__ void bayer_slab(const uint8_t* __restrict__ in, long long in_pitch, long long in_stride, int nframes, int width, int height,
                                           uint8_t* __restrict__ out, long long out_pitch, long long out_stride, int x0, int y0, int y1, uint32_t c0,
                                           uint32_t c1) {
    for (int f = (int)blockIdx.z; f < nframes; f += (int)gridDim.z) {
        const uint8_t* __restrict__ src = in + (long long)f * in_pitch;
        uint8_t* __restrict__ dst = out + (long long)f * out_pitch;
        auto window = [&](int y) { return bayer_window<ES>(src + (long long)bayer_reflect(y, height) * in_stride, x0, width, WHOLE); };
        BayerWindow<ES> a = window(y0 - 1), b = window(y0);
        for (int y = y0; y < y1; y += 2) {  // y is even
            const BayerWindow<ES> c = window(y + 1);
            bayer_emit<ES, G0E>(a, b, c, c0, c1, dst + (long long)y * out_stride, x0, width, WHOLE);
            if (y + 1 < y1) {
                a = window(y + 2);
                bayer_emit<ES, !G0E>(b, c, a, c1, c0, dst + (long long)(y + 1) * out_stride, x0, width, WHOLE);
                b = a;
                a = c;
            }
        }
    }
}

template <int ES, bool G0E>
__global__ __launch_bounds__(kBayerLanes) void bayer_grey_kernel(const uint8_t* __restrict__ in, long long in_pitch, long long in_stride, int nframes,
                                                                 int width, int height, uint8_t* __restrict__ out, long long out_pitch,
                                                                 long long out_stride, int xbase, uint32_t c0, uint32_t c1) {
    constexpr int NP = 16 / ES;
    const int x0 = xbase + ((int)blockIdx.x * kBayerLanes + (int)threadIdx.x) * NP;
    const int y0 = (int)blockIdx.y * kBayerSlabRows, y1 = min(y0 + kBayerSlabRows, height);
    if (x0 >= width) return;
    if (x0 >= 0 && x0 + NP <= width)
        bayer_slab<ES, G0E, true>(in, in_pitch, in_stride, nframes, width, height, out, out_pitch, out_stride, x0, y0, y1, c0, c1);
    else  // (at most two lanes of a row)
        bayer_slab<ES, G0E, false>(in, in_pitch, in_stride, nframes, width, height, out, out_pitch, out_stride, x0, y0, y1, c0, c1);
}

}  // namespace

extern "C" {

void mrgingham_amd_bayer_grey_geometry(int* lanes_per_workgroup, int* rows_per_slab, int* max_workgroups_per_cu) {
    if (lanes_per_workgroup) *lanes_per_workgroup = kBayerLanes;
    if (rows_per_slab) *rows_per_slab = kBayerSlabRows;
    if (max_workgroups_per_cu) *max_workgroups_per_cu = 0;  // the grid is not capped: one workgroup per slab and span of a row
}

int mrgingham_amd_bayer_grey_batch(mrgingham_amd_ctx* ctx, const void* d_in, int bits, int nframes, int width, int height, int64_t in_frame_pitch,
                                   int64_t in_stride, int pattern, void* d_out, int64_t out_frame_pitch, int64_t out_stride, void* stream) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (!bayer_pattern_ok(pattern)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bayer mosaics: pattern is one of MRGINGHAM_AMD_BAYER_RGGB, _GRBG, _GBRG, _BGGR");
    if (bits != 8 && bits != 16) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bayer mosaics: 8 or 16 bits");
    if (width < 2 || height < 2 || width > 32767 || height > 32767) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bayer mosaics: sides 2 .. 32767");
    const int es = bits / 8;
    const int64_t big = (int64_t)1 << 40, extent_in = (int64_t)(height - 1) * in_stride + width, extent_out = (int64_t)(height - 1) * out_stride + width;
    if (nframes < 0 || in_stride < width || out_stride < width || in_stride > big || out_stride > big || in_frame_pitch < 0 || out_frame_pitch < 0 ||
        (nframes > 1 && (in_frame_pitch > big || out_frame_pitch > big || out_frame_pitch < extent_out)) || (nframes > 0 && (!d_in || !d_out)) ||
        (((uintptr_t)d_in | (uintptr_t)d_out) & (uintptr_t)(es - 1)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad bayer mosaic batch descriptor");
    if (nframes == 0) return 0;
    // what the launch reads and what it writes, as byte ranges
    const uintptr_t in0 = (uintptr_t)d_in, in1 = in0 + (uintptr_t)es * ((uintptr_t)(nframes - 1) * (uintptr_t)in_frame_pitch + (uintptr_t)extent_in);
    const uintptr_t out0 = (uintptr_t)d_out, out1 = out0 + (uintptr_t)es * ((uintptr_t)(nframes - 1) * (uintptr_t)out_frame_pitch + (uintptr_t)extent_out);
    if (in0 < out1 && out0 < in1) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bayer mosaics: input and output must not overlap");
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    // the first whole word of frame 0, row 0 begins `head` samples into the row
    const int np = 16 / es, head = (int)((16 - (out0 & 15)) & 15) / es, xbase = head ? head - np : 0;
    const int words = (width - xbase + np - 1) / np;
    const dim3 grid((unsigned)((words + kBayerLanes - 1) / kBayerLanes), (unsigned)((height + kBayerSlabRows - 1) / kBayerSlabRows),
                    (unsigned)(nframes < 65535 ? nframes : 65535));
    const bool g0e = bayer_green_first(pattern) == ((xbase & 1) == 0);
    const uint32_t c0 = bayer_row_coef(pattern, 0), c1 = bayer_row_coef(pattern, 1);
#define MRG_BAYER_LAUNCH(ES, G)                                                                                                              \
    hipLaunchKernelGGL((bayer_grey_kernel<ES, G>), grid, dim3(kBayerLanes), 0, (hipStream_t)stream, (const uint8_t*)d_in,                    \
                       (long long)in_frame_pitch * ES, (long long)in_stride * ES, nframes, width, height, (uint8_t*)d_out,                   \
                       (long long)out_frame_pitch * ES, (long long)out_stride * ES, xbase, c0, c1)
    if (es == 1) {
        if (g0e) MRG_BAYER_LAUNCH(1, true); else MRG_BAYER_LAUNCH(1, false);
    } else {
        if (g0e) MRG_BAYER_LAUNCH(2, true); else MRG_BAYER_LAUNCH(2, false);
    }
#undef MRG_BAYER_LAUNCH
    MRG_HIP_CHECK(hipGetLastError());  // (the stream used as given: NULL is HIP's default stream)
    return 0;
}

}  // extern "C"
