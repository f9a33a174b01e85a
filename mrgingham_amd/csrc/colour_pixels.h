// Colour frames to grey, one text for the host entry (image_io.cpp: mrgingham_amd_colour_grey_image) and the device kernel
// (colour_grey.hip), like bayer_pixels.h.  The definition is in include/mrgingham_amd.h at MRGINGHAM_AMD_COLOUR_RGB:
// interleaved RGB / BGR with 3 or 4 samples per pixel, three planes, or packed YUV 4:2:2, uint8 or native uint16, to grey
// samples of the same type.
//
// The eight formats are four LAYOUTS and two facts.  The layout says where the samples of a pixel lie (3 or 4 side by
// side, three planes, or the Y byte of a 2-byte pixel) and is a template argument.  Which of the outer samples is red is
// two coefficients that change places, ca for the first sample and cb for the third, as in bayer_pixels.h:
//   grey = (ca * s0 + 9617 * s1 + cb * s2 + 8192) >> 14,   (ca, cb) = (4899, 1868) for R G B, (1868, 4899) for B G R
// which is png_grey (png_filter.h) of the three samples in the order R, G, B; tests/test_colour.py holds the two together
// through the PNG and PAM readers.  Where the Y byte of a 4:2:2 pixel lies (0: YUYV, 1: UYVY) is an addend to the byte at
// which the lane's source bytes begin, which is a run-time value anyway: it costs no instruction.
//
// colour_pixels gives the grey samples of the pixels [x0, x0 + n) of a row packed into four dwords as the *_pixels.h texts
// pack them: n <= 16 bytes at ES 1 (pixel x0 + p is byte p & 3 of out[p >> 2]), n <= 8 halves at ES 2 (pixel x0 + p is
// half p & 1 of out[p >> 1]); what lies beyond n is unspecified.
//
// What it reads (colour_stream): the aligned dwords that hold the first to the last source byte of those pixels, each
// once -- as 16-byte loads where all of them are needed and the first is 16-byte aligned (device), else one by one
// (pnm_dword), behind a funnel shift by the first byte's place in its dword (pnm_funnel).  They hold samples of the frames,
// so nothing outside the frames' dwords is read.  The host loads the same dwords with memcpy from any address and takes of
// the last one only the bytes inside `limit`.
#pragma once
#include <stdint.h>
#include <string.h>

#include "bayer_pixels.h"  // kBayerR, kBayerG, kBayerB: the weights of png_grey by name
#include "png_filter.h"
#include "pnm_pixels.h"

namespace mrg {

// MRGINGHAM_AMD_COLOUR_*: RGB 0, BGR 1, RGBA 2, BGRA 3, RGB_PLANAR 4, BGR_PLANAR 5, YUYV 6, UYVY 7
constexpr int kColourPacked3 = 0, kColourPacked4 = 1, kColourPlanar = 2, kColour422 = 3;

MRG_PNG_HD bool colour_format_ok(int format, int bits) { return format >= 0 && format <= 7 && (bits == 8 || (bits == 16 && format <= 5)); }
MRG_PNG_HD int colour_layout(int format) { return format >> 1; }
// the samples a pixel takes of its row (planar: of one plane's row)
MRG_PNG_HD int colour_row_samples(int layout) { return layout == kColourPacked3 ? 3 : layout == kColourPacked4 ? 4 : layout == kColourPlanar ? 1 : 2; }
// the coefficients of the first and the third sample
MRG_PNG_HD uint32_t colour_coef_first(int format) { return (format & 1) ? kBayerB : kBayerR; }
MRG_PNG_HD uint32_t colour_coef_third(int format) { return (format & 1) ? kBayerR : kBayerB; }
// the byte of a 4:2:2 pixel that holds Y
MRG_PNG_HD int colour_y_byte(int format) { return format == 7 ? 1 : 0; }
// the ELEMENTS from the first sample of a frame to behind its last one
MRG_PNG_HD long long colour_extent(int layout, int width, int height, long long stride, long long plane_pitch) {
    return (long long)(height - 1) * stride + (long long)colour_row_samples(layout) * width + (layout == kColourPlanar ? 2 * plane_pitch : 0);
}

// A row: plane k (one plane unless the layout is planar) begins off[k] bytes behind base[k]; `limit`: the bytes behind a
// base that may be read (host; there every base is the image).  On the device a base is a multiple of 16.
template <int LAYOUT>
struct ColourRow {
    static constexpr int kPlanes = LAYOUT == kColourPlanar ? 3 : 1;
    const uint8_t* base[kPlanes];
    long long off[kPlanes];
    long long limit;
};

// v[]: the NB source bytes from byte `first` behind base on, of which the first nbytes (1 .. NB) are needed and looked at;
// whole: nbytes >= NB - 1, every dword that holds some of the NB bytes is needed
template <int NB>
MRG_PNG_HD void colour_stream(const uint8_t* base, long long limit, long long first, int nbytes, bool whole, uint32_t v[NB / 4]) {
    static_assert(NB % 16 == 0, "whole 16-byte words");
    constexpr int NV = NB / 4;
    const long long d0 = first >> 2;
    const int nd = (int)(((first + nbytes - 1) >> 2) - d0) + 1;  // 1 .. NV + 1
    const int r = 8 * (int)(first & 3);
    uint32_t w[NV + 1];
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t* q = (const uint32_t*)base + d0;
    if (whole && ((uintptr_t)q & 15) == 0) {
        MRG_PNM_UNROLL
        for (int i = 0; i < NV / 4; ++i) {
            const uint4 g = ((const uint4*)q)[i];
            w[4 * i] = g.x, w[4 * i + 1] = g.y, w[4 * i + 2] = g.z, w[4 * i + 3] = g.w;
        }
        w[NV] = nd > NV ? q[NV] : 0u;
    } else
#endif
    {
        (void)whole;
        MRG_PNM_UNROLL
        for (int i = 0; i < NV + 1; ++i) w[i] = i < nd ? pnm_dword(base, d0, i, limit) : 0u;
    }
    MRG_PNM_UNROLL
    for (int i = 0; i < NV; ++i) v[i] = pnm_funnel(w[i], w[i + 1], r);
}

// sample k of a stream of native samples of ES bytes held in v[] from byte 0 on (k a constant once the loops are unrolled)
template <int ES>
MRG_PNG_HD uint32_t colour_sample(const uint32_t* v, int k) {
    if constexpr (ES == 1) return (v[k >> 2] >> (8 * (k & 3))) & 255u;
    return (v[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
}

// (the coefficients are below 2^14 and the samples below 2^16; said where the device compiler sees it, so that it multiplies
// with v_mad_u32_u24)
MRG_PNG_HD uint32_t colour_luma(uint32_t ca, uint32_t cb, uint32_t s0, uint32_t s1, uint32_t s2) {
    return ((ca & 0x3FFFu) * s0 + kBayerG * s1 + (cb & 0x3FFFu) * s2 + 8192u) >> 14;
}

template <int ES, int LAYOUT>
MRG_PNG_HD void colour_pixels(const ColourRow<LAYOUT>& row, uint32_t ca, uint32_t cb, int ybyte, int x0, int n, uint32_t out[4]) {
    static_assert(ES == 1 || ES == 2, "bytes of a sample");
    static_assert(LAYOUT >= kColourPacked3 && LAYOUT <= kColour422 && (LAYOUT != kColour422 || ES == 1), "4:2:2 is 8 bit");
    constexpr int NP = 16 / ES, PER = 4 / ES;
    const bool whole = n == NP;
    if constexpr (LAYOUT == kColour422) {
        // Y of pixel x at byte 2x + ybyte: from the first Y to the last one, 2n - 1 bytes, of which every second is taken
        uint32_t v[8];
        colour_stream<32>(row.base[0], row.limit, row.off[0] + 2ll * x0 + ybyte, 2 * n - 1, whole, v);
        MRG_PNM_UNROLL
        for (int q = 0; q < 4; ++q)
            out[q] = (v[2 * q] & 255u) | ((v[2 * q] >> 8) & 0xFF00u) | ((v[2 * q + 1] & 255u) << 16) | ((v[2 * q + 1] << 8) & 0xFF000000u);
    } else if constexpr (LAYOUT == kColourPlanar) {
        (void)ybyte;
        uint32_t v[3][4];
        MRG_PNM_UNROLL
        for (int k = 0; k < 3; ++k) colour_stream<16>(row.base[k], row.limit, row.off[k] + (long long)x0 * ES, n * ES, whole, v[k]);
        MRG_PNM_UNROLL
        for (int q = 0; q < 4; ++q) {
            uint32_t d = 0;
            MRG_PNM_UNROLL
            for (int p = 0; p < PER; ++p) {
                const int px = PER * q + p;
                d |= colour_luma(ca, cb, colour_sample<ES>(v[0], px), colour_sample<ES>(v[1], px), colour_sample<ES>(v[2], px)) << (8 * ES * p);
            }
            out[q] = d;
        }
    } else {
        (void)ybyte;
        constexpr int CH = LAYOUT == kColourPacked3 ? 3 : 4, NB = NP * CH * ES;
        uint32_t v[NB / 4];
        colour_stream<NB>(row.base[0], row.limit, row.off[0] + (long long)x0 * CH * ES, n * CH * ES, whole, v);
        MRG_PNM_UNROLL
        for (int q = 0; q < 4; ++q) {
            uint32_t d = 0;
            MRG_PNM_UNROLL
            for (int p = 0; p < PER; ++p) {
                const int px = PER * q + p;
                d |= colour_luma(ca, cb, colour_sample<ES>(v, CH * px), colour_sample<ES>(v, CH * px + 1), colour_sample<ES>(v, CH * px + 2)) << (8 * ES * p);
            }
            out[q] = d;
        }
    }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One frame on the host: rows at image + y*stride and out + y*out_stride (ELEMENTS of ES bytes, any address), the planes
// of a planar frame plane_pitch elements apart; only the width x height outputs are written.  Arguments checked by the
// caller.
template <int ES, int LAYOUT>
inline void colour_grey_rows(const uint8_t* image, int format, int width, int height, long long stride, long long plane_pitch, uint8_t* out,
                             long long out_stride) {
    constexpr int NP = 16 / ES;
    const uint32_t ca = colour_coef_first(format), cb = colour_coef_third(format);
    const int ybyte = colour_y_byte(format);
    ColourRow<LAYOUT> row;
    row.limit = colour_extent(LAYOUT, width, height, stride, plane_pitch) * ES;
    for (int y = 0; y < height; ++y) {
        for (int k = 0; k < ColourRow<LAYOUT>::kPlanes; ++k) row.base[k] = image, row.off[k] = ((long long)y * stride + k * plane_pitch) * ES;
        for (int x0 = 0; x0 < width; x0 += NP) {
            const int n = width - x0 < NP ? width - x0 : NP;
            uint32_t d[4];
            colour_pixels<ES, LAYOUT>(row, ca, cb, ybyte, x0, n, d);
            memcpy(out + ((long long)y * out_stride + x0) * ES, d, (size_t)n * ES);  // (little-endian hosts only, like the rest of the readers' fast paths)
        }
    }
}

// the same by a sample width and a format known at run time (colour_format_ok holds)
inline void colour_grey_rows_any(const uint8_t* image, int bits, int format, int width, int height, long long stride, long long plane_pitch,
                                 uint8_t* out, long long out_stride) {
#define MRG_COLOUR_CASE(ES, L)                                                                            \
    if (bits == 8 * ES && colour_layout(format) == L)                                                      \
        return colour_grey_rows<ES, L>(image, format, width, height, stride, plane_pitch, out, out_stride);
    MRG_COLOUR_CASE(1, kColourPacked3) MRG_COLOUR_CASE(1, kColourPacked4) MRG_COLOUR_CASE(1, kColourPlanar) MRG_COLOUR_CASE(1, kColour422)
    MRG_COLOUR_CASE(2, kColourPacked3) MRG_COLOUR_CASE(2, kColourPacked4) MRG_COLOUR_CASE(2, kColourPlanar)
#undef MRG_COLOUR_CASE
}
#endif

}  // namespace mrg
