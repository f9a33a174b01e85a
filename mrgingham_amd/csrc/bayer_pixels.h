// Bayer mosaics to grey, one text for the host entry (image_io.cpp: mrgingham_amd_bayer_grey_image) and the device
// kernel (bayer_grey.hip), like raw_pixels.h.  The definition is in include/mrgingham_amd.h: bilinear demosaicing and
// the fixed-point luma 4899 R + 9617 G + 1868 B folded into one rounding, borders by reflect-101.
//
// The four patterns are two facts.  Whether pixel (0,0) is green (GRBG, GBRG) or not (RGGB, BGGR), and which colour
// shares the green's rows: in row 0 red (RGGB, GRBG) or blue (GBRG, BGGR), in row 1 the other one.  So a site is
// described by `green` and by two coefficients: ca, that of the row's own colour (red or blue), and cb, that of the other.
//   green site:  (2 cG v + ca (W + E) + cb (N + S) + 16384) >> 15
//   other site:  (4 ca v + cG (N + S + W + E) + cb diag + 32768) >> 16
// Green alternates along a row and along a column, ca and cb change places from one row to the next.
//
// A WINDOW holds the NP + 2 samples x0 - 1 .. x0 + NP of one source row, NP = 16 / ES the samples of a 16-byte
// destination word: m[] the NP samples of the word as they lie in memory, lr the sample to the left (low half) and the
// one to the right (high half).  What a window holds of samples outside the row (after reflection) is its builder's
// business; bayer_word turns three windows into the NP destination samples, those outside the row unspecified.
#pragma once
#include <stdint.h>
#include <string.h>

#include "png_filter.h"

#if defined(__clang__)
#define MRG_BAYER_UNROLL _Pragma("unroll")
#else
#define MRG_BAYER_UNROLL
#endif

namespace mrg {

constexpr uint32_t kBayerR = 4899u, kBayerG = 9617u, kBayerB = 1868u;

MRG_PNG_HD bool bayer_pattern_ok(int pattern) { return pattern >= 0 && pattern <= 3; }
// pixel (0,0) is green: GRBG (1), GBRG (2)
MRG_PNG_HD bool bayer_green_first(int pattern) { return pattern == 1 || pattern == 2; }
// the coefficient of the colour in row 0 (RGGB, GRBG: red) and in row 1
MRG_PNG_HD uint32_t bayer_row_coef(int pattern, int row_parity) { return ((pattern < 2) == (row_parity == 0)) ? kBayerR : kBayerB; }

// BORDER_REFLECT_101 for one step outside 0 .. n - 1, n >= 2
MRG_PNG_HD int bayer_reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; }

template <int ES>
struct BayerWindow {
    uint32_t m[4], lr;
};

// sample i (0 .. NP + 1) of a window: x0 - 1 + i of the row (i a constant once the loops are unrolled)
template <int ES>
MRG_PNG_HD uint32_t bayer_sample(const BayerWindow<ES>& w, int i) {
    constexpr int NP = 16 / ES;
    if (i == 0) return w.lr & 0xFFFFu;
    if (i == NP + 1) return w.lr >> 16;
    const int k = i - 1;
    if constexpr (ES == 1) return (w.m[k >> 2] >> (8 * (k & 3))) & 255u;
    return (w.m[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
}

// one site: c the sample, h = W + E, v = N + S, d the four diagonals (unsigned 32-bit: the largest sum is
// 4 * 16384 * 65535 + 32768)
MRG_PNG_HD uint32_t bayer_site(bool green, uint32_t ca, uint32_t cb, uint32_t c, uint32_t h, uint32_t v, uint32_t d) {
    return green ? (2u * kBayerG * c + ca * h + cb * v + 16384u) >> 15 : (4u * ca * c + kBayerG * (h + v) + cb * d + 32768u) >> 16;
}

// The NP samples of a destination word from the windows of the rows above (n), at (c) and below (s) it.  G0: the first
// sample of the word is a green site; ca, cb: the coefficients of this row (see above).
template <int ES, bool G0>
MRG_PNG_HD void bayer_word(const BayerWindow<ES>& n, const BayerWindow<ES>& c, const BayerWindow<ES>& s, uint32_t ca, uint32_t cb, uint32_t out[4]) {
    static_assert(ES == 1 || ES == 2, "bytes of a sample");
    constexpr int NP = 16 / ES, PER = 4 / ES;
    // (both coefficients are below 2^13 and every sum below 2^19; said here so that the device compiler, which gets them as
    // kernel arguments, multiplies with v_mad_u32_u24 and not with the quarter-rate v_mul_lo_u32)
    ca &= 0x1FFFu, cb &= 0x1FFFu;
    uint32_t cc[NP + 2], vv[NP + 2];  // the row itself and the column sums N + S
    MRG_BAYER_UNROLL
    for (int i = 0; i < NP + 2; ++i) {
        cc[i] = bayer_sample<ES>(c, i);
        vv[i] = bayer_sample<ES>(n, i) + bayer_sample<ES>(s, i);
    }
    MRG_BAYER_UNROLL
    for (int q = 0; q < 4; ++q) {
        uint32_t d = 0;
        MRG_BAYER_UNROLL
        for (int p = 0; p < PER; ++p) {
            const int i = PER * q + p + 1;
            const bool green = G0 == (((i - 1) & 1) == 0);
            d |= bayer_site(green, ca, cb, cc[i], cc[i - 1] + cc[i + 1], vv[i], vv[i - 1] + vv[i + 1]) << (8 * ES * p);
        }
        out[q] = d;
    }
}

// A window built sample by sample, for the words at the ends of a row and for the host: sample x of the row is
// row[reflect(x)] for -1 <= x <= width; further out, where no destination sample inside the row depends on it, it is
// that of -1 or of width (a load without a condition).  On the host `row` may sit at any address: the samples are
// read bytewise there.
template <int ES>
MRG_PNG_HD uint32_t bayer_load(const uint8_t* row, int x) {
    if constexpr (ES == 1) return row[x];
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const uint16_t*)row)[x];  // (the device entry refuses an odd address)
#else
    return (uint32_t)row[2 * (long long)x] | ((uint32_t)row[2 * (long long)x + 1] << 8);  // native little-endian uint16
#endif
}
template <int ES>
MRG_PNG_HD BayerWindow<ES> bayer_window_edge(const uint8_t* row, int x0, int width) {
    constexpr int NP = 16 / ES;
    uint32_t s[NP + 2];
    MRG_BAYER_UNROLL
    for (int i = 0; i < NP + 2; ++i) {
        const int x = x0 - 1 + i;
        s[i] = bayer_load<ES>(row, bayer_reflect(x < -1 ? -1 : x > width ? width : x, width));
    }
    BayerWindow<ES> w;
    w.lr = s[0] | (s[NP + 1] << 16);
    MRG_BAYER_UNROLL
    for (int q = 0; q < 4; ++q) {
        uint32_t d = 0;
        MRG_BAYER_UNROLL
        for (int p = 0; p < 4 / ES; ++p) d |= s[1 + (4 / ES) * q + p] << (8 * ES * p);
        w.m[q] = d;
    }
    return w;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the window of a whole word inside the row (0 <= x0, x0 + NP <= width) on the host: its 16 bytes at once
template <int ES>
inline BayerWindow<ES> bayer_window_whole(const uint8_t* row, int x0, int width) {
    constexpr int NP = 16 / ES;
    BayerWindow<ES> w;
    memcpy(w.m, row + (long long)x0 * ES, 16);  // (little-endian hosts only, like the rest of the readers' fast paths)
    w.lr = bayer_load<ES>(row, bayer_reflect(x0 - 1, width)) | (bayer_load<ES>(row, bayer_reflect(x0 + NP, width)) << 16);
    return w;
}

// One frame on the host: rows at mosaic + y*stride and out + y*out_stride (ELEMENTS of ES bytes, any address); only
// the width x height outputs are written.  Arguments checked by the caller.
template <int ES>
inline void bayer_grey_rows(const uint8_t* mosaic, int width, int height, long long stride, int pattern, uint8_t* out, long long out_stride) {
    constexpr int NP = 16 / ES;
    const bool gf = bayer_green_first(pattern);
    for (int y = 0; y < height; ++y) {
        const uint8_t* rn = mosaic + (long long)bayer_reflect(y - 1, height) * stride * ES;
        const uint8_t* rc = mosaic + (long long)y * stride * ES;
        const uint8_t* rs = mosaic + (long long)bayer_reflect(y + 1, height) * stride * ES;
        const uint32_t ca = bayer_row_coef(pattern, y & 1), cb = bayer_row_coef(pattern, (y & 1) ^ 1);
        const bool g0 = gf == ((y & 1) == 0);  // words begin at even x
        for (int x0 = 0; x0 < width; x0 += NP) {
            const int k = width - x0 < NP ? width - x0 : NP;
            BayerWindow<ES> wn, wc, ws;
            if (k == NP) {
                wn = bayer_window_whole<ES>(rn, x0, width), wc = bayer_window_whole<ES>(rc, x0, width), ws = bayer_window_whole<ES>(rs, x0, width);
            } else {
                wn = bayer_window_edge<ES>(rn, x0, width), wc = bayer_window_edge<ES>(rc, x0, width), ws = bayer_window_edge<ES>(rs, x0, width);
            }
            uint32_t d[4];
            if (g0)
                bayer_word<ES, true>(wn, wc, ws, ca, cb, d);
            else
                bayer_word<ES, false>(wn, wc, ws, ca, cb, d);
            memcpy(out + ((long long)y * out_stride + x0) * ES, d, (size_t)k * ES);
        }
    }
}
#endif

}  // namespace mrg
