// The pixels of one row of a Windows Bitmap to grey, one text for the host decoder (image_io.cpp: decode_bmp) and the
// device kernel (bmp_unpack.hip), like png_filter.h and tiff_lzw.h.  A source row is rowb = ((width*bits + 31) / 32) * 4
// bytes as they lie in the file: palette indices of 1, 4 or 8 bits (the leftmost pixel in the most significant bits of a
// byte), B G R triples, or B G R X quadruples.  bmp_pixels gives the grey bytes of the pixels [x0, x0 + n), n <= 16, packed
// into four dwords (pixel x0 + p is byte p & 3 of out[p >> 2]); the bytes beyond n are unspecified.  rowb is the row's padded
// length.
//
// What it reads of the row: the dwords (x0*bits) / 32 .. ((x0 + n)*bits - 1) / 32 of it, each with one aligned load and none
// of them twice.  With x0 + n <= width they all lie inside the row's rowb bytes, so nothing beyond a row's padded length
// is ever read.  On the device the row is 4-byte aligned (a payload is 16-byte aligned and rowb a multiple of 4); the
// host, whose rows lie wherever the file put them, loads the same dwords with memcpy.
#pragma once
#include <stdint.h>
#include <string.h>

#include "png_filter.h"

// (every loop below has a constant trip count; the device compiler is told to unroll them so that the arrays stay in registers)
#if defined(__clang__)
#define MRG_BMP_UNROLL _Pragma("unroll")
#else
#define MRG_BMP_UNROLL
#endif

namespace mrg {

// dword i of a row
MRG_PNG_HD uint32_t bmp_dword(const uint8_t* row, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const uint32_t*)row)[i];
#else
    uint32_t v;
    memcpy(&v, row + 4 * (size_t)i, 4);  // (little-endian hosts only, like the rest of the readers' fast paths)
    return v;
#endif
}

// the 32 bits that begin r bits (0 .. 31) into lo and go on in hi (the device has the instruction: v_alignbit_b32)
MRG_PNG_HD uint32_t bmp_funnel(uint32_t lo, uint32_t hi, int r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)r);
#else
    return (uint32_t)((((unsigned long long)hi << 32) | lo) >> r);
#endif
}

MRG_PNG_HD uint32_t bmp_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

// the most dwords of a row that hold 16 pixels beginning at any pixel: 16 bits from any bit, 64 bits from any nibble,
// 16 and 48 bytes from any byte, 64 bytes from a dword
template <int BITS>
struct BmpSpan {
    static constexpr int kDwords = BITS == 1 ? 2 : BITS == 4 ? 3 : BITS == 8 ? 5 : BITS == 24 ? 13 : 16;
};

// BITS 1, 4, 8: lut is the file's 256-byte grey table (bmp_layout); LUT false (8 bits only): the table is the identity
// and is not read.  BITS 24, 32: png_grey of the sample triple, lut is not read.
template <int BITS, bool LUT>
MRG_PNG_HD void bmp_pixels(const uint8_t* row, int rowb, const uint8_t* lut, int x0, int n, uint32_t out[4]) {
    static_assert(BITS == 1 || BITS == 4 || BITS == 8 || BITS == 24 || BITS == 32, "BMP depths");
    static_assert(LUT ? BITS <= 8 : BITS >= 8, "a table for palette depths; none at 8 bits (identity) and for colour");
    constexpr int ND = BmpSpan<BITS>::kDwords;
    const int bit0 = x0 * BITS, d0 = bit0 >> 5;
    int dlast = ((x0 + n) * BITS - 1) >> 5;
    if (dlast > (rowb >> 2) - 1) dlast = (rowb >> 2) - 1;  // (never taken with x0 + n <= width)
    // w[ND]: one dword more than is loaded, for the funnel shifts below
    uint32_t w[ND + 1];
    MRG_BMP_UNROLL
    for (int i = 0; i < ND; ++i) w[i] = d0 + i <= dlast ? bmp_dword(row, d0 + i) : 0u;
    w[ND] = 0u;
    if constexpr (BITS == 1 || BITS == 4) {
        // a bit stream, most significant bit first: the dwords byte-swapped, then shifted up by the first pixel's bit
        constexpr int NV = BITS == 1 ? 1 : 2;
        const int sh = bit0 & 31;
        uint32_t v[NV];
        MRG_BMP_UNROLL
        for (int i = 0; i < NV; ++i) {
            const unsigned long long two = ((unsigned long long)bmp_bswap(w[i]) << 32) | bmp_bswap(w[i + 1]);
            v[i] = (uint32_t)((two << sh) >> 32);
        }
        const uint32_t t0 = lut[0], t1 = lut[1];  // (all of a 1-bit table)
        MRG_BMP_UNROLL
        for (int q = 0; q < 4; ++q) {
            uint32_t d = 0;
            MRG_BMP_UNROLL
            for (int p = 0; p < 4; ++p) {
                const int px = 4 * q + p;
                if constexpr (BITS == 1) d |= (((v[0] >> (31 - px)) & 1u) ? t1 : t0) << (8 * p);
                else d |= (uint32_t)lut[(v[px >> 3] >> (28 - 4 * (px & 7))) & 15u] << (8 * p);
            }
            out[q] = d;
        }
    } else {
        // whole bytes: shifted down by the first pixel's byte inside its dword
        constexpr int NV = BITS == 8 ? 4 : BITS == 24 ? 12 : 16;
        const int r = 8 * ((bit0 >> 3) & 3);
        uint32_t v[NV];
        MRG_BMP_UNROLL
        for (int i = 0; i < NV; ++i) v[i] = bmp_funnel(w[i], w[i + 1], r);
        MRG_BMP_UNROLL
        for (int q = 0; q < 4; ++q) {
            uint32_t d = 0;
            MRG_BMP_UNROLL
            for (int p = 0; p < 4; ++p) {
                const int px = 4 * q + p;
                if constexpr (BITS == 8) {
                    const uint32_t idx = (v[q] >> (8 * p)) & 255u;
                    if constexpr (LUT) d |= (uint32_t)lut[idx] << (8 * p);
                    else d |= idx << (8 * p);
                } else if constexpr (BITS == 32) {
                    // B G R X: the fourth byte is ignored
                    d |= png_grey((v[px] >> 16) & 255u, (v[px] >> 8) & 255u, v[px] & 255u) << (8 * p);
                } else {
                    const int k = 3 * px;  // byte k of the 48: B, then G, then R
                    const uint32_t b = (v[k >> 2] >> (8 * (k & 3))) & 255u;
                    const uint32_t g = (v[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 255u;
                    const uint32_t rr = (v[(k + 2) >> 2] >> (8 * ((k + 2) & 3))) & 255u;
                    d |= png_grey(rr, g, b) << (8 * p);
                }
            }
            out[q] = d;
        }
    }
}

// the same by a depth known at run time (the host decoder); lut NULL at 8 bits: the identity table
MRG_PNG_HD void bmp_pixels_any(const uint8_t* row, int rowb, int bits, const uint8_t* lut, int x0, int n, uint32_t out[4]) {
    switch (bits) {
        case 1: bmp_pixels<1, true>(row, rowb, lut, x0, n, out); break;
        case 4: bmp_pixels<4, true>(row, rowb, lut, x0, n, out); break;
        case 8:
            if (lut) bmp_pixels<8, true>(row, rowb, lut, x0, n, out);
            else bmp_pixels<8, false>(row, rowb, lut, x0, n, out);
            break;
        case 24: bmp_pixels<24, false>(row, rowb, lut, x0, n, out); break;
        default: bmp_pixels<32, false>(row, rowb, lut, x0, n, out); break;
    }
}

}  // namespace mrg
