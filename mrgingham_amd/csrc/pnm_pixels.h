// The pixels of one row of a binary Netpbm raster (PBM "P4", PGM "P5", PAM "P7") to grey, one text for the host
// decoder (image_io.cpp: decode_pnm) and the device kernel (pnm_unpack.hip), like bmp_pixels.h.  A raster is `height` rows of
// row_bytes bytes without any padding, so a row begins at ANY byte of the payload: its phase against the aligned dwords
// changes from row to row.  BITS 1: packed bits, the leftmost pixel in the most significant bit of a byte, bit 1 black.
// BITS 8 / 16: CH samples per pixel (16: big-endian pairs); the grey is the first sample (CH 1, 2) or png_grey of the first
// three (CH 3, 4), at the samples' own width; BW: 255 where the first sample is non-zero, else 0.
//
// pnm_pixels gives the grey samples of the pixels [x0, x0 + n) of the row that begins `row_off` bytes behind `base`, packed
// into four dwords: n <= 16 bytes (pixel x0 + p is byte p & 3 of out[p >> 2]) for BITS 1 and 8, n <= 8 native 16-bit samples
// (pixel x0 + p is half p & 1 of out[p >> 1]) for BITS 16; what lies beyond n is unspecified.
//
// What it reads: the aligned dwords of `base` that hold the first to the last source byte of those pixels, each with one
// load and none of them twice -- at most 17 (64 bytes from any byte).  With x0 + n <= width they hold bytes of the row, so
// nothing behind the payload rounded up to dwords is read; on the device `base` is 16-byte aligned and the payload padded
// to 16 bytes.  The host, whose payload lies wherever the file put it and ends where the file ends, loads the same dwords
// with memcpy and takes of the last one only the bytes inside `limit`.
#pragma once
#include <stdint.h>
#include <string.h>

#include "png_filter.h"

// (every loop below has a constant trip count; the device compiler is told to unroll them so that the arrays stay in registers)
#if defined(__clang__)
#define MRG_PNM_UNROLL _Pragma("unroll")
#else
#define MRG_PNM_UNROLL
#endif

namespace mrg {

// dword d0 + i of the payload; limit: the bytes of the payload that may be read (the device's is padded: every dword is whole)
MRG_PNG_HD uint32_t pnm_dword(const uint8_t* base, long long d0, int i, long long limit) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)limit;
    return ((const uint32_t*)base + d0)[i];  // (one address per word, the dwords at constant offsets from it)
#else
    uint32_t v = 0;
    const long long left = limit - 4 * (d0 + i);
    memcpy(&v, base + 4 * (d0 + i), left >= 4 ? 4 : left > 0 ? (size_t)left : 0);  // (little-endian hosts only, like the rest of the readers' fast paths)
    return v;
#endif
}

// the 32 bits that begin r bits (0 .. 31) into lo and go on in hi (the device has the instruction: v_alignbit_b32)
MRG_PNG_HD uint32_t pnm_funnel(uint32_t lo, uint32_t hi, int r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)r);
#else
    return r ? (lo >> r) | (hi << (32 - r)) : lo;
#endif
}

MRG_PNG_HD uint32_t pnm_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

template <int BITS, int CH>
struct PnmSpan {
    static constexpr int kPixels = BITS == 16 ? 8 : 16;                        // of one 16-byte destination word
    static constexpr int kBytes = BITS == 1 ? 2 : kPixels * CH * (BITS / 8);   // their source bytes (bits: from any bit, see below)
    static constexpr int kShifted = BITS == 1 ? 1 : kBytes / 4;                // dwords behind the shift
    static constexpr int kDwords = BITS == 1 ? 2 : kShifted + 1;               // the most dwords that hold them, from any byte
};

// sample k of a byte stream held in v[] from byte 0 on (k a constant once the loops are unrolled)
template <int BITS>
MRG_PNG_HD uint32_t pnm_sample(const uint32_t* v, int k) {
    if constexpr (BITS == 8) {
        return (v[k >> 2] >> (8 * (k & 3))) & 255u;
    } else {
        const uint32_t h = (v[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;  // the pair as a little-endian load sees it
        return ((h & 255u) << 8) | (h >> 8);
    }
}

template <int BITS, int CH, bool BW>
MRG_PNG_HD void pnm_pixels(const uint8_t* base, long long limit, long long row_off, int x0, int n, uint32_t out[4]) {
    static_assert(BITS == 1 || BITS == 8 || BITS == 16, "Netpbm sample widths");
    static_assert(CH >= 1 && CH <= 4 && (BITS != 1 || CH == 1), "1 .. 4 samples per pixel; bits are one channel");
    static_assert(!BW || (BITS == 8 && CH <= 2), "black and white: 8-bit samples, depth 1 or 2");
    using S = PnmSpan<BITS, CH>;
    constexpr int ND = S::kDwords, NV = S::kShifted;
    // the first and the last source bit of the pixels, and the dwords that hold them
    const long long bit0 = BITS == 1 ? 8 * row_off + x0 : 8 * (row_off + (long long)x0 * CH * (BITS / 8));
    const long long bit1 = bit0 + (BITS == 1 ? (long long)n : (long long)n * CH * BITS) - 1;
    const long long d0 = bit0 >> 5;
    const int nd = (int)((bit1 >> 5) - d0) + 1;  // 1 .. ND
    // w[ND]: one dword more than is loaded, for the funnel shifts below
    uint32_t w[ND + 1];
    MRG_PNM_UNROLL
    for (int i = 0; i < ND; ++i) w[i] = i < nd ? pnm_dword(base, d0, i, limit) : 0u;
    w[ND] = 0u;
    if constexpr (BITS == 1) {
        // a bit stream, most significant bit first: the dwords byte-swapped, then shifted up by the first pixel's bit
        const int sh = (int)(bit0 & 31);
        const uint32_t a = pnm_bswap(w[0]), b = pnm_bswap(w[1]);
        const uint32_t v = sh ? pnm_funnel(b, a, 32 - sh) : a;
        MRG_PNM_UNROLL
        for (int q = 0; q < 4; ++q) {
            uint32_t d = 0;
            MRG_PNM_UNROLL
            for (int p = 0; p < 4; ++p) d |= (((v >> (31 - (4 * q + p))) & 1u) ? 0u : 255u) << (8 * p);  // bit 1 is black
            out[q] = d;
        }
    } else {
        // whole bytes: shifted down by the first pixel's byte inside its dword
        const int r = (int)(bit0 & 31);
        uint32_t v[NV];
        MRG_PNM_UNROLL
        for (int i = 0; i < NV; ++i) v[i] = pnm_funnel(w[i], w[i + 1], r);
        MRG_PNM_UNROLL
        for (int q = 0; q < 4; ++q) {
            uint32_t d = 0;
            constexpr int per = BITS == 16 ? 2 : 4;  // samples of a destination dword
            MRG_PNM_UNROLL
            for (int p = 0; p < per; ++p) {
                const int px = per * q + p;
                uint32_t g = pnm_sample<BITS>(v, CH * px);
                if constexpr (CH >= 3) g = png_grey(g, pnm_sample<BITS>(v, CH * px + 1), pnm_sample<BITS>(v, CH * px + 2));
                if constexpr (BW) g = g ? 255u : 0u;
                d |= g << (BITS * p);
            }
            out[q] = d;
        }
    }
}

// the same by a layout known at run time; false: not a layout of the subset
MRG_PNG_HD bool pnm_pixels_any(const uint8_t* base, long long limit, long long row_off, int bits, int channels, bool bw, int x0, int n,
                               uint32_t out[4]) {
#define MRG_PNM_CASE(B, C, W)                                  \
    if (bits == B && channels == C && bw == W) {                \
        pnm_pixels<B, C, W>(base, limit, row_off, x0, n, out); \
        return true;                                            \
    }
    MRG_PNM_CASE(1, 1, false)
    MRG_PNM_CASE(8, 1, false) MRG_PNM_CASE(8, 2, false) MRG_PNM_CASE(8, 3, false) MRG_PNM_CASE(8, 4, false)
    MRG_PNM_CASE(16, 1, false) MRG_PNM_CASE(16, 2, false) MRG_PNM_CASE(16, 3, false) MRG_PNM_CASE(16, 4, false)
    MRG_PNM_CASE(8, 1, true) MRG_PNM_CASE(8, 2, true)
#undef MRG_PNM_CASE
    return false;
}

}  // namespace mrg
