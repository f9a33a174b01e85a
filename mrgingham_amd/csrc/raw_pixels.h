// The samples of one row of a packed 10 / 12 / 14-bit camera frame (GenICam Mono10p / Mono12p / Mono14p, GigE Vision
// Mono10Packed / Mono12Packed) as native 16-bit values, one text for the host decoder (image_io.cpp:
// mrgingham_amd_raw_unpack_image) and the device kernel (raw_unpack.hip), like pnm_pixels.h.  A frame is `height` rows,
// row y at byte y * row_bytes of the payload; nothing is shared between rows, and a row begins at ANY byte, so its phase
// against the aligned dwords changes from row to row.
//   stream formats (P10, P12, P14): a row is one bit stream, least significant bit first -- stream bit b is bit b % 8 of
//     byte b / 8 --, sample x its bits [x*N, (x+1)*N), least significant first: as dwords loaded little-endian, simply bit
//     x*N onwards of the row;
//   pair formats (GEV10, GEV12): pixels 2g, 2g+1 are bytes 3g .. 3g+2, p0 = byte0 << L | (byte1 & (2^L - 1)),
//     p1 = byte2 << L | ((byte1 >> 4) & (2^L - 1)), L = 2 or 4 (at L = 2 the bits 2, 3, 6, 7 of byte1 are ignored).
// The value is the sample as it is, 0 .. 2^N - 1, not left-justified.
//
// raw_pixels gives the samples [x0, x0 + n), n <= 8, of the row that begins `row_off` bytes behind `base`, for any x0 --
// an odd one in the pair formats, every bit phase in the stream formats --, packed into four dwords (sample x0 + p is
// half p & 1 of out[p >> 1]); what lies beyond n is unspecified.
//
// What it reads: the aligned dwords of `base` that hold the first to the last source byte of those samples, each with one
// load and none of them twice -- at most 5.  With x0 + n <= width they hold bytes of the row, so nothing behind the
// payload rounded up to dwords is read; on the device `base` is 16-byte aligned and the payload padded to 16 bytes.  The
// host, whose payload lies wherever its owner put it, loads the same dwords with memcpy and takes of the last one only the
// bytes inside `limit` (pnm_dword).
#pragma once
#include <stdint.h>

#include "../../include/mrgingham_amd.h"
#include "pnm_pixels.h"

namespace mrg {

MRG_PNG_HD constexpr bool raw_format_ok(int fmt) { return fmt >= MRGINGHAM_AMD_RAW_P10 && fmt <= MRGINGHAM_AMD_RAW_GEV12; }
MRG_PNG_HD constexpr bool raw_pairs(int fmt) { return fmt == MRGINGHAM_AMD_RAW_GEV10 || fmt == MRGINGHAM_AMD_RAW_GEV12; }
MRG_PNG_HD constexpr int raw_bits(int fmt) {
    return fmt == MRGINGHAM_AMD_RAW_P10 || fmt == MRGINGHAM_AMD_RAW_GEV10 ? 10 : fmt == MRGINGHAM_AMD_RAW_P14 ? 14 : 12;
}
// the fewest bytes that hold a row of `width` samples
MRG_PNG_HD constexpr long long raw_min_row_bytes(int width, int fmt) {
    return raw_pairs(fmt) ? 3ll * ((width + 1) / 2) : ((long long)width * raw_bits(fmt) + 7) / 8;
}

template <int FMT>
MRG_PNG_HD void raw_pixels(const uint8_t* base, long long limit, long long row_off, int x0, int n, uint32_t out[4]) {
    static_assert(raw_format_ok(FMT), "packed camera formats");
    constexpr int N = raw_bits(FMT);
    constexpr uint32_t mask = (1u << N) - 1u;
    if constexpr (!raw_pairs(FMT)) {
        constexpr int NV = (8 * N + 31) / 32;       // dwords of eight samples from bit 0
        constexpr int ND = (31 + 8 * N + 31) / 32;  // the most dwords that hold them, from any bit
        const long long bit0 = 8 * row_off + (long long)x0 * N, bit1 = bit0 + (long long)n * N - 1;
        const long long d0 = bit0 >> 5;
        const int nd = (int)((bit1 >> 5) - d0) + 1;  // 1 .. ND
        uint32_t w[ND + 1];                          // (one dword more than is loaded, for the funnel shifts below)
        MRG_PNM_UNROLL
        for (int i = 0; i < ND; ++i) w[i] = i < nd ? pnm_dword(base, d0, i, limit) : 0u;
        w[ND] = 0u;
        // shifted down by the first sample's bit inside its dword
        const int r = (int)(bit0 & 31);
        uint32_t v[NV + 1];
        MRG_PNM_UNROLL
        for (int i = 0; i < NV; ++i) v[i] = pnm_funnel(w[i], w[i + 1], r);
        v[NV] = 0u;
        MRG_PNM_UNROLL
        for (int q = 0; q < 4; ++q) {
            uint32_t d = 0;
            MRG_PNM_UNROLL
            for (int p = 0; p < 2; ++p) {
                const int lo = (2 * q + p) * N, word = lo >> 5, off = lo & 31;  // (constants once unrolled)
                const uint32_t s = off + N <= 32 ? v[word] >> off : pnm_funnel(v[word], v[word + 1], off);
                d |= (s & mask) << (16 * p);
            }
            out[q] = d;
        }
    } else {
        // five pairs from the pair of x0 on: an odd x0 begins at the second sample of its pair
        constexpr int L = N - 8;
        constexpr uint32_t lmask = (1u << L) - 1u;
        constexpr int NV = 4, ND = 5;  // 15 bytes from byte 0; from any byte
        const int odd = x0 & 1, xl = x0 + n - 1;
        const long long byte0 = row_off + 3ll * (x0 >> 1), byte1 = row_off + 3ll * (xl >> 1) + 1 + (xl & 1);
        const long long d0 = byte0 >> 2;
        const int nd = (int)((byte1 >> 2) - d0) + 1;  // 1 .. ND
        uint32_t w[ND + 1];
        MRG_PNM_UNROLL
        for (int i = 0; i < ND; ++i) w[i] = i < nd ? pnm_dword(base, d0, i, limit) : 0u;
        w[ND] = 0u;
        const int r = 8 * (int)(byte0 & 3);
        uint32_t v[NV];
        MRG_PNM_UNROLL
        for (int i = 0; i < NV; ++i) v[i] = pnm_funnel(w[i], w[i + 1], r);
        uint32_t s[10];
        MRG_PNM_UNROLL
        for (int g = 0; g < 5; ++g) {
            const uint32_t b0 = pnm_sample<8>(v, 3 * g), b1 = pnm_sample<8>(v, 3 * g + 1), b2 = pnm_sample<8>(v, 3 * g + 2);
            s[2 * g] = (b0 << L) | (b1 & lmask);
            s[2 * g + 1] = (b2 << L) | ((b1 >> 4) & lmask);
        }
        MRG_PNM_UNROLL
        for (int q = 0; q < 4; ++q)
            out[q] = odd ? s[2 * q + 1] | (s[2 * q + 2] << 16) : s[2 * q] | (s[2 * q + 1] << 16);
    }
}

// the same by a format known at run time; false: not a format
MRG_PNG_HD bool raw_pixels_any(const uint8_t* base, long long limit, long long row_off, int fmt, int x0, int n, uint32_t out[4]) {
    switch (fmt) {
        case MRGINGHAM_AMD_RAW_P10: raw_pixels<MRGINGHAM_AMD_RAW_P10>(base, limit, row_off, x0, n, out); return true;
        case MRGINGHAM_AMD_RAW_P12: raw_pixels<MRGINGHAM_AMD_RAW_P12>(base, limit, row_off, x0, n, out); return true;
        case MRGINGHAM_AMD_RAW_P14: raw_pixels<MRGINGHAM_AMD_RAW_P14>(base, limit, row_off, x0, n, out); return true;
        case MRGINGHAM_AMD_RAW_GEV10: raw_pixels<MRGINGHAM_AMD_RAW_GEV10>(base, limit, row_off, x0, n, out); return true;
        case MRGINGHAM_AMD_RAW_GEV12: raw_pixels<MRGINGHAM_AMD_RAW_GEV12>(base, limit, row_off, x0, n, out); return true;
    }
    return false;
}

}  // namespace mrg
