// The Huffman decode of ONE restart interval of a baseline JPEG, ONE text for the host (jpeg.cpp's scan hands out the
// intervals; tests/boundary/jpeg_lane_main.cpp runs it under the sanitizers) and for the device (jpeg_huff.hip: one lane
// per interval).  A restart interval begins byte-aligned with the DC predictors reset, so the intervals of a file are
// independent streams.  It is decode_block of jpeg.cpp restated so that the lanes of a wave stay together: every trip of
// the loop decodes exactly one Huffman symbol, DC or AC, and the position in the MCU (component, block, k) lives in
// registers.  It fails where the host decoder fails -- a code the table does not have, a DC category above 11, an AC size
// above 10, a run past coefficient 63, a predictor that leaves int16, a bit consumed beyond `end`, and, for every interval
// but the file's last, a whole unread byte left in front of the marker.
// Termination is structural: a trip consumes at least one real bit or fails, so there are at most 8 * (end - begin) of
// them.  Every index that comes from the stream (symbol index, k, block address) is checked before use; the stream is
// read as the aligned dwords that overlap [begin, end), i.e. up to 3 bytes on either side of it on the device (the
// staging is padded for that; what those bytes hold never matters) and not one byte outside it on the host.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define MRG_JPEG_HD __host__ __device__
#else
#define MRG_JPEG_HD
#endif

// position in the zigzag scan -> position in the block, row-major
#define MRG_JPEG_NATURAL_ORDER                                                                                          \
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, \
        35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, \
        55, 62, 63

namespace mrg {

constexpr int kJpegLookBits = 9;

// One Huffman table, flat and pointer-free (1424 bytes, a whole number of dwords: copied to LDS as it is).
struct JpegHuffTable {
    uint16_t look[1 << kJpegLookBits];  // the next 9 bits -> (code length << 8) | symbol; 0: a longer code, or none
    int32_t maxcode[17];                // [l]: the largest code of l bits, -1 where there is none
    int32_t valoff[17];                 // symbol index of a code of l bits = code + valoff[l]
    int32_t nvals;
    int32_t defined;
    uint8_t vals[256];
};
static_assert(sizeof(JpegHuffTable) == 1424, "JpegHuffTable is copied as dwords");

// What the frame gives every one of its lanes (uniform over a workgroup).
struct JpegLaneGeom {
    int32_t ncomp;
    int32_t H0, V0;        // luma blocks per MCU, across and down (1, 1 for a single-component scan)
    int32_t mcus_x;        // MCUs per MCU row
    uint32_t nblk;         // byte c: blocks of component c in an MCU (h * v, 1 .. 16)
    uint32_t slots;        // nibble c: where in `tables` component c's DC table lies; nibble 4 + c: its AC table
    int32_t blocks_h;      // block rows the coefficient area holds
    int32_t pitch_blocks;  // blocks per stored block row
};

constexpr int kJpegLaneTables = 6;  // at most three DC and three AC tables are named by a scan

// The dword `w` of the stream (bytes 4w .. 4w + 3, the first in the low byte).
MRG_JPEG_HD inline uint32_t jpeg_lane_word(const uint8_t* stream, uint32_t w, uint32_t begin, uint32_t end) {
#ifdef __HIP_DEVICE_COMPILE__
    return ((const uint32_t*)stream)[w];  // `stream` is dword aligned and padded past `end`
#else
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t p = 4 * w + j;
        if (p >= begin && p < end) v |= (uint32_t)stream[p] << (8 * j);
    }
    return v;
#endif
}

// stream[begin .. end): the entropy-coded bytes of the interval, up to (not including) the marker that ends it, so that
// every FF inside is followed by its stuffed 00.  first_mcu / nmcu: the MCUs it holds, in the frame's MCU raster order.
// coef: the frame's luma coefficients, int16 [blocks_h][pitch_blocks][64], natural order inside a block.  kWholeBlocks:
// every luma block of the interval is written in full (zeros included); otherwise only the non-zero coefficients are
// stored, into an area the caller has zeroed.  true: decoded; false: the host decoder calls this file unreadable.
template <bool kWholeBlocks>
MRG_JPEG_HD inline bool jpeg_huff_lane(const uint8_t* stream, uint32_t begin, uint32_t end, const JpegHuffTable* tables,
                                       const uint8_t* natural, const JpegLaneGeom& g, uint32_t first_mcu, uint32_t nmcu,
                                       bool last_interval, int16_t* coef) {
    // the bit reader: zero bits are fed and counted where the data ends; having CONSUMED one of them is the overrun
    uint64_t acc = 0;
    int n = 0;            // valid bits at the bottom of acc
    int pad = 0;          // of which fed zeros: always the lowest ones
    uint32_t pos = begin;  // the next unread byte
    bool after_ff = false;  // the byte at pos is the 00 stuffed behind an FF

    int pred0 = 0, pred1 = 0, pred2 = 0;
    int c = 0, bi = 0, k = 0;  // component, block of it inside the MCU, coefficient (0: the DC symbol is next)
    int bcol = 0, brow = 0;    // where block bi of the luma component lies inside the MCU
    uint32_t done = 0;         // MCUs of the interval behind us
    uint32_t mx = first_mcu % (uint32_t)g.mcus_x, my = first_mcu / (uint32_t)g.mcus_x;
    int16_t* dst = nullptr;  // the luma block being filled

    while (done < nmcu) {
        if (n < 32) {  // a code (<= 16 bits) and its value bits (<= 11) fit
            if (pos < end) {
                const uint32_t w = jpeg_lane_word(stream, pos >> 2, begin, end);
                const uint32_t base = pos & ~3u;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t p = base + j;
                    if (p < pos || p >= end) continue;
                    const uint32_t b = (w >> (8 * j)) & 0xFFu;
                    if (!after_ff) {
                        acc = (acc << 8) | b;
                        n += 8;
                    }
                    after_ff = !after_ff && b == 0xFFu;
                }
                pos = base + 4 < end ? base + 4 : end;
                continue;  // (n < 32 again: one more dword; at most 32 bits are added to fewer than 32)
            }
            acc <<= 32;
            n += 32;
            pad += 32;
        }
        const uint32_t slot = (g.slots >> (4 * (k == 0 ? c : 4 + c))) & 15u;
        const JpegHuffTable& t = tables[slot < (uint32_t)kJpegLaneTables ? slot : 0];
        // one symbol
        int sym, len;
        const uint32_t e = t.look[(uint32_t)(acc >> (n - kJpegLookBits)) & ((1u << kJpegLookBits) - 1u)];
        if (e) {
            len = (int)(e >> 8);
            sym = (int)(e & 0xFFu);
        } else {
            sym = -1;
            len = 0;
            for (int l = kJpegLookBits + 1; l <= 16; ++l) {
                const int32_t code = (int32_t)((uint32_t)(acc >> (n - l)) & ((1u << l) - 1u));
                if (code <= t.maxcode[l]) {
                    const int idx = code + t.valoff[l];
                    if (idx >= 0 && idx < t.nvals && idx < 256) {
                        sym = t.vals[idx];
                        len = l;
                    }
                    break;
                }
            }
            if (sym < 0) return false;
        }
        n -= len;
        const int s = k == 0 ? sym : sym & 15;
        int v = 0;
        if (s) {
            if (s > (k == 0 ? 11 : 10)) return false;
            v = (int)((uint32_t)(acc >> (n - s)) & ((1u << s) - 1u));
            n -= s;
            if (v < (1 << (s - 1))) v += 1 - (1 << s);
        }
        if (n < pad) return false;  // a bit beyond `end` was consumed
        bool block_done = false;
        if (k == 0) {  // the DC difference onto the component's predictor
            int pred = (c == 0 ? pred0 : c == 1 ? pred1 : pred2) + v;
            if (pred < -32768 || pred > 32767) return false;
            if (c == 0) pred0 = pred;
            else if (c == 1) pred1 = pred;
            else pred2 = pred;
            dst = nullptr;
            if (c == 0) {
                const uint32_t bx = mx * (uint32_t)g.H0 + (uint32_t)bcol, by = my * (uint32_t)g.V0 + (uint32_t)brow;
                if (bx >= (uint32_t)g.pitch_blocks || by >= (uint32_t)g.blocks_h) return false;
                dst = coef + ((size_t)by * (size_t)g.pitch_blocks + bx) * 64;
                if (kWholeBlocks) {
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
                    for (int q = 0; q < 8; ++q) ((uint4*)dst)[q] = make_uint4(0, 0, 0, 0);  // (the area is 16-byte aligned)
#else
                    memset(dst, 0, 64 * sizeof(int16_t));
#endif
                    dst[0] = (int16_t)pred;
                } else if (pred) {
                    dst[0] = (int16_t)pred;
                }
            }
            k = 1;
        } else {
            const int r = sym >> 4;
            if (s == 0) {
                if (r != 15) {
                    block_done = true;  // end of block (r != 0: a progressive file's EOB run has no meaning here)
                } else {
                    if (k + 15 > 63) return false;  // sixteen zeros that do not fit
                    k += 16;
                }
            } else {
                k += r;
                if (k > 63) return false;
                if (dst && (kWholeBlocks || v)) dst[natural[k]] = (int16_t)v;
                ++k;
            }
            if (k > 63) block_done = true;
        }
        if (block_done) {
            k = 0;
            if (++bcol >= g.H0) { bcol = 0; ++brow; }
            if (++bi >= (int)((g.nblk >> (8 * c)) & 0xFFu)) {
                bi = bcol = brow = 0;
                if (++c >= g.ncomp) {
                    c = 0;
                    ++done;
                    if (++mx >= (uint32_t)g.mcus_x) { mx = 0; ++my; }
                }
            }
        }
    }
    // RSTn exactly here: nothing but the last byte's padding bits is left over (the file's last interval: not looked at)
    // (a stuffed 00 that lies in the next dword is no unread byte)
    return last_interval || (pos + (after_ff ? 1u : 0u) >= end && n - pad < 8);
}

}  // namespace mrg
