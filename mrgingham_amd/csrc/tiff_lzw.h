// The LZW decoder of one TIFF strip, one text for the host decoder (image_io.cpp: decode_tiff) and the device kernel
// (tiff_decode.hip: one lane per strip), like jpeg_huff_lane.h and png_filter.h.  TIFF's flavour: codes MSB first, 9 to 12
// bits, ClearCode 256, EOI 257, and the width grows one code early -- the decoder reads the next code at width + 1 as
// soon as its next free code reaches 2^width - 1.
//
// The table holds no strings.  Every string the decoder emits lies in the strip's own output, so an entry is (position in
// the output, length): the string of a new code is the previous string plus the first byte of the current one, and those
// bytes are already contiguous in the output.  Adding an entry is one store; emitting a string is a forward byte copy from
// the decoder's own earlier output; the code-equals-next-free case (KwKwK) is that same copy overlapping its destination.
// Where the table lives is the template parameter: anything with set(code, position, length) and get(code, &position,
// &length) for codes 258 .. 4095.
//
// The rules (include/mrgingham_amd.h, mrgingham_amd_tiff_layout): the decoder starts cleared whether or not the stream
// opens with ClearCode; it stops as soon as `nout` bytes are out and ignores what follows; a code above the next free one,
// a non-clear code after the table is full, an EOI or the end of the bytes before `nout` bytes are out are errors.  It
// never reads beyond src + nsrc and never writes beyond out + nout.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRG_TIFF_HD __host__ __device__ inline
#else
#define MRG_TIFF_HD inline
#endif

namespace mrg {

constexpr int kTiffLzwClear = 256, kTiffLzwEoi = 257, kTiffLzwFirst = 258, kTiffLzwCodes = 4096;
// what tiff_lzw_decode returns
constexpr int kTiffLzwOk = 0;
constexpr int kTiffLzwCodeAboveNext = 1;  // a code above the next free one (or a table code right after a clear)
constexpr int kTiffLzwEarlyEoi = 2;       // EOI before the strip's bytes are out
constexpr int kTiffLzwCutShort = 3;       // the bytes end before the strip's bytes are out
constexpr int kTiffLzwTableFull = 4;      // a non-clear code after the table is full
constexpr int kTiffLzwBadStrip = 5;       // (the kernel's own: a strip record that does not fit its file or its frame)

// a table entry in one dword: 20 bits of position, 12 bits of length -- strips of up to 1 MiB (strings are shorter than
// 4096 bytes: a string is one byte longer than an earlier one, and there are fewer than 4096 of them between two clears)
constexpr uint32_t kTiffLzwMaxStrip20 = 1u << 20;
MRG_TIFF_HD uint32_t tiff_lzw_pack(uint32_t position, uint32_t length) { return position << 12 | length; }

// the host's table: any strip size
struct TiffLzwHostTable {
    uint32_t pos[kTiffLzwCodes];
    uint16_t len[kTiffLzwCodes];
    void set(int code, uint32_t position, uint32_t length) { pos[code] = position; len[code] = (uint16_t)length; }
    void get(int code, uint32_t* position, uint32_t* length) const { *position = pos[code]; *length = len[code]; }
};

// packed dwords `stride` apart (the kernel: the tables of the lanes of a launch interleaved by lane, so that the lanes of a
// wave touch consecutive words; 1: a table of its own, what the sanitizer program walks); strips of at most 1 MiB
struct TiffLzwPackedTable {
    uint32_t* word;  // entry of code c at word[c * stride]
    uint32_t stride;
    MRG_TIFF_HD void set(int code, uint32_t position, uint32_t length) { word[(uint32_t)code * stride] = tiff_lzw_pack(position, length); }
    MRG_TIFF_HD void get(int code, uint32_t* position, uint32_t* length) const {
        const uint32_t v = word[(uint32_t)code * stride];
        *position = v >> 12;
        *length = v & 4095u;
    }
};

template <class Table>
MRG_TIFF_HD int tiff_lzw_decode(const uint8_t* src, uint32_t nsrc, uint8_t* out, uint32_t nout, Table& tab) {
    uint32_t in = 0, acc = 0, o = 0;   // bytes taken, the bits not yet used (the low `have` bits of acc), bytes out
    int have = 0, width = 9, next = kTiffLzwFirst;
    bool fresh = true;                 // no previous string: right after a clear
    uint32_t ppos = 0, plen = 0;       // the previous string
    while (o < nout) {
        while (have < width && in < nsrc) {
            acc = (acc << 8) | src[in++];
            have += 8;
        }
        if (have < width) return kTiffLzwCutShort;
        const int code = (int)((acc >> (have - width)) & ((1u << width) - 1u));
        have -= width;
        if (code == kTiffLzwClear) {
            width = 9;
            next = kTiffLzwFirst;
            fresh = true;
            continue;
        }
        if (code == kTiffLzwEoi) return kTiffLzwEarlyEoi;
        const uint32_t at = o;
        uint32_t len;
        if (fresh) {
            if (code > 255) return kTiffLzwCodeAboveNext;
            out[o++] = (uint8_t)code;
            len = 1;
            fresh = false;
        } else {
            if (next >= kTiffLzwCodes) return kTiffLzwTableFull;
            if (code > next) return kTiffLzwCodeAboveNext;
            if (code < 256) {
                out[o++] = (uint8_t)code;
                len = 1;
            } else {
                uint32_t from;
                if (code == next) {  // the previous string and its own first byte: the copy runs into what it writes
                    from = ppos;
                    len = plen + 1;
                } else {
                    tab.get(code, &from, &len);
                }
                const uint32_t n = len < nout - o ? len : nout - o;
                for (uint32_t i = 0; i < n; ++i) out[o + i] = out[from + i];
                o += n;
            }
            // the previous string and the first byte of this one lie side by side in the output
            tab.set(next, ppos, plen + 1);
            ++next;
            if (next + 1 >= (1 << width) && width < 12) ++width;
        }
        ppos = at;
        plen = len;
    }
    return kTiffLzwOk;
}

}  // namespace mrg
