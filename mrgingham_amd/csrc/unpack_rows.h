// The row schedule of the unpack kernels (bmp_unpack_kernel, pnm_unpack_kernel, raw_unpack_kernel), once: which pixels
// a 16-byte word of a destination row holds, how many lanes take a row and how many workgroups a launch has (host and
// device, for a stand-alone program too: tests/boundary/unpack_rows_main.cpp), and the loop itself (device).
//
// THE SCHEDULE.  A grid-stride loop over the rows of all frames; a row is taken by 2^lpr_shift lanes of a workgroup
// (256 >> lpr_shift rows side by side), lane l by the words l, l + lanes, ... of the DESTINATION row: consecutive lanes
// store consecutive 16-byte words.  Word k of a row whose destination begins `ph` bytes behind a 16-byte boundary holds
// the samples of the pixels [(16k - ph) / ES, (16k - ph) / ES + 16 / ES) that lie inside the row (ES: bytes of a
// destination sample; ph is even at ES 2); a whole word is one 16-byte store (its address is a multiple of 16 by
// construction), the head and the tail of a row go out sample by sample.  Where a row's source begins and what fills a
// word is the kernel's own: a row-source object, see unpack_rows below.
//
// pgm_unpack_kernel (pgm_unpack.hip) has the same launch shape and is NOT this loop, on purpose: it keeps two words of a
// lane in flight, addresses bytes and not pixels, and is not __restrict__ because its `out` may be the payload itself.
#pragma once
#include <stdint.h>

#include "png_filter.h"

namespace mrg {

constexpr int kUnpackLanes = 256;
constexpr int kUnpackWorkgroupsPerCu = 8;  // eight workgroups of 256 lanes fill a CU

// the 16-byte words that a row of `width` samples of ES bytes touches when it begins ph bytes behind a boundary
template <int ES>
MRG_PNG_HD int unpack_row_words(int ph, int width) {
    return (ph + width * ES + 15) >> 4;
}

// word k of such a row: the pixels [x0, x0 + *n) of it, 1 <= *n <= 16 / ES; the value is x0
template <int ES>
MRG_PNG_HD int unpack_word(int ph, int width, int k, int* n) {
    int x0 = (16 * k - ph) / ES, hi = x0 + 16 / ES;  // (16k - ph < 0 only with k == 0: x0 becomes 0 either way)
    if (x0 < 0) x0 = 0;
    if (hi > width) hi = width;
    *n = hi - x0;
    return x0;
}

// the most words of a row of row_bytes_out destination bytes: one more where a row can begin inside a word
inline int unpack_max_row_words(long long row_bytes_out, bool aligned) { return (int)((row_bytes_out + 15) / 16) + (aligned ? 0 : 1); }

// The launch: the lanes of a row are the power of two that covers its words, the workgroups are sized to the device.
struct UnpackShape {
    int lpr_shift;
    long long blocks;
};
inline UnpackShape unpack_shape(int cus, bool aligned, long long row_bytes_out, long long nrows) {
    const int kmax = unpack_max_row_words(row_bytes_out, aligned);
    UnpackShape sh{0, 0};
    while ((1 << sh.lpr_shift) < kmax && (1 << sh.lpr_shift) < kUnpackLanes) ++sh.lpr_shift;
    const int rows_per_block = kUnpackLanes >> sh.lpr_shift;
    sh.blocks = (nrows + rows_per_block - 1) / rows_per_block;
    if (sh.blocks > (long long)cus * kUnpackWorkgroupsPerCu) sh.blocks = (long long)cus * kUnpackWorkgroupsPerCu;
    return sh;
}

#if defined(__HIPCC__)
// The loop.  `source.row(f, y)`, once per row, gives what the pixel text needs of row y of frame f (base, limit, row
// offset; BMP: the flipped row and the frame's table); `.pixels(x0, n, d)` on that, once per word, fills d with the
// samples [x0, x0 + n) as the *_pixels.h texts pack them.  `out` must not alias anything the source reads.
template <int ES, class Source>
__device__ __forceinline__ void unpack_rows(const Source& source, int width, int height, long long nrows, uint8_t* __restrict__ out,
                                            long long frame_pitch_b, long long stride_b, int lpr_shift) {
    static_assert(ES == 1 || ES == 2, "bytes of a destination sample");
    constexpr int NP = 16 / ES;
    const int lanes = 1 << lpr_shift, l = (int)threadIdx.x & (lanes - 1), sub = (int)threadIdx.x >> lpr_shift;
    const long long rows_per_step = (long long)gridDim.x * (kUnpackLanes >> lpr_shift);
    for (long long row = (long long)blockIdx.x * (kUnpackLanes >> lpr_shift) + sub; row < nrows; row += rows_per_step) {
        const long long f = row / height;
        const int y = (int)(row - f * height);
        const auto src = source.row(f, y);
        uint8_t* dst = out + f * frame_pitch_b + (long long)y * stride_b;
        const int ph = (int)((uintptr_t)dst & 15);
        const int K = unpack_row_words<ES>(ph, width);
        for (int k = l; k < K; k += lanes) {
            int n;
            const int x0 = unpack_word<ES>(ph, width, k, &n);
            uint32_t d[4];
            src.pixels(x0, n, d);
            uint8_t* o = dst + (long long)x0 * ES;
            if (n == NP) {
                *(uint4*)o = make_uint4(d[0], d[1], d[2], d[3]);
            } else if (ES == 2) {
#pragma unroll
                for (int p = 0; p < 7; ++p)
                    if (p < n) ((uint16_t*)o)[p] = (uint16_t)(d[p >> 1] >> (16 * (p & 1)));
            } else {
#pragma unroll
                for (int p = 0; p < 15; ++p)
                    if (p < n) o[p] = (uint8_t)(d[p >> 2] >> (8 * (p & 3)));
            }
        }
    }
}
#endif

}  // namespace mrg
