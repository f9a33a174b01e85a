// PNG row filters and the colour-to-grey weights, one text for the host decoder (image_io.cpp: decode_png) and the device
// kernel (png_recon.hip), like jpeg_idct8.h.  A reconstructed byte is (filtered + predictor) mod 256, the predictor taken
// from a = the byte one pixel (bpp bytes) to the left, b = the byte above and c = the byte above a; whatever lies outside
// the image is 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRG_PNG_HD __host__ __device__ inline
#else
#define MRG_PNG_HD inline
#endif

namespace mrg {

constexpr int kPngFilters = 5;  // None, Sub, Up, Average, Paeth: a filter byte above 4 makes the file unreadable

// the one of a, b, c nearest to a + b - c; ties in the order a, b, c
MRG_PNG_HD int png_paeth(int a, int b, int c) {
    const int pa = b - c, pb = a - c, pc = pa + pb;
    const int xa = pa < 0 ? -pa : pa, xb = pb < 0 ? -pb : pb, xc = pc < 0 ? -pc : pc;
    return (xa <= xb && xa <= xc) ? a : (xb <= xc ? b : c);
}

// the predictor of filter type ft (0 .. 4), by branches: the host decoder's loop, where ft changes once per row
MRG_PNG_HD int png_predict(int ft, int a, int b, int c) {
    switch (ft) {
        case 1: return a;
        case 2: return b;
        case 3: return (a + b) >> 1;
        case 4: return png_paeth(a, b, c);
        default: return 0;
    }
}

// the same values by selection: the lanes of a wave hold rows of different filter types, and five short selects cost
// less than five diverged paths
MRG_PNG_HD int png_predict_select(int ft, int a, int b, int c) {
    int p = ft == 1 ? a : 0;
    p = ft == 2 ? b : p;
    p = ft == 3 ? (a + b) >> 1 : p;
    p = ft == 4 ? png_paeth(a, b, c) : p;
    return p;
}

// grey of an RGB sample triple, 8 or 16 bit: fixed-point BT.601 (image_io.h)
MRG_PNG_HD uint32_t png_grey(uint32_t r, uint32_t g, uint32_t b) { return (r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14; }

// bytes between a byte and its left neighbour: colour types 0, 2, 4, 6 at 8 or 16 bit (0: no such combination; the
// palette type 3 has 1 at 8 bit and is the host decoder's alone)
MRG_PNG_HD int png_bpp(int bits, int color_type) {
    if (bits != 8 && bits != 16) return 0;
    const int ch = color_type == 0 ? 1 : color_type == 2 ? 3 : color_type == 4 ? 2 : color_type == 6 ? 4 : 0;
    return ch * bits / 8;
}

}  // namespace mrg
