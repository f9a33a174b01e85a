// Shared arithmetic of the two 16-bit preprocessing paths (preprocess16.hip, preprocess16_batch.hip): the CLI's 16-bit
// branch, mrgingham-from-image.cc:85-92 -- cv::normalize(0, 65535, NORM_MINMAX), CLAHE(8) on 16 bits (65 536 bins, 8 x 8
// tiles), convertTo(CV_8U, 255/65535).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrg {
namespace pre16 {

constexpr int kTiles16 = 8, kBins16 = 65536;

__device__ __forceinline__ int reflect101_16(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

__device__ __forceinline__ unsigned sat_rint(float v, float hi) {  // saturate_cast<>(cvRound(v)): round half to even
    const float r = __builtin_rintf(v);
    return (unsigned)(r < 0.f ? 0.f : (r > hi ? hi : r));
}

// the tile grid of OpenCV's CLAHE: both sides padded by 8 - size % 8 as soon as one of them is ragged (the padding is
// sampled with BORDER_REFLECT_101)
struct Geom16 {
    int w, h, ew, eh, tw, th;
};
inline Geom16 geom16(int w, int h) {
    Geom16 g{w, h, w, h, 0, 0};
    if (w % kTiles16 != 0 || h % kTiles16 != 0) {
        g.ew = w + (kTiles16 - w % kTiles16);
        g.eh = h + (kTiles16 - h % kTiles16);
    }
    g.tw = g.ew / kTiles16;
    g.th = g.eh / kTiles16;
    return g;
}
// clip count of a tile for OpenCV's clip limit
inline int clip16(double clip_limit, long long area) {
    int clip = 0;
    if (clip_limit > 0.0) {
        clip = (int)(clip_limit * (double)area / kBins16);
        if (clip < 1) clip = 1;
    }
    return clip;
}

// cv::normalize(.., 0, 65535, NORM_MINMAX) of a frame with extrema (smin, smax) as convertTo(CV_16U, a, b): the double
// scale / shift, then single-precision multiply and add (no contraction) and cvRound
struct NormMap16 {
    float a, b;
    __device__ __forceinline__ NormMap16(unsigned smin, unsigned smax) {
        const double dmin = smin, dmax = smax;
        const double scale = 65535.0 * (dmax - dmin > 2.220446049250313e-16 ? 1.0 / (dmax - dmin) : 0.0);
        const double shift = 0.0 - dmin * scale;
        a = (float)scale;
        b = (float)shift;
    }
    __device__ __forceinline__ unsigned operator()(unsigned v) const {
        return sat_rint(__fadd_rn(__fmul_rn((float)v, a), b), 65535.f);
    }
};

}  // namespace pre16
}  // namespace mrg
