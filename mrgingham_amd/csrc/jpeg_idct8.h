// The one-dimensional step of libjpeg's default integer inverse DCT (13-bit constants), ONE text for the host decoder
// (jpeg.cpp) and the device kernel (jpeg_idct.hip): they agree on every input, crafted ones included.  All sums and
// products are taken modulo 2^32 (uint32_t); the descaling shift is an arithmetic shift of the value taken as int32_t.
// A valid stream never wraps, and for it this is libjpeg's arithmetic in `long`.  Pass 1 runs it down the columns of the
// dequantised block with S = 11, pass 2 along the rows of the result with S = 18; the pixel is clamp(x + 128, 0, 255).
// The order of the passes matters: the rounding does not commute.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MRG_JPEG_HD __host__ __device__
#else
#define MRG_JPEG_HD
#endif

namespace mrg {

template <int S>
MRG_JPEG_HD inline void jpeg_idct8(const uint32_t d[8], int32_t out[8]) {
    uint32_t z1 = (d[2] + d[6]) * 4433u;
    const uint32_t t2 = z1 - d[6] * 15137u, t3 = z1 + d[2] * 6270u;
    const uint32_t t0 = (d[0] + d[4]) << 13, t1 = (d[0] - d[4]) << 13;
    const uint32_t e0 = t0 + t3, e3 = t0 - t3, e1 = t1 + t2, e2 = t1 - t2;
    uint32_t o0 = d[7], o1 = d[5], o2 = d[3], o3 = d[1];
    z1 = o0 + o3;
    uint32_t z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    o0 *= 2446u; o1 *= 16819u; o2 *= 25172u; o3 *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
    z3 = z3 * (uint32_t)-16069 + z5;
    z4 = z4 * (uint32_t)-3196 + z5;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    constexpr uint32_t r = 1u << (S - 1);
    out[0] = (int32_t)(e0 + o3 + r) >> S; out[7] = (int32_t)(e0 - o3 + r) >> S;
    out[1] = (int32_t)(e1 + o2 + r) >> S; out[6] = (int32_t)(e1 - o2 + r) >> S;
    out[2] = (int32_t)(e2 + o1 + r) >> S; out[5] = (int32_t)(e2 - o1 + r) >> S;
    out[3] = (int32_t)(e3 + o0 + r) >> S; out[4] = (int32_t)(e3 - o0 + r) >> S;
}

}  // namespace mrg
