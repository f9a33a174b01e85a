// Stand-alone driver of the host half of the colour frames for tests/test_colour.py: built with
// -fsanitize=address,undefined together with the host readers (tests/host_program.py).  Every shape, format and sample
// width, the frame of random samples in a heap buffer of EXACTLY the bytes the arguments describe -- from the first sample
// to the last one -- that ends where the allocation ends and begins at each of the 16 byte phases of a 16-byte word (dense
// rows at the even phases, rows with a stride of their own at the odd ones; the output at phase 5*p + 3), and the output
// in such a buffer too: colour_pixels.h loads the dwords that hold a word's source bytes and cuts the last one at the
// limit, and one byte read or written outside either buffer is a report.
//   mrgingham_amd_colour_grey_image against a decoder that walks the definition of include/mrgingham_amd.h pixel by pixel
//   (not through colour_pixels.h);
//   the argument errors, which must write nothing.
// Prints "frames N pixels P refused R"; any sanitizer report ends it with a failure.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "image_io.h"

static uint32_t rng_state = 2463534242u;
static uint32_t rng() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

struct Frame {
    const uint8_t* base;
    int es, format, w, h;
    long long stride, plane_pitch;
    // sample at element offset e
    uint32_t at(long long e) const {
        const uint8_t* p = base + e * es;
        return es == 1 ? p[0] : (uint32_t)p[0] | ((uint32_t)p[1] << 8);
    }
    // channel c (0 R, 1 G, 2 B) of pixel (y, x), formats 0 .. 5
    uint32_t channel(int y, int x, int c) const {
        const int k = (format & 1) ? 2 - c : c;  // B G R orders
        if (format >= 4) return at(k * plane_pitch + (long long)y * stride + x);
        return at((long long)y * stride + (long long)x * (format >= 2 ? 4 : 3) + k);
    }
    uint32_t grey(int y, int x) const {
        if (format >= 6) return at((long long)y * stride + 2ll * x + (format == 7 ? 1 : 0));
        return (4899u * channel(y, x, 0) + 9617u * channel(y, x, 1) + 1868u * channel(y, x, 2) + 8192u) >> 14;
    }
};

static int row_samples(int format) { return format < 2 ? 3 : format < 4 ? 4 : format < 6 ? 1 : 2; }

int main() {
    static const int shapes[][2] = {{1, 1}, {1, 2}, {2, 3}, {3, 5}, {5, 15}, {4, 16}, {9, 17}, {3, 31}, {4, 33}, {70, 33}, {33, 130}, {2, 300}};
    unsigned long frames = 0, pixels = 0, refused = 0;
    for (const auto& sh : shapes)
        for (int format = 0; format < 8; ++format)
            for (int es = 1; es <= (format < 6 ? 2 : 1); ++es)
                for (int start = 0; start < 16; ++start) {
                    const int h = sh[0], w = sh[1], bits = 8 * es, rs = row_samples(format), ostart = (5 * start + 3) % 16;
                    const long long stride = start & 1 ? (long long)rs * w + 3 : (long long)rs * w, ostride = start & 1 ? w + 2 : w;
                    const long long pp = format == 4 || format == 5 ? h * stride + (start & 1 ? 5 : 0) : 0;
                    const size_t nin = (size_t)(2 * pp + (h - 1) * stride + (long long)rs * w) * es, nout = (size_t)((h - 1) * ostride + w) * es;
                    // exactly those bytes behind `start` bytes, to the end of each allocation
                    uint8_t* hin = (uint8_t*)malloc(start + nin);
                    uint8_t* hout = (uint8_t*)malloc(ostart + nout);
                    if (!hin || !hout) return 2;
                    uint8_t *in = hin + start, *out = hout + ostart;
                    for (size_t i = 0; i < nin; ++i) in[i] = (uint8_t)rng();
                    memset(out, 0xA5, nout);
                    const int bad[] = {
                        mrgingham_amd_colour_grey_image(nullptr, bits, format, w, h, stride, pp, out, ostride),
                        mrgingham_amd_colour_grey_image(in, bits, format, w, h, stride, pp, nullptr, ostride),
                        mrgingham_amd_colour_grey_image(in, bits, 8, w, h, stride, pp, out, ostride),
                        mrgingham_amd_colour_grey_image(in, bits, -1, w, h, stride, pp, out, ostride),
                        mrgingham_amd_colour_grey_image(in, format < 6 ? 12 : 16, format, w, h, stride, pp, out, ostride),
                        mrgingham_amd_colour_grey_image(in, bits, format, w, 32768, stride, pp, out, ostride),
                        mrgingham_amd_colour_grey_image(in, bits, format, w, h, (long long)rs * w - 1, pp, out, ostride),
                        mrgingham_amd_colour_grey_image(in, bits, format, w, h, stride, pp, out, w - 1),
                    };
                    for (int rc : bad) {
                        if (rc != MRGINGHAM_AMD_ERR_ARG) { fprintf(stderr, "an argument error returned %d\n", rc); return 3; }
                        ++refused;
                    }
                    for (size_t i = 0; i < nout; ++i)
                        if (out[i] != 0xA5) { fprintf(stderr, "an argument error wrote\n"); return 3; }
                    if (mrgingham_amd_colour_grey_image(in, bits, format, w, h, stride, pp, out, ostride) != 0) {
                        fprintf(stderr, "format %d %d bits %dx%d: refused\n", format, bits, w, h);
                        return 3;
                    }
                    const Frame m{in, es, format, w, h, stride, pp};
                    for (int y = 0; y < h; ++y)
                        for (long long x = 0; x < ostride && (y < h - 1 || x < w); ++x) {
                            const uint8_t* p = out + ((long long)y * ostride + x) * es;
                            const uint32_t got = es == 1 ? p[0] : (uint32_t)p[0] | ((uint32_t)p[1] << 8);
                            const uint32_t exp = x < w ? m.grey(y, (int)x) : (es == 1 ? 0xA5u : 0xA5A5u);
                            if (got != exp) {
                                fprintf(stderr, "format %d %d bits %dx%d start %d: row %d sample %lld is %u, not %u\n", format, bits, w, h, start, y, x,
                                        got, exp);
                                return 3;
                            }
                            pixels += x < w;
                        }
                    free(hin);
                    free(hout);
                    ++frames;
                }
    printf("frames %lu pixels %lu refused %lu\n", frames, pixels, refused);
    return 0;
}
