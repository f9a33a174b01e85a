// Stand-alone driver of the host half of the Bayer mosaics for tests/test_bayer.py: built with
// -fsanitize=address,undefined together with the host readers (tests/host_program.py).  Every shape, pattern and sample width,
// the mosaic of random samples in a heap buffer of EXACTLY the bytes the arguments describe -- (height-1)*stride + width
// samples -- that ends where the allocation ends and begins at each of the four byte phases of a dword (dense rows at the
// even phases, rows with a stride of their own at the odd ones), and the output in such a buffer too: bayer_pixels.h
// takes whole words with one 16-byte copy and the ends of a row sample by sample, and one byte read or written outside
// either buffer is a report.
//   mrgingham_amd_bayer_grey_image against a decoder that walks the definition of include/mrgingham_amd.h pixel by pixel
//   (not through bayer_pixels.h);
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

static int reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

struct Mosaic {
    const uint8_t* base;
    int es, w, h;
    long long stride;
    uint32_t at(int y, int x) const {
        const uint8_t* p = base + ((long long)reflect(y, h) * stride + reflect(x, w)) * es;
        return es == 1 ? p[0] : (uint32_t)p[0] | ((uint32_t)p[1] << 8);
    }
};

// 'R', 'G', 'B' at (y, x): the pattern names the colours of (0,0), (0,1), (1,0), (1,1)
static char colour(int pattern, int y, int x) {
    static const char* names[4] = {"RGGB", "GRBG", "GBRG", "BGGR"};
    return names[pattern][2 * (y & 1) + (x & 1)];
}

static uint32_t grey_of(const Mosaic& m, int pattern, int y, int x) {
    const uint32_t cR = 4899, cG = 9617, cB = 1868;
    const uint32_t v = m.at(y, x), hor = m.at(y, x - 1) + m.at(y, x + 1), ver = m.at(y - 1, x) + m.at(y + 1, x);
    const uint32_t diag = m.at(y - 1, x - 1) + m.at(y - 1, x + 1) + m.at(y + 1, x - 1) + m.at(y + 1, x + 1);
    switch (colour(pattern, y, x)) {
        case 'R': return (4 * cR * v + cG * (hor + ver) + cB * diag + 32768) >> 16;
        case 'B': return (4 * cB * v + cG * (hor + ver) + cR * diag + 32768) >> 16;
    }
    return colour(pattern, y, x + 1) == 'R' ? (2 * cG * v + cR * hor + cB * ver + 16384) >> 15 : (2 * cG * v + cB * hor + cR * ver + 16384) >> 15;
}

int main() {
    static const int shapes[][2] = {{2, 2}, {2, 3}, {3, 2}, {5, 3}, {3, 15}, {3, 16}, {3, 17}, {4, 31}, {4, 32}, {4, 33}, {9, 17}, {70, 33},
                                    {2, 300}, {33, 130}};
    unsigned long frames = 0, pixels = 0, refused = 0;
    for (const auto& sh : shapes)
        for (int pattern = 0; pattern < 4; ++pattern)
            for (int es = 1; es <= 2; ++es)
                for (int start = 0; start < 4; ++start) {
                    const int h = sh[0], w = sh[1], bits = 8 * es;
                    const long long stride = start & 1 ? w + 3 : w, ostride = start & 1 ? w + 2 : w;
                    const size_t nin = (size_t)((h - 1) * stride + w) * es, nout = (size_t)((h - 1) * ostride + w) * es;
                    // exactly those bytes behind `start` bytes, to the end of each allocation
                    uint8_t* hin = (uint8_t*)malloc(start + nin);
                    uint8_t* hout = (uint8_t*)malloc(start + nout);
                    if (!hin || !hout) return 2;
                    uint8_t *in = hin + start, *out = hout + start;
                    for (size_t i = 0; i < nin; ++i) in[i] = (uint8_t)rng();
                    memset(out, 0xA5, nout);
                    const int bad[] = {
                        mrgingham_amd_bayer_grey_image(nullptr, bits, w, h, stride, pattern, out, ostride),
                        mrgingham_amd_bayer_grey_image(in, bits, w, h, stride, pattern, nullptr, ostride),
                        mrgingham_amd_bayer_grey_image(in, bits, w, h, stride, 4, out, ostride),
                        mrgingham_amd_bayer_grey_image(in, bits, w, h, stride, -1, out, ostride),
                        mrgingham_amd_bayer_grey_image(in, 12, w, h, stride, pattern, out, ostride),
                        mrgingham_amd_bayer_grey_image(in, bits, 1, h, stride, pattern, out, ostride),
                        mrgingham_amd_bayer_grey_image(in, bits, w, 1, stride, pattern, out, ostride),
                        mrgingham_amd_bayer_grey_image(in, bits, w, 32768, stride, pattern, out, ostride),
                        mrgingham_amd_bayer_grey_image(in, bits, w, h, w - 1, pattern, out, ostride),
                        mrgingham_amd_bayer_grey_image(in, bits, w, h, stride, pattern, out, w - 1),
                    };
                    for (int rc : bad) {
                        if (rc != MRGINGHAM_AMD_ERR_ARG) { fprintf(stderr, "an argument error returned %d\n", rc); return 3; }
                        ++refused;
                    }
                    for (size_t i = 0; i < nout; ++i)
                        if (out[i] != 0xA5) { fprintf(stderr, "an argument error wrote\n"); return 3; }
                    if (mrgingham_amd_bayer_grey_image(in, bits, w, h, stride, pattern, out, ostride) != 0) {
                        fprintf(stderr, "pattern %d %d bits %dx%d: refused\n", pattern, bits, w, h);
                        return 3;
                    }
                    const Mosaic m{in, es, w, h, stride};
                    for (int y = 0; y < h; ++y)
                        for (long long x = 0; x < ostride && (y < h - 1 || x < w); ++x) {
                            const uint8_t* p = out + ((long long)y * ostride + x) * es;
                            const uint32_t got = es == 1 ? p[0] : (uint32_t)p[0] | ((uint32_t)p[1] << 8);
                            const uint32_t exp = x < w ? grey_of(m, pattern, y, (int)x) : (es == 1 ? 0xA5u : 0xA5A5u);
                            if (got != exp) {
                                fprintf(stderr, "pattern %d %d bits %dx%d start %d: row %d sample %lld is %u, not %u\n", pattern, bits, w, h, start, y, x,
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
