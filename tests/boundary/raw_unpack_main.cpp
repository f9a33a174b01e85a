// Stand-alone driver of the host half of the packed camera formats for tests/test_raw_unpack.py: built with
// -fsanitize=address,undefined together with the host readers (tests/host_program.py).  Every format over a list of shapes, at
// the minimum row_bytes, with 3 bytes of row padding and with a few more, the payload of random bytes in a heap buffer of
// EXACTLY nbytes = (height-1)*row_bytes + minimum that ends where the allocation ends (and begins at each of the four
// byte phases of a dword): raw_pixels.h loads aligned dwords, and the guard on the last one -- of which only the bytes
// inside the payload may be touched -- is what this program is there for; one byte read past the buffer is a report.
//   mrgingham_amd_raw_unpack_image against a decoder that walks the definitions of include/mrgingham_amd.h bit by bit;
//   mrg::raw_pixels_any, the text the kernel runs, at every first sample a destination phase can ask for (odd ones in the
//   pair formats, every bit phase in the streams);
//   the argument errors, which must write nothing.
// Prints "frames N multiple4 A other B words W"; any sanitizer report ends it with a failure.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "image_io.h"
#include "raw_pixels.h"

static const int kBits[5] = {10, 12, 14, 10, 12};

static int bit_of(const uint8_t* row, long long b) { return (row[b / 8] >> (b % 8)) & 1; }

// sample x of a row, from the definitions
static uint16_t sample_of(const uint8_t* row, int x, int fmt) {
    const int n = kBits[fmt];
    if (fmt <= MRGINGHAM_AMD_RAW_P14) {
        unsigned v = 0;
        for (int i = 0; i < n; ++i) v |= (unsigned)bit_of(row, (long long)x * n + i) << i;
        return (uint16_t)v;
    }
    const int L = n - 8, g = x / 2;
    const unsigned b0 = row[3 * g], b1 = row[3 * g + 1], b2 = row[3 * g + 2], lm = (1u << L) - 1u;
    return (uint16_t)(x % 2 == 0 ? (b0 << L) | (b1 & lm) : (b2 << L) | ((b1 >> 4) & lm));
}

static uint32_t rng_state = 12345u;
static uint32_t rng() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

int main() {
    static const int shapes[][2] = {{1, 1}, {5, 3}, {9, 17}, {3, 7}, {3, 8}, {3, 9}, {3, 15}, {3, 16}, {3, 17}, {70, 33}, {2, 300},
                                    {1, 2}, {1, 5}, {2, 6}, {4, 11}, {1, 8}, {1, 16}, {7, 64}, {1, 301}};
    static const int pads[] = {0, 3, 1, 2, 16};
    unsigned long frames = 0, mult4 = 0, other = 0, words = 0;
    for (int fmt = 0; fmt < 5; ++fmt)
        for (const auto& sh : shapes)
            for (int pad : pads)
                for (int start = 0; start < 4; ++start) {
                    const int h = sh[0], w = sh[1];
                    const long long rmin = mrgingham_amd_raw_row_bytes(w, fmt), rowb = rmin + pad;
                    if (rmin != mrg::raw_min_row_bytes(w, fmt) || rmin < 1) { fprintf(stderr, "row bytes of %d at format %d\n", w, fmt); return 3; }
                    const size_t nbytes = (size_t)((h - 1) * rowb + rmin);
                    ((long long)h * rowb) % 4 == 0 ? ++mult4 : ++other;
                    // exactly nbytes behind `start` bytes, to the end of the allocation
                    uint8_t* heap = (uint8_t*)malloc(start + nbytes);
                    if (!heap) return 2;
                    uint8_t* pay = heap + start;
                    for (size_t i = 0; i < nbytes; ++i) pay[i] = (uint8_t)rng();
                    const int stride = w + 3;
                    std::vector<uint16_t> out((size_t)h * stride, 0xA5A5), want((size_t)h * w);
                    for (int y = 0; y < h; ++y)
                        for (int x = 0; x < w; ++x) want[(size_t)y * w + x] = sample_of(pay + (size_t)y * rowb, x, fmt);
                    // the argument errors first: nothing may be written
                    const int bad[] = {
                        mrgingham_amd_raw_unpack_image(pay, nbytes - 1, w, h, rowb, fmt, out.data(), stride),
                        mrgingham_amd_raw_unpack_image(pay, nbytes, w, h, rmin - 1, fmt, out.data(), stride),
                        mrgingham_amd_raw_unpack_image(pay, nbytes, w, h, rowb, 5, out.data(), stride),
                        mrgingham_amd_raw_unpack_image(pay, nbytes, w, h, rowb, -1, out.data(), stride),
                        mrgingham_amd_raw_unpack_image(pay, nbytes, w, h, rowb, fmt, out.data(), w - 1),
                        mrgingham_amd_raw_unpack_image(pay, nbytes, 0, h, rowb, fmt, out.data(), stride),
                        mrgingham_amd_raw_unpack_image(pay, nbytes, w, 0, rowb, fmt, out.data(), stride),
                        mrgingham_amd_raw_unpack_image(nullptr, nbytes, w, h, rowb, fmt, out.data(), stride),
                        mrgingham_amd_raw_unpack_image(pay, nbytes, w, h, rowb, fmt, nullptr, stride),
                    };
                    for (int rc : bad)
                        if (rc != MRGINGHAM_AMD_ERR_ARG) { fprintf(stderr, "an argument error returned %d\n", rc); return 3; }
                    for (uint16_t v : out)
                        if (v != 0xA5A5) { fprintf(stderr, "an argument error wrote\n"); return 3; }
                    if (mrgingham_amd_raw_unpack_image(pay, nbytes, w, h, rowb, fmt, out.data(), stride) != 0) {
                        fprintf(stderr, "format %d %dx%d row_bytes %lld: refused\n", fmt, w, h, rowb);
                        return 3;
                    }
                    for (int y = 0; y < h; ++y)
                        for (int x = 0; x < stride; ++x) {
                            const uint16_t got = out[(size_t)y * stride + x], exp = x < w ? want[(size_t)y * w + x] : (uint16_t)0xA5A5;
                            if (got != exp) {
                                fprintf(stderr, "format %d %dx%d row_bytes %lld start %d: row %d sample %d is %u, not %u\n", fmt, w, h, rowb, start, y,
                                        x, got, exp);
                                return 3;
                            }
                        }
                    // the words of a destination row that begins ph bytes behind a 16-byte boundary (raw_unpack_kernel)
                    for (int y = 0; y < h; ++y)
                        for (int ph = 0; ph < 16; ph += 2)
                            for (int k = 0; 16 * k - ph < w * 2; ++k) {
                                int x0 = (16 * k - ph) / 2, hi = x0 + 8;
                                if (x0 < 0) x0 = 0;
                                if (hi > w) hi = w;
                                if (hi <= x0) continue;
                                uint32_t d[4];
                                if (!mrg::raw_pixels_any(pay, (long long)nbytes, (long long)y * rowb, fmt, x0, hi - x0, d)) return 3;
                                ++words;
                                for (int p = 0; p < hi - x0; ++p)
                                    if ((uint16_t)(d[p >> 1] >> (16 * (p & 1))) != want[(size_t)y * w + x0 + p]) {
                                        fprintf(stderr, "format %d %dx%d row_bytes %lld: row %d sample %d at phase %d differs\n", fmt, w, h, rowb, y,
                                                x0 + p, ph);
                                        return 3;
                                    }
                            }
                    free(heap);
                    ++frames;
                }
    if (mrgingham_amd_raw_row_bytes(0, 0) != -1 || mrgingham_amd_raw_row_bytes(32768, 1) != -1 || mrgingham_amd_raw_row_bytes(8, 5) != -1 ||
        mrgingham_amd_raw_row_bytes(8, -1) != -1 || mrgingham_amd_raw_row_bytes(32767, 2) != (32767ll * 14 + 7) / 8)
        return 3;
    printf("frames %lu multiple4 %lu other %lu words %lu\n", frames, mult4, other, words);
    return 0;
}
