// Stand-alone driver of the host Netpbm reader for tests/test_pnm_io.py: built with -fsanitize=address,undefined together
// with the host readers (tests/host_program.py), it walks a corpus of good, broken and mutated files
//   corpus file: u32 count, then per case u32 length + bytes (little endian)
// through mrg::pnm_header (the whole file, and its first 4096 bytes with the file's size, as probe_image sees it) and, by
// way of a scratch file, mrg::read_image and mrg::probe_image, which must agree with it.  Every P4 / P7 file that is
// readable then goes through csrc/pnm_pixels.h -- the text the kernel runs -- with its raster copied into a heap buffer of
// EXACTLY the payload's size padded to 16 bytes (what the device holds), every row at every first pixel a destination
// phase can ask for, and the samples are compared with read_image's at their own depth.  Prints
// "cases N readable M rows R"; any sanitizer report ends it with a failure.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "image_io.h"
#include "pnm_pixels.h"

static bool get_u32(FILE* f, uint32_t* v) {
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    *v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s corpus.bin scratch-file\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint32_t count = 0;
    if (!f || !get_u32(f, &count)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    unsigned readable = 0;
    unsigned long rows_walked = 0;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t len = 0;
        if (!get_u32(f, &len)) return 2;
        // exactly `len` bytes on the heap: one byte read past them is a report
        std::vector<uint8_t> data(len);
        if (len && fread(data.data(), 1, len, f) != len) return 2;
        mrgingham_amd_pnm_info pi;
        memset(&pi, 0, sizeof(pi));
        const int head = mrg::pnm_header(data.data(), data.size(), data.size(), &pi);
        const bool is_pnm = len >= 2 && data[0] == 'P' && (data[1] == '4' || data[1] == '7');
        const bool ok = head == 0 && len >= 8;  // (read_image and probe_image look at no file below 8 bytes)
        {
            // the first bytes alone, in a buffer of their own: what the probe and the loader hand to the parser
            std::vector<uint8_t> front(data.begin(), data.begin() + (len < 4096 ? len : 4096));
            mrgingham_amd_pnm_info p2;
            memset(&p2, 0, sizeof(p2));
            const int h2 = mrg::pnm_header(front.data(), front.size(), data.size(), &p2);
            // (a header that is longer than the first bytes asks for more)
            if (h2 != head && !(h2 == mrg::kPgmHeaderCut && front.size() < data.size())) {
                fprintf(stderr, "case %u: the parser says %d of the first bytes and %d of the file\n", i, h2, head);
                return 3;
            }
            if (h2 == 0 && memcmp(&p2, &pi, sizeof(pi))) { fprintf(stderr, "case %u: two headers of one file\n", i); return 3; }
        }
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        if (len) fwrite(data.data(), 1, len, o);
        fclose(o);
        int w = 0, h = 0, bits = 0, kind = 0;
        const bool probed = mrg::probe_image(argv[2], &w, &h, &bits, &kind);
        const int depth = pi.bits == 16 ? 16 : 8;
        if (is_pnm && (probed != ok || (probed && (kind != 6 || w != pi.width || h != pi.height || bits != depth)))) {
            fprintf(stderr, "case %u: probe_image and pnm_header disagree\n", i);
            return 3;
        }
        mrg::Image im;
        const bool via_file = mrg::read_image(argv[2], im);
        if (is_pnm && (via_file != ok || (via_file && (im.w != pi.width || im.h != pi.height || im.depth != depth ||
                                                       (depth == 8 ? im.px8.size() : im.px16.size()) != (size_t)im.w * im.h)))) {
            fprintf(stderr, "case %u: read_image and pnm_header disagree\n", i);
            return 3;
        }
        readable += is_pnm && via_file;
        if (!is_pnm || !ok) continue;
        if ((size_t)pi.width * pi.height > (1u << 22)) continue;  // (a mutation may ask for more than this program wants to walk)
        // the pixel text on a raster of exactly its padded size
        const size_t need = (size_t)pi.row_bytes * pi.height, padded = (need + 15) & ~(size_t)15;
        std::vector<uint8_t> pay(padded, 0xEE);
        memcpy(pay.data(), data.data() + pi.payload_offset, need);
        const int es = depth / 8, np = 16 / es;
        for (int y = 0; y < pi.height; ++y) {
            ++rows_walked;
            for (int ph = 0; ph < 16; ph += es) {
                // the words of a destination row that begins ph bytes behind a 16-byte boundary (pnm_unpack_kernel)
                for (int k = 0; 16 * k - ph < pi.width * es; ++k) {
                    int x0 = (16 * k - ph) / es, hi = x0 + np;
                    if (x0 < 0) x0 = 0;
                    if (hi > pi.width) hi = pi.width;
                    if (hi <= x0) continue;
                    uint32_t d[4];
                    if (!mrg::pnm_pixels_any(pay.data(), (long long)padded, (long long)y * pi.row_bytes, pi.bits, pi.channels,
                                             pi.black_and_white != 0, x0, hi - x0, d)) {
                        fprintf(stderr, "case %u: a layout the pixel text does not have\n", i);
                        return 3;
                    }
                    for (int p = 0; p < hi - x0; ++p) {
                        const size_t at = (size_t)y * pi.width + x0 + p;
                        const bool same = es == 2 ? (uint16_t)(d[p >> 1] >> (16 * (p & 1))) == im.px16[at]
                                                  : (uint8_t)(d[p >> 2] >> (8 * (p & 3))) == im.px8[at];
                        if (!same) {
                            fprintf(stderr, "case %u: row %d pixel %d at phase %d differs from read_image\n", i, y, x0 + p, ph);
                            return 3;
                        }
                    }
                }
            }
        }
    }
    fclose(f);
    printf("cases %u readable %u rows %lu\n", count, readable, rows_walked);
    return 0;
}
