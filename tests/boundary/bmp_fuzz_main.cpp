// Stand-alone driver of the host BMP reader for tests/test_bmp_io.py: built with -fsanitize=address,undefined together
// with the host readers (tests/host_program.py), it walks a corpus of good, broken and mutated files
//   corpus file: u32 count, then per case u32 length + bytes (little endian)
// through mrg::bmp_layout (the whole file, and its first 4096 bytes with the file's size, as probe_image sees it) and, by
// way of a scratch file, mrg::read_image and mrg::probe_image, which must agree with it.  Every file the device route would
// take then goes row by row through csrc/bmp_pixels.h -- the text the kernel runs -- with each source row copied into a heap
// buffer of EXACTLY the padded row length, at every first pixel a destination phase can ask for, and the bytes are
// compared with read_image's.  Prints "cases N readable M rows R"; any sanitizer report ends it with a failure.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bmp_pixels.h"
#include "image_io.h"

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
        mrgingham_amd_bmp_info bi;
        memset(&bi, 0, sizeof(bi));
        const int head = mrg::bmp_layout(data.data(), data.size(), data.size(), &bi);
        const bool ok = head == 0 || head == mrg::kBmpNotTaken;
        {
            // the first bytes alone, in a buffer of their own: what the probe and the loader hand to the parser
            std::vector<uint8_t> front(data.begin(), data.begin() + (len < 4096 ? len : 4096));
            mrgingham_amd_bmp_info b2;
            memset(&b2, 0, sizeof(b2));
            const int h2 = mrg::bmp_layout(front.data(), front.size(), data.size(), &b2);
            // (an RLE8 stream is judged only by a caller that holds the whole file)
            if (h2 != head && !(h2 == mrg::kBmpNotTaken && head == -1 && front.size() < data.size())) {
                fprintf(stderr, "case %u: the parser says %d of the first bytes and %d of the file\n", i, h2, head);
                return 3;
            }
            if (h2 == 0 && memcmp(&b2, &bi, sizeof(bi))) { fprintf(stderr, "case %u: two layouts of one file\n", i); return 3; }
        }
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        if (len) fwrite(data.data(), 1, len, o);
        fclose(o);
        int w = 0, h = 0, bits = 0, kind = 0;
        const bool probed = mrg::probe_image(argv[2], &w, &h, &bits, &kind);
        const bool is_bmp = len >= 2 && data[0] == 'B' && data[1] == 'M';
        if (is_bmp && (probed != ok || (probed && (kind != 5 || w != bi.width || h != bi.height || bits != 8)))) {
            fprintf(stderr, "case %u: probe_image and bmp_layout disagree\n", i);
            return 3;
        }
        mrg::Image im;
        const bool via_file = mrg::read_image(argv[2], im);
        if (is_bmp && (via_file != ok || (via_file && (im.w != bi.width || im.h != bi.height || im.depth != 8 || im.px8.size() != (size_t)im.w * im.h)))) {
            fprintf(stderr, "case %u: read_image and bmp_layout disagree\n", i);
            return 3;
        }
        readable += is_bmp && via_file;
        if (!is_bmp || head != 0) continue;
        if ((size_t)bi.width * bi.height > (1u << 24)) continue;  // (a mutation may ask for more than this program wants to walk)
        // the pixel text on rows of exactly their padded length
        const uint8_t* lut = bi.bits == 8 && bi.lut_identity ? nullptr : bi.lut;
        for (int y = 0; y < bi.height; ++y) {
            const uint8_t* src = data.data() + bi.payload_offset + (size_t)bi.row_bytes * (size_t)(bi.top_down ? y : bi.height - 1 - y);
            std::vector<uint8_t> row(src, src + bi.row_bytes);
            ++rows_walked;
            for (int ph = 0; ph < 16; ++ph) {
                // the words of a destination row that begins ph bytes behind a 16-byte boundary (bmp_unpack_kernel)
                for (int k = 0; 16 * k - ph < bi.width; ++k) {
                    int x0 = 16 * k - ph, hi = x0 + 16;
                    if (x0 < 0) x0 = 0;
                    if (hi > bi.width) hi = bi.width;
                    if (hi <= x0) continue;
                    uint32_t d[4];
                    mrg::bmp_pixels_any(row.data(), bi.row_bytes, bi.bits, lut, x0, hi - x0, d);
                    for (int p = 0; p < hi - x0; ++p)
                        if ((uint8_t)(d[p >> 2] >> (8 * (p & 3))) != im.px8[(size_t)y * bi.width + x0 + p]) {
                            fprintf(stderr, "case %u: row %d pixel %d at phase %d differs from read_image\n", i, y, x0 + p, ph);
                            return 3;
                        }
                }
            }
        }
    }
    fclose(f);
    printf("cases %u readable %u rows %lu\n", count, readable, rows_walked);
    return 0;
}
