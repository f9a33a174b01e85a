// Stand-alone driver of the host half of the PNG device route for tests/test_png_scanlines.py: built with
// -fsanitize=address,undefined together with the host readers (tests/host_program.py), it walks a corpus of good, crafted and
// cut-off PNG files
//   corpus file: u32 count, then per case u32 length + bytes (little endian)
// through mrg::png_scanlines -- sizes only, then into a heap buffer of exactly the reported size (one byte more would be
// an overflow the sanitizer reports), then into one that is a byte short -- and, by way of a scratch file, through
// mrg::read_image, whose verdict must be the same.  Prints "cases N taken M not_taken K"; a disagreement or any
// sanitizer report ends it with a failure.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "image_io.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s corpus.bin scratch-file\n", argv[0]); return 2; }
    std::vector<uint8_t> blob;
    if (!mrg::read_file(argv[1], blob) || blob.size() < 4) { fprintf(stderr, "no corpus\n"); return 2; }
    auto u32 = [&](size_t p) { return (uint32_t)blob[p] | (uint32_t)blob[p + 1] << 8 | (uint32_t)blob[p + 2] << 16 | (uint32_t)blob[p + 3] << 24; };
    const uint32_t count = u32(0);
    size_t p = 4;
    int taken = 0, not_taken = 0;
    for (uint32_t i = 0; i < count; ++i) {
        if (p + 4 > blob.size()) return 2;
        const uint32_t len = u32(p);
        p += 4;
        if (p + len > blob.size()) return 2;
        std::vector<uint8_t> data(blob.begin() + p, blob.begin() + p + len);  // (a buffer of its own: reads behind it are reports)
        p += len;
        int w = 0, h = 0, bits = 0, ct = -1;
        const int head = mrg::png_scanlines(data.data(), data.size(), nullptr, 0, &w, &h, &bits, &ct);
        int verdict = head;
        if (head == 0) {
            const int ch = ct == 0 ? 1 : ct == 2 ? 3 : ct == 4 ? 2 : 4;
            const size_t need = ((size_t)w * ch * bits / 8 + 1) * h;
            std::vector<uint8_t> scan(need), shorter(need - 1);
            verdict = mrg::png_scanlines(data.data(), data.size(), scan.data(), scan.size(), &w, &h, &bits, &ct);
            if (mrg::png_scanlines(data.data(), data.size(), shorter.data(), shorter.size(), &w, &h, &bits, &ct) != -2) {
                fprintf(stderr, "case %u: a buffer one byte short was not refused\n", i);
                return 1;
            }
        }
        FILE* f = fopen(argv[2], "wb");
        if (!f) return 2;
        if (!data.empty()) fwrite(data.data(), 1, data.size(), f);
        fclose(f);
        mrg::Image im;
        const bool readable = mrg::read_image(argv[2], im);
        if (readable != (verdict == 0 || verdict == mrg::kPngNotTaken)) {
            fprintf(stderr, "case %u: png_scanlines says %d, read_image %d\n", i, verdict, (int)readable);
            return 1;
        }
        taken += verdict == 0;
        not_taken += verdict == mrg::kPngNotTaken;
    }
    printf("cases %u taken %d not_taken %d\n", count, taken, not_taken);
    return 0;
}
