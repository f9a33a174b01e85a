// Stand-alone driver of the host JPEG decoder for tests/test_jpeg_io.py: built with -fsanitize=address,undefined together
// with the host readers (tests/host_program.py), it walks a corpus of truncated and corrupted files
//   corpus file: u32 count, then per case u32 length + bytes (little endian)
// through mrg::jpeg_coefficients (header only, then into a buffer of exactly the reported size), mrg::jpeg_idct_host and,
// by way of a scratch file, mrg::read_image.  Prints "cases N readable M"; any sanitizer report ends it with a failure.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "image_io.h"
#include "jpeg.h"

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
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t len = 0;
        if (!get_u32(f, &len)) return 2;
        // exactly `len` bytes on the heap: one byte read past them is a report
        std::vector<uint8_t> data(len);
        if (len && fread(data.data(), 1, len, f) != len) return 2;
        mrg::JpegInfo info;
        const int head = mrg::jpeg_coefficients(data.data(), data.size(), nullptr, 0, 0, &info);
        bool ok = false;
        if (head == 0) {
            std::vector<int16_t> coef((size_t)info.blocks_w * info.blocks_h * 64);
            if (mrg::jpeg_coefficients(data.data(), data.size(), coef.data(), coef.size() - 1, 0, &info) != -2) return 3;
            if (mrg::jpeg_coefficients(data.data(), data.size(), coef.data(), coef.size(), 0, &info) == 0) {
                std::vector<uint8_t> px((size_t)info.width * info.height);
                mrg::jpeg_idct_host(coef.data(), 0, info, px.data());
                ok = true;
            }
        }
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        if (len) fwrite(data.data(), 1, len, o);
        fclose(o);
        mrg::Image im;
        const bool via_file = mrg::read_image(argv[2], im);
        if (via_file != ok) { fprintf(stderr, "case %u: read_image and jpeg_coefficients disagree\n", i); return 3; }
        if (ok && (im.w != info.width || im.h != info.height || im.px8.size() != (size_t)im.w * im.h)) return 3;
        readable += ok;
    }
    fclose(f);
    printf("cases %u readable %u\n", count, readable);
    return 0;
}
