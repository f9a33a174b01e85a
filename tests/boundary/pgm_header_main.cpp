// Stand-alone driver of the PGM header parser for tests/test_pgm_header.py: built with -fsanitize=address,undefined
// together with the host readers (tests/host_program.py).  From one good 16-bit PGM file it makes every truncation and, for
// every byte of the header, a handful of single-byte corruptions; each case goes through mrg::pgm_header in a heap
// buffer of exactly its size (a read behind it is a sanitizer report) and, by way of a scratch file, through
// mrg::read_image and mrg::probe_image, whose verdicts must be the parser's: readable when the header is good and the
// bytes behind it hold the payload.  Prints "cases N readable M cut K"; a disagreement or any sanitizer report ends it
// with a failure.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "image_io.h"

static int one_case(const std::vector<uint8_t>& data, const char* scratch, int* readable_out, int* cut_out) {
    int w = 0, h = 0, bits = 0;
    size_t off = 0;
    const int rc = mrg::pgm_header(data.empty() ? nullptr : data.data(), data.size(), &w, &h, &bits, &off);
    if (rc == 0 && (off > data.size() || (bits != 8 && bits != 16) || w < 1 || h < 1 || w > 32767 || h > 32767)) {
        fprintf(stderr, "a good header with fields out of range: %d x %d, %d bits, offset %zu of %zu\n", w, h, bits, off, data.size());
        return 1;
    }
    const bool readable = rc == 0 && data.size() - off >= (size_t)w * h * (bits / 8);
    FILE* f = fopen(scratch, "wb");
    if (!f) return 2;
    if (!data.empty()) fwrite(data.data(), 1, data.size(), f);
    fclose(f);
    mrg::Image im;
    const bool read = mrg::read_image(scratch, im);
    int pw = 0, ph = 0, pb = 0, pk = 0;
    const bool probed = mrg::probe_image(scratch, &pw, &ph, &pb, &pk);
    // (a case whose first bytes are no longer "P5" may be read as nothing at all: never as an image of another kind here)
    if (read != readable || probed != readable) {
        fprintf(stderr, "pgm_header says %d (readable %d), read_image %d, probe_image %d\n", rc, (int)readable, (int)read, (int)probed);
        return 1;
    }
    if (readable && (im.w != w || im.h != h || im.depth != bits || pw != w || ph != h || pb != bits || pk != 1)) {
        fprintf(stderr, "the three disagree about a readable file\n");
        return 1;
    }
    *readable_out += readable;
    *cut_out += rc == mrg::kPgmHeaderCut;
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s good.pgm scratch-file\n", argv[0]); return 2; }
    std::vector<uint8_t> good;
    if (!mrg::read_file(argv[1], good)) { fprintf(stderr, "no file\n"); return 2; }
    int w = 0, h = 0, bits = 0;
    size_t off = 0;
    if (mrg::pgm_header(good.data(), good.size(), &w, &h, &bits, &off) != 0 || bits != 16 || good.size() - off != (size_t)w * h * 2) {
        fprintf(stderr, "not a good 16-bit PGM with nothing behind its payload\n");
        return 2;
    }
    int cases = 0, readable = 0, cut = 0, rc;
    for (size_t n = 0; n <= good.size(); ++n, ++cases) {  // every truncation (the last one is the whole file)
        const std::vector<uint8_t> data(good.begin(), good.begin() + n);
        if ((rc = one_case(data, argv[2], &readable, &cut))) { fprintf(stderr, "... at truncation %zu\n", n); return rc; }
    }
    static const uint8_t values[] = {0, '\n', ' ', '#', '0', '9', '6', 'P', 0xff};
    for (size_t p = 0; p < off; ++p)
        for (uint8_t v : values) {
            if (good[p] == v) continue;
            std::vector<uint8_t> data(good);
            data[p] = v;
            ++cases;
            if ((rc = one_case(data, argv[2], &readable, &cut))) { fprintf(stderr, "... with byte %zu set to %u\n", p, (unsigned)v); return rc; }
        }
    printf("cases %d readable %d cut %d\n", cases, readable, cut);
    return 0;
}
