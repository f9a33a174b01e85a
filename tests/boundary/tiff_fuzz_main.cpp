// Stand-alone driver of the host TIFF reader for tests/test_tiff_io.py: built with -fsanitize=address,undefined together
// with the host readers (tests/host_program.py), it walks a corpus of good, broken and mutated files
//   corpus file: u32 count, then per case u32 length + bytes (little endian)
// through mrg::tiff_layout (counts only, then into an array of exactly the reported size and into one a record short),
// the shared strip decoder of csrc/tiff_lzw.h -- with the host's table and with the packed table the kernel uses, the
// output going into a buffer of exactly the strip's size -- and, by way of a scratch file, mrg::read_image and
// mrg::probe_image.  Prints "cases N layouts L readable M lzw_strips S lzw_broken B"; any sanitizer report ends it with a
// failure.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "image_io.h"
#include "tiff_lzw.h"

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
    unsigned layouts = 0, readable = 0, lzw_strips = 0, lzw_broken = 0;
    std::unique_ptr<mrg::TiffLzwHostTable> host_table(new mrg::TiffLzwHostTable);
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t len = 0;
        if (!get_u32(f, &len)) return 2;
        // exactly `len` bytes on the heap: one byte read past them is a report
        std::vector<uint8_t> data(len);
        if (len && fread(data.data(), 1, len, f) != len) return 2;
        mrgingham_amd_tiff_info ti{};
        size_t ns = 0;
        const int head = mrg::tiff_layout(data.data(), data.size(), 0, &ti, nullptr, 0, &ns);
        const bool header_ok = head == 0 || head == mrg::kTiffNotTaken;
        bool strips_ok = header_ok, all_walked = true;
        if (header_ok) {
            ++layouts;
            std::vector<mrgingham_amd_tiff_strip> strips(ns);
            if (ns > 1 && mrg::tiff_layout(data.data(), data.size(), 0, &ti, strips.data(), ns - 1, &ns) != -2) return 3;
            if (mrg::tiff_layout(data.data(), data.size(), 0, &ti, strips.data(), ns, &ns) != head) return 3;
            const size_t rowb = (size_t)ti.width * ti.samples * (ti.bits / 8);
            for (const mrgingham_amd_tiff_strip& st : strips) {
                if (st.offset < 0 || st.nbytes < 0 || (size_t)st.offset > data.size() || (size_t)st.nbytes > data.size() - (size_t)st.offset) return 3;
                if (ti.compression != 5) continue;
                const size_t need = rowb * (size_t)st.rows;
                if (need > (64u << 20)) { all_walked = false; continue; }  // (a mutation may ask for more than this program wants to hold)
                ++lzw_strips;
                // the strip's bytes and its output in buffers of exactly their sizes
                std::vector<uint8_t> src(data.begin() + st.offset, data.begin() + st.offset + st.nbytes), out(need), out2(need);
                const int a = mrg::tiff_lzw_decode(src.data(), (uint32_t)src.size(), out.data(), (uint32_t)need, *host_table);
                if (need <= mrg::kTiffLzwMaxStrip20) {  // the kernel's table and its 20 + 12 bit entries
                    std::vector<uint32_t> words(mrg::kTiffLzwCodes);
                    mrg::TiffLzwPackedTable packed{words.data(), 1};
                    const int b = mrg::tiff_lzw_decode(src.data(), (uint32_t)src.size(), out2.data(), (uint32_t)need, packed);
                    if (a != b || (a == 0 && memcmp(out.data(), out2.data(), need))) {
                        fprintf(stderr, "case %u: the two tables disagree\n", i);
                        return 3;
                    }
                }
                if (a) { ++lzw_broken; strips_ok = false; }
            }
        }
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        if (len) fwrite(data.data(), 1, len, o);
        fclose(o);
        int w = 0, h = 0, bits = 0, kind = 0;
        const bool probed = mrg::probe_image(argv[2], &w, &h, &bits, &kind);
        if (probed != header_ok || (probed && (kind != 4 || w != ti.width || h != ti.height || bits != ti.bits))) {
            fprintf(stderr, "case %u: probe_image and tiff_layout disagree\n", i);
            return 3;
        }
        mrg::Image im;
        const bool via_file = mrg::read_image(argv[2], im);
        if (via_file && (!header_ok || im.w != ti.width || im.h != ti.height || im.depth != ti.bits ||
                         (ti.bits == 8 ? im.px8.size() : im.px16.size()) != (size_t)im.w * im.h))
            return 3;
        if (via_file && !strips_ok && all_walked) { fprintf(stderr, "case %u: read_image took a file with a broken LZW strip\n", i); return 3; }
        if (header_ok && (ti.compression == 1 || ti.compression == 5) && strips_ok && all_walked && !via_file) {
            fprintf(stderr, "case %u: every strip decodes, read_image refuses the file\n", i);
            return 3;
        }
        readable += via_file;
    }
    fclose(f);
    printf("cases %u layouts %u readable %u lzw_strips %u lzw_broken %u\n", count, layouts, readable, lzw_strips, lzw_broken);
    return 0;
}
