// Stand-alone driver of the tiled TIFF reader for tests/test_tiff_tiles.py: built with -fsanitize=address,undefined together
// with the host readers (tests/host_program.py), it walks a corpus of good, broken, truncated and mutated tiled files
//   corpus file: u32 count, then per case u32 length + bytes (little endian)
// through mrg::tiff_layout_tiled (counts only, then into an array of exactly the reported size and into one a record short,
// with the limits of the device route off and on), and, by way of a scratch file, mrg::probe_image and mrg::read_image.
// Every buffer has exactly the size it is said to have: one byte read or written past it is a report.  No verdict may
// differ between probe_image and the parser at header level, and mrg::tiff_layout_ex must go on calling every tiled file
// unreadable.  Prints "cases N layouts L tiled T readable M"; any sanitizer report ends it with a failure.
#include <stdio.h>
#include <string.h>

#include <vector>

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
    unsigned layouts = 0, tiled = 0, readable = 0;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t len = 0;
        if (!get_u32(f, &len)) return 2;
        std::vector<uint8_t> data(len);
        if (len && fread(data.data(), 1, len, f) != len) return 2;
        mrgingham_amd_tiff_info ti{};
        size_t ns = 0;
        int32_t tw = -1, tl = -1;
        const int head = mrg::tiff_layout_tiled(data.data(), data.size(), 0, 0, &ti, &tw, &tl, nullptr, 0, &ns);
        const bool header_ok = head == 0 || head == mrg::kTiffNotTaken;
        if (header_ok) {
            ++layouts;
            if ((tw == 0) != (tl == 0) || tw < 0 || tl < 0 || tw > 32767 || tl > 32767) return 3;
            tiled += tw > 0;
            // (a mutation may ask for more records than this program wants to hold)
            if (ns <= (1u << 22)) {
                std::vector<mrgingham_amd_tiff_strip> recs(ns), fewer(ns > 1 ? ns - 1 : 0);
                int32_t a = 0, b = 0;
                if (ns > 1 && mrg::tiff_layout_tiled(data.data(), data.size(), 0, 0, &ti, &a, &b, fewer.data(), ns - 1, &ns) != -2) return 3;
                if (mrg::tiff_layout_tiled(data.data(), data.size(), 0, 0, &ti, &a, &b, recs.data(), ns, &ns) != head || a != tw || b != tl) return 3;
                // the device route's limits on: the same records, 0 only where the route takes the file
                std::vector<mrgingham_amd_tiff_strip> again(ns);
                const int dev = mrg::tiff_layout_tiled(data.data(), data.size(), 4096, 4096, &ti, &a, &b, again.data(), ns, &ns);
                if ((dev != 0 && dev != mrg::kTiffNotTaken) || (ns && memcmp(recs.data(), again.data(), ns * sizeof(recs[0])))) return 3;
                if (dev == 0 && tw % 16 != 0) return 3;
                const size_t across = tw ? ((size_t)ti.width + tw - 1) / tw : 1;
                for (size_t k = 0; k < ns; ++k) {
                    const mrgingham_amd_tiff_strip& st = recs[k];
                    if (st.offset < 0 || st.nbytes < 0 || (size_t)st.offset > data.size() || (size_t)st.nbytes > data.size() - (size_t)st.offset) return 3;
                    if (tw && (st.rows != tl || st.first_row != (int32_t)(k / across) * tl)) return 3;
                }
            }
            // the strip parsers: a tiled file stays unreadable to them, a strip file reads as before
            const int strip_head = mrg::tiff_layout_ex(data.data(), data.size(), 0, 0, nullptr, nullptr, 0, nullptr);
            if (tw > 0 ? strip_head != -1 : strip_head != head) return 3;
        } else if (mrg::tiff_layout_ex(data.data(), data.size(), 0, 0, nullptr, nullptr, 0, nullptr) >= 0) {
            return 3;
        }
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        if (len) fwrite(data.data(), 1, len, o);
        fclose(o);
        int w = 0, h = 0, bits = 0, kind = 0;
        const bool probed = mrg::probe_image(argv[2], &w, &h, &bits, &kind);
        if (probed != header_ok || (probed && (kind != 4 || w != ti.width || h != ti.height || bits != ti.bits))) {
            fprintf(stderr, "case %u: probe_image and tiff_layout_tiled disagree\n", i);
            return 3;
        }
        mrg::Image im;
        const bool via_file = mrg::read_image(argv[2], im);
        if (via_file && (!header_ok || im.w != ti.width || im.h != ti.height || im.depth != ti.bits ||
                         (ti.bits == 8 ? im.px8.size() : im.px16.size()) != (size_t)im.w * im.h)) {
            fprintf(stderr, "case %u: read_image took what the parser refuses, or gave another size\n", i);
            return 3;
        }
        if (header_ok && ti.compression == 1 && !via_file) {
            fprintf(stderr, "case %u: an uncompressed file the parser accepts, read_image refuses\n", i);
            return 3;
        }
        readable += via_file;
    }
    fclose(f);
    printf("cases %u layouts %u tiled %u readable %u\n", count, layouts, tiled, readable);
    return 0;
}
