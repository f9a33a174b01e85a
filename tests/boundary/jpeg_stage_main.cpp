// Stand-alone driver of the staging-image builders of the device entropy decoders (csrc/jpeg_stage.h: plan, lay out,
// fill) for tests/test_jpeg_scan.py: built with -fsanitize=address,undefined together with csrc/jpeg.cpp, it walks a corpus
//   corpus file: u32 count, then per case u32 length + bytes (little endian)
// of readable baseline files, with and without restart intervals, whose LAST FOUR cases are one chunk of their own: a
// file with restart intervals (longer than one MCU), one without, a progressive file and a file of another size.  The
// cases in front are grouped by size into chunks of at most 8, in the block geometry the loader gives the size.  Per
// chunk and subsequence size (8, 32, 128) both images are laid out and filled twice, into heap blocks of exactly `total`
// bytes preset to 00 and to FF.  Required:
//   (a) every region lies inside [0, total), no two overlap, the uploaded ones tile [0, back) and the read-back area
//       begins at back; table and stream offsets are multiples of 4;
//   (b) the two fills agree over [0, back): every uploaded byte is written;
//   (c) every file of the interval route decodes from the image alone -- its HuffFrame, tables and interval records read
//       back out of it, jpeg_huff_lane over every interval in reverse order -- to what jpeg_coefficients gives;
//   (d) every file of the sync route has its tables and stream bytes in the image as in the file, and a SyncFrame that
//       says what jpeg_sync_begin computes for the file at that subsequence size;
//   (e) the last chunk is planned [0 intervals, -3 sync, -1, -2], and [-3, -3, -1, -2] without a route with the sync
//       decoder off and max_interval one below the first file's interval.
// No case in front of the last four may be unreadable or left to the host.  Prints "cases N chunks C intervals I sync Y";
// any violation (exit 3) or sanitizer report ends it with a failure.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "jpeg.h"
#include "jpeg_stage.h"

using namespace mrg;

static const uint8_t kNatural[64] = {MRG_JPEG_NATURAL_ORDER};

#define REQUIRE(cond, ...)                                           \
    do {                                                             \
        if (!(cond)) {                                               \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                            \
            fputc('\n', stderr);                                     \
            exit(3);                                                 \
        }                                                            \
    } while (0)

static bool get_u32(FILE* f, uint32_t* v) {
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    *v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    return true;
}

// the largest block count any sampling gives a side (luma factors 1 .. 4), as the loader pads it
static int padded(int side) {
    int most = 0;
    for (int h = 1; h <= 4; ++h) most = std::max(most, (side + 8 * h - 1) / (8 * h) * h);
    return most;
}

struct Region {
    size_t off, bytes;
    bool uploaded;
};

// (a) for one image
static void check_regions(std::vector<Region> r, size_t back, size_t total, const char* what) {
    size_t uploaded = 0;
    for (const Region& q : r) {
        REQUIRE(q.off <= total && q.bytes <= total - q.off, "%s: region [%zu, +%zu) outside %zu", what, q.off, q.bytes, total);
        REQUIRE(q.uploaded ? q.off + q.bytes <= back : q.off >= back, "%s: region [%zu, +%zu) on the wrong side of %zu", what, q.off, q.bytes, back);
        if (q.uploaded) uploaded += q.bytes;
    }
    std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.off != b.off ? a.off < b.off : a.bytes < b.bytes; });
    for (size_t i = 0; i + 1 < r.size(); ++i)
        REQUIRE(r[i].off + r[i].bytes <= r[i + 1].off, "%s: regions [%zu, +%zu) and [%zu, ..) overlap", what, r[i].off, r[i].bytes, r[i + 1].off);
    REQUIRE(uploaded == back && back <= total, "%s: %zu bytes of regions in an upload of %zu", what, uploaded, back);
}

struct Counts {
    unsigned intervals = 0, sync = 0;
};

// one chunk at one subsequence size; decode: (c) as well
static void check_chunk(const std::vector<const std::vector<uint8_t>*>& datas, int width, int height, uint32_t S, bool decode, bool all_taken,
                        Counts* counts) {
    const int n = (int)datas.size(), bw = padded(width), bh = padded(height);
    std::vector<JpegStageFile> files((size_t)n);
    for (int i = 0; i < n; ++i) {
        files[i].data = datas[i]->data();
        files[i].nbytes = datas[i]->size();
        jpeg_stage_plan(files[i], width, height, bw, bh, 1024, true);
        REQUIRE(!all_taken || files[i].route != JpegRoute::kNone, "file %d of a %d x %d chunk: status %d, no decoder takes it", i, width, height, files[i].status);
        REQUIRE((files[i].route == JpegRoute::kIntervals) == (files[i].status == 0), "file %d: status %d beside its route", i, files[i].status);
    }
    const JpegImageLayout lh = jpeg_huff_lay_out(files.data(), n);
    const JpegSyncLayout ls = jpeg_sync_lay_out(files.data(), n, S);

    // (a)
    std::vector<Region> rh = {{0, (size_t)n * sizeof(HuffFrame), true}, {lh.quant, (size_t)n * 64 * sizeof(uint16_t), true},
                              {lh.items, lh.nitems * 2 * sizeof(uint32_t), true}, {lh.back, lh.total - lh.back, false}};
    std::vector<Region> rs = {{0, (size_t)ls.nfiles * sizeof(SyncFrame), true}, {ls.back, ls.total - ls.back, false}};
    REQUIRE(lh.total - lh.back >= lh.nitems, "%zu status bytes for %zu intervals", lh.total - lh.back, lh.nitems);
    REQUIRE(ls.total - ls.back == (size_t)ls.nfiles * sizeof(SyncWords), "%zu bytes of words for %d files", ls.total - ls.back, ls.nfiles);
    REQUIRE(ls.items == ls.streams && ls.quant == ls.tables, "the sync image has regions of the interval image");
    REQUIRE(ls.d_spec >= (size_t)ls.nfiles * sizeof(SyncWords) && ls.d_spec % 32 == 0 &&
                ls.d_bytes == ls.d_spec + ls.nitems * (3 * sizeof(JpegSyncRecord) + sizeof(JpegSyncStart)),
            "scratch: spec at %zu of %zu", ls.d_spec, ls.d_bytes);
    size_t items_h = 0, items_s = 0;
    int nsync = 0;
    for (int i = 0; i < n; ++i) {
        const JpegStageFile& j = files[i];
        if (j.route == JpegRoute::kNone) continue;
        const bool iv = j.route == JpegRoute::kIntervals;
        REQUIRE(j.table_off % 4 == 0 && j.stream_off % 4 == 0, "file %d: tables at %zu, stream at %zu", i, j.table_off, j.stream_off);
        REQUIRE(j.ntables >= 1 && j.ntables <= kJpegLaneTables, "file %d: %d tables", i, j.ntables);
        (iv ? rh : rs).push_back({j.table_off, (size_t)j.ntables * sizeof(JpegHuffTable), true});
        (iv ? rh : rs).push_back({j.stream_off, jpeg_stage_padded(j.len), true});
        REQUIRE(jpeg_stage_padded(j.len) % 4 == 0 && jpeg_stage_padded(j.len) >= (size_t)j.len + 4, "padding of %u bytes", j.len);
        size_t& items = iv ? items_h : items_s;
        REQUIRE(j.item_first == items, "file %d: its items begin at %zu, not %zu", i, j.item_first, items);
        items += j.nitems;
        if (!iv) REQUIRE(j.index == nsync++ && j.frame == i, "file %d: sync file %d, frame %d", i, j.index, j.frame);
    }
    REQUIRE(items_h == lh.nitems && items_s == ls.nitems && nsync == ls.nfiles, "items: %zu of %zu, %zu of %zu", items_h, lh.nitems, items_s, ls.nitems);
    check_regions(rh, lh.back, lh.total, "interval image");
    check_regions(rs, ls.back, ls.total, "sync image");

    // (b): blocks of exactly `total` bytes, so that one byte past the end is a report
    std::unique_ptr<char[]> h0(new char[lh.total]), h1(new char[lh.total]), s0(new char[ls.total]), s1(new char[ls.total]);
    memset(h0.get(), 0x00, lh.total);
    memset(h1.get(), 0xFF, lh.total);
    memset(s0.get(), 0x00, ls.total);
    memset(s1.get(), 0xFF, ls.total);
    for (int i = 0; i < n; ++i) {
        jpeg_huff_fill(h0.get(), lh.total, lh, files[i], i, bh, bw);
        jpeg_huff_fill(h1.get(), lh.total, lh, files[i], i, bh, bw);
        if (files[i].route != JpegRoute::kSync) continue;
        jpeg_sync_fill(s0.get(), ls.total, ls, files[i], files[i].index, bh, bw);
        jpeg_sync_fill(s1.get(), ls.total, ls, files[i], files[i].index, bh, bw);
    }
    REQUIRE(memcmp(h0.get(), h1.get(), lh.back) == 0, "interval image: an uploaded byte that no fill writes");
    REQUIRE(memcmp(s0.get(), s1.get(), ls.back) == 0, "sync image: an uploaded byte that no fill writes");

    const char* image = h1.get();
    for (int i = 0; i < n; ++i) {
        const JpegStageFile& j = files[i];
        HuffFrame fr;
        memcpy(&fr, image + (size_t)i * sizeof(HuffFrame), sizeof(fr));
        uint16_t quant[64];
        memcpy(quant, image + lh.quant + (size_t)i * sizeof(quant), sizeof(quant));
        if (j.route != JpegRoute::kIntervals) {  // nothing for the kernel, no table for the transform
            const HuffFrame none = {};
            const uint16_t zeros[64] = {};
            REQUIRE(memcmp(&fr, &none, sizeof(fr)) == 0 && memcmp(quant, zeros, sizeof(quant)) == 0, "file %d: a record for a file not taken", i);
        }
        if (j.route == JpegRoute::kIntervals && decode) {  // (c)
            ++counts->intervals;
            REQUIRE(memcmp(quant, j.scan.info.quant, sizeof(quant)) == 0, "file %d: quantisation table", i);
            REQUIRE(fr.nintervals > 0 && fr.ntables == j.ntables && fr.geom.blocks_h == bh && fr.geom.pitch_blocks == bw, "file %d: record", i);
            JpegHuffTable tables[kJpegLaneTables];
            memcpy(tables, image + fr.table_off, (size_t)fr.ntables * sizeof(JpegHuffTable));
            std::vector<int16_t> got((size_t)bw * bh * 64, 0x5A5A), want(got.size(), 0x5A5A);
            JpegInfo info;
            REQUIRE(jpeg_coefficients(j.data, j.nbytes, want.data(), want.size(), bw, &info) == 0, "file %d: the host decoder rejects it", i);
            for (int q = fr.nintervals; q-- > 0;) {
                uint32_t iv[2];
                memcpy(iv, image + lh.items + ((size_t)fr.interval_first + (size_t)q) * sizeof(iv), sizeof(iv));
                const uint32_t first = (uint32_t)q * (uint32_t)fr.restart_interval, left = (uint32_t)fr.nmcu - first;
                REQUIRE(jpeg_huff_lane<true>((const uint8_t*)image + fr.stream_off, iv[0], iv[1], tables, kNatural, fr.geom, first,
                                             std::min(left, (uint32_t)fr.restart_interval), q == fr.nintervals - 1, got.data()),
                        "file %d: interval %d does not decode from the image", i, q);
                REQUIRE((uint8_t)image[lh.back + fr.interval_first + (size_t)q] == 0, "file %d: status byte %d not cleared", i, q);
            }
            REQUIRE(got == want, "file %d: coefficients out of the image differ from the host decoder's", i);
        }
        if (j.route == JpegRoute::kSync) {  // (d)
            if (decode) ++counts->sync;
            const char* simage = s1.get();
            SyncFrame sf;
            memcpy(&sf, simage + (size_t)j.index * sizeof(SyncFrame), sizeof(sf));
            JpegSyncState st;
            const int rc = jpeg_sync_begin(j.data, j.nbytes, (int)S, &st);
            REQUIRE(rc == 0 || (rc == -1 && st.nsub == 0), "file %d: jpeg_sync_begin %d", i, rc);
            REQUIRE(sf.len == st.len && sf.nsub == st.nsub && sf.total == st.total_blocks && sf.frame == (uint32_t)i && sf.rec_first == j.item_first &&
                        sf.stream_off == j.stream_off && sf.table_off == j.table_off,
                    "file %d S %u: SyncFrame len %u nsub %u total %u frame %u", i, S, sf.len, sf.nsub, sf.total, sf.frame);
            REQUIRE(memcmp(simage + sf.stream_off, j.data + j.scan.entropy_begin, sf.len) == 0, "file %d: stream bytes", i);
            if (rc == 0) {
                JpegLaneGeom g = st.geom;  // (jpeg_sync_begin: the file's own block geometry)
                g.blocks_h = bh;
                g.pitch_blocks = bw;
                REQUIRE((int)sf.ntables == st.ntables && memcmp(&sf.geom, &g, sizeof(g)) == 0, "file %d: geometry", i);
                REQUIRE(memcmp(simage + sf.table_off, st.tables, (size_t)st.ntables * sizeof(JpegHuffTable)) == 0, "file %d: tables", i);
            }
        }
    }
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint32_t count = 0;
    if (!f || !get_u32(f, &count) || count < 4) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<std::vector<uint8_t>> cases(count);
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t len = 0;
        if (!get_u32(f, &len)) return 2;
        cases[i].resize(len);
        cases[i].shrink_to_fit();  // exactly `len` bytes on the heap: one byte read past them is a report
        if (len && fread(cases[i].data(), 1, len, f) != len) return 2;
    }
    fclose(f);
    const uint32_t sizes[3] = {8, 32, 128};
    Counts counts;
    unsigned chunks = 0;
    // the cases in front, by size, in chunks of at most 8
    std::vector<bool> done(count - 4, false);
    for (uint32_t i = 0; i + 4 < count; ++i) {
        if (done[i]) continue;
        JpegInfo info;
        REQUIRE(jpeg_coefficients(cases[i].data(), cases[i].size(), nullptr, 0, 0, &info) == 0, "case %u: the host decoder rejects it", i);
        std::vector<const std::vector<uint8_t>*> chunk;
        auto flush = [&]() {
            for (int q = 0; q < 3; ++q) check_chunk(chunk, info.width, info.height, sizes[q], q == 0, true, &counts);
            ++chunks;
            chunk.clear();
        };
        for (uint32_t k = i; k + 4 < count; ++k) {
            JpegInfo other;
            if (done[k] || jpeg_coefficients(cases[k].data(), cases[k].size(), nullptr, 0, 0, &other) != 0 || other.width != info.width ||
                other.height != info.height)
                continue;
            done[k] = true;
            chunk.push_back(&cases[k]);
            if (chunk.size() == 8) flush();
        }
        if (!chunk.empty()) flush();
    }
    // (e) and the mixed chunk through the same checks
    std::vector<const std::vector<uint8_t>*> mixed;
    for (uint32_t i = count - 4; i < count; ++i) mixed.push_back(&cases[i]);
    JpegStageFile m[4];
    for (int i = 0; i < 4; ++i) {
        m[i].data = mixed[i]->data();
        m[i].nbytes = mixed[i]->size();
    }
    JpegInfo info;
    REQUIRE(jpeg_coefficients(m[0].data, m[0].nbytes, nullptr, 0, 0, &info) == 0, "the first file of the mixed chunk is unreadable");
    const int bw = padded(info.width), bh = padded(info.height);
    for (int i = 0; i < 4; ++i) jpeg_stage_plan(m[i], info.width, info.height, bw, bh, 1024, true);
    REQUIRE(m[0].scan.restart_interval >= 2 && m[1].scan.restart_interval == 0, "the mixed chunk: intervals of %u and %u MCUs", m[0].scan.restart_interval,
            m[1].scan.restart_interval);
    REQUIRE(m[0].status == 0 && m[0].route == JpegRoute::kIntervals && m[1].status == -3 && m[1].route == JpegRoute::kSync && m[2].status == -1 &&
                m[2].route == JpegRoute::kNone && m[3].status == -2 && m[3].route == JpegRoute::kNone,
            "the mixed chunk is planned %d %d %d %d", m[0].status, m[1].status, m[2].status, m[3].status);
    printf("mixed %d %d %d %d\n", m[0].status, m[1].status, m[2].status, m[3].status);
    const int below = (int)m[0].scan.restart_interval - 1;
    for (int i = 0; i < 4; ++i) jpeg_stage_plan(m[i], info.width, info.height, bw, bh, below, false);
    for (int i = 0; i < 4; ++i) REQUIRE(m[i].route == JpegRoute::kNone, "file %d of the mixed chunk has a route with both decoders off", i);
    REQUIRE(m[0].status == -3 && m[1].status == -3 && m[2].status == -1 && m[3].status == -2, "the mixed chunk without the decoders is planned %d %d %d %d",
            m[0].status, m[1].status, m[2].status, m[3].status);
    printf("mixed_off %d %d %d %d\n", m[0].status, m[1].status, m[2].status, m[3].status);
    Counts in_mixed;
    for (int q = 0; q < 3; ++q) check_chunk(mixed, info.width, info.height, sizes[q], q == 0, false, &in_mixed);
    REQUIRE(in_mixed.intervals == 1 && in_mixed.sync == 1, "the mixed chunk: %u and %u files decoded", in_mixed.intervals, in_mixed.sync);
    ++chunks;
    printf("cases %u chunks %u intervals %u sync %u\n", count, chunks, counts.intervals, counts.sync);
    return 0;
}
