// Stand-alone driver of the per-interval Huffman decoder (csrc/jpeg_huff_lane.h, the text the device kernel compiles) for
// tests/test_jpeg_scan.py: built with -fsanitize=address,undefined together with csrc/jpeg.cpp, it walks a corpus
//   corpus file: u32 count, then per case u32 length + bytes (little endian)
// of files with restart intervals, intact and corrupted.  Every file is decoded twice: by mrg::jpeg_coefficients, and
// interval by interval -- mrg::jpeg_scan, then mrg::jpeg_huff_lane over each interval in REVERSE order (the intervals
// are independent), each interval's bytes copied into a heap block of exactly its size (at the alignment it has in the
// file: the decoder reads whole dwords and must ignore what lies outside).  Required: the interval-wise decode accepts
// exactly when jpeg_coefficients does, and then gives the same int16 values, both with whole blocks written over a
// poisoned buffer and with the non-zero values alone stored into a zeroed one.
// Prints "cases N accepted M" and writes one byte per case (1 accepted, 0 not) to the second argument; any disagreement
// (exit 3) or sanitizer report ends it with a failure.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "jpeg.h"
#include "jpeg_huff_lane.h"

static const uint8_t kNatural[64] = {MRG_JPEG_NATURAL_ORDER};

static bool get_u32(FILE* f, uint32_t* v) {
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    *v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    return true;
}

// the interval-wise decode of a scanned file into coef [blocks_h][blocks_w][64]
template <bool kWholeBlocks>
static bool by_intervals(const std::vector<uint8_t>& data, const mrg::JpegScan& sc, int16_t* coef) {
    mrg::JpegHuffTable tables[mrg::kJpegLaneTables];
    mrg::JpegLaneGeom g;
    memset(&g, 0, sizeof(g));
    int ntables = 0;
    const mrg::JpegHuffTable* seen[mrg::kJpegLaneTables] = {};
    for (int c = 0; c < sc.ncomp; ++c)
        for (int ac = 0; ac < 2; ++ac) {
            const mrg::JpegHuffTable* t = ac ? &sc.ac[sc.ta[c]] : &sc.dc[sc.td[c]];
            int s = 0;
            while (s < ntables && seen[s] != t) ++s;
            if (s == ntables) { seen[ntables] = t; tables[ntables++] = *t; }
            g.slots |= (uint32_t)s << (4 * (ac ? 4 + c : c));
        }
    g.ncomp = sc.ncomp;
    g.H0 = sc.comp_h[0];
    g.V0 = sc.comp_v[0];
    g.mcus_x = sc.mcus_x;
    for (int c = 0; c < sc.ncomp; ++c) g.nblk |= (uint32_t)(sc.comp_h[c] * sc.comp_v[c]) << (8 * c);
    g.blocks_h = sc.info.blocks_h;
    g.pitch_blocks = sc.info.blocks_w;
    const size_t n = sc.intervals.size() / 2, nmcu = (size_t)sc.mcus_x * sc.mcus_y;
    bool ok = true;
    for (size_t i = n; i-- > 0;) {
        const size_t begin = (size_t)sc.intervals[2 * i], end = (size_t)sc.intervals[2 * i + 1];
        if (begin > end || end > data.size()) return false;
        const size_t lead = begin & 3;
        std::vector<uint8_t> piece(lead + (end - begin));
        if (end > begin) memcpy(piece.data() + lead, data.data() + begin, end - begin);
        const size_t first = i * sc.restart_interval, left = nmcu - first;
        // (a failed interval does not stop the others: on the device they all run)
        ok &= mrg::jpeg_huff_lane<kWholeBlocks>(piece.data(), (uint32_t)lead, (uint32_t)piece.size(), tables, kNatural, g, (uint32_t)first,
                                                (uint32_t)(left < sc.restart_interval ? left : sc.restart_interval), i + 1 == n, coef);
    }
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s corpus.bin accepted.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    uint32_t count = 0;
    if (!f || !o || !get_u32(f, &count)) { fprintf(stderr, "cannot read %s or write %s\n", argv[1], argv[2]); return 2; }
    unsigned accepted = 0;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t len = 0;
        if (!get_u32(f, &len)) return 2;
        std::vector<uint8_t> data(len);  // exactly `len` bytes on the heap: one byte read past them is a report
        if (len && fread(data.data(), 1, len, f) != len) return 2;
        mrg::JpegInfo info;
        std::vector<int16_t> want;
        bool host = mrg::jpeg_coefficients(data.data(), data.size(), nullptr, 0, 0, &info) == 0;
        if (host) {
            want.assign((size_t)info.blocks_w * info.blocks_h * 64, 0x5A5A);
            host = mrg::jpeg_coefficients(data.data(), data.size(), want.data(), want.size(), 0, &info) == 0;
        }
        mrg::JpegScan sc;
        bool lanes = mrg::jpeg_scan(data.data(), data.size(), &sc) == 0;
        if (lanes && sc.restart_interval == 0) { fprintf(stderr, "case %u: no restart interval\n", i); return 2; }
        if (lanes) {
            if (sc.intervals.size() / 2 != ((size_t)sc.mcus_x * sc.mcus_y + sc.restart_interval - 1) / sc.restart_interval) return 3;
            std::vector<int16_t> whole((size_t)sc.info.blocks_w * sc.info.blocks_h * 64, 0x5A5A), sparse(whole.size(), 0);
            const bool a = by_intervals<true>(data, sc, whole.data()), b = by_intervals<false>(data, sc, sparse.data());
            if (a != b) { fprintf(stderr, "case %u: the two variants disagree\n", i); return 3; }
            lanes = a;
            if (lanes && host && (whole != want || sparse != want)) { fprintf(stderr, "case %u: coefficients differ\n", i); return 3; }
        }
        if (lanes != host) { fprintf(stderr, "case %u: intervals %d, jpeg_coefficients %d\n", i, (int)lanes, (int)host); return 3; }
        accepted += host;
        fputc(host ? 1 : 0, o);
    }
    fclose(f);
    fclose(o);
    printf("cases %u accepted %u\n", count, accepted);
    return 0;
}
