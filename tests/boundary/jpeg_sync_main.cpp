// Stand-alone driver of the self-synchronising Huffman decoder (csrc/jpeg_huff_sync.h, the text the device kernels
// compile, under the serial schedule of csrc/jpeg.cpp) for tests/test_jpeg_sync.py: built with
// -fsanitize=address,undefined together with csrc/jpeg.cpp, it walks a corpus
//   corpus file: u32 count, then per case u32 length + bytes (little endian)
// of files WITHOUT restart intervals, intact and corrupted, at every subsequence size given on the command line.  Every
// file is decoded by mrg::jpeg_coefficients and, per size, by the schedule: round 0, update rounds until one changes
// nothing (at most as many as there are subsequences), the scan, the write pass.  Required per file and size:
//   - the schedule accepts the file exactly when jpeg_coefficients does, and then gives the same int16 values;
//   - one more update round over the converged records changes none of them (the fixed point);
//   - with "cap" in front of the sizes: mrg::jpeg_sync_decode with the measured round count as its cap agrees, and with
//     one round less reports -3.
// Prints "cases N accepted M" and writes one text line per case to the second argument: "1" or "0" (accepted), then the
// round count at every size.  Any disagreement (exit 3) or sanitizer report ends it with a failure.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jpeg.h"

static bool get_u32(FILE* f, uint32_t* v) {
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    *v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    return true;
}

static bool same_records(const std::vector<mrg::JpegSyncRecord>& a, const std::vector<mrg::JpegSyncRecord>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!mrg::jpeg_sync_same(a[i], b[i]) || a[i].entry != b[i].entry || a[i].blocks != b[i].blocks) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s corpus.bin result.txt [cap] SUBSEQUENCE...\n", argv[0]); return 2; }
    const bool cap = !strcmp(argv[3], "cap");
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "w");
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
        fprintf(o, "%d", (int)host);
        for (int a = cap ? 4 : 3; a < argc; ++a) {
            const int S = atoi(argv[a]);
            mrg::JpegSyncState st;
            int rounds = -1;
            int rc = mrg::jpeg_sync_begin(data.data(), data.size(), S, &st);
            if (rc == -3) { fprintf(stderr, "case %u: restart intervals\n", i); return 2; }
            std::vector<int16_t> got;
            if (rc == 0) {
                rounds = 0;
                while (mrg::jpeg_sync_round(&st))
                    if (++rounds > (int)st.nsub) { fprintf(stderr, "case %u S %d: more rounds than subsequences\n", i, S); return 3; }
                const std::vector<mrg::JpegSyncRecord> fixed = st.cur;
                if (mrg::jpeg_sync_round(&st) || !same_records(fixed, st.cur)) { fprintf(stderr, "case %u S %d: not a fixed point\n", i, S); return 3; }
                got.assign((size_t)st.scan.info.blocks_w * st.scan.info.blocks_h * 64, 0x5A5A);
                rc = mrg::jpeg_sync_finish(st, got.data(), got.size(), 0);
            }
            if ((rc == 0) != host) { fprintf(stderr, "case %u S %d: schedule %d, jpeg_coefficients %d\n", i, S, rc, (int)host); return 3; }
            if (host && got != want) { fprintf(stderr, "case %u S %d: coefficients differ\n", i, S); return 3; }
            if (cap && rounds >= 0) {  // the one-call form and the cap
                std::vector<int16_t> again(got.size(), 0x5A5A);
                int r2 = -7;
                size_t nsub = 0;
                const int rc2 = mrg::jpeg_sync_decode(data.data(), data.size(), S, rounds, again.data(), again.size(), 0, &info, &r2, &nsub);
                if (rc2 != rc || r2 != rounds || nsub != st.nsub || (rc == 0 && again != want)) { fprintf(stderr, "case %u S %d: jpeg_sync_decode %d rounds %d\n", i, S, rc2, r2); return 3; }
                if (rounds > 0 && mrg::jpeg_sync_decode(data.data(), data.size(), S, rounds - 1, again.data(), again.size(), 0, &info, &r2, &nsub) != -3) {
                    fprintf(stderr, "case %u S %d: converged below its round count\n", i, S);
                    return 3;
                }
            }
            fprintf(o, " %d", host ? rounds : -1);
        }
        fputc('\n', o);
        accepted += host;
    }
    fclose(f);
    fclose(o);
    printf("cases %u accepted %u\n", count, accepted);
    return 0;
}
