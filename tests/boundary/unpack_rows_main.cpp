// The word arithmetic and the launch shape of the unpack kernels (csrc/unpack_rows.h) on the host, stand-alone, for the
// address and undefined-behaviour sanitizers: which pixels word k of a destination row holds, for every phase of the row
// against the 16-byte words, and how many lanes and workgroups a launch gets, against the formula written out here.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "unpack_rows.h"

using namespace mrg;

static long checks = 0;
#define REQUIRE(c)                                                                                         \
    do {                                                                                                   \
        ++checks;                                                                                          \
        if (!(c)) {                                                                                        \
            fprintf(stderr, "%s:%d: %s (ES %d ph %d width %d k %d)\n", __FILE__, __LINE__, #c, ES, ph, width, k); \
            exit(1);                                                                                       \
        }                                                                                                  \
    } while (0)

template <int ES>
static long words_of_rows() {
    long nwords = 0;
    for (int width = 1; width <= 70; ++width) {
        int most = 0, ph = 0, k = -1;
        const int row_bytes = width * ES;
        for (ph = 0; ph < 16; ph += ES) {  // (a 16-bit frame is 2-byte aligned: even phases only)
            const int K = unpack_row_words<ES>(ph, width);
            REQUIRE(K >= 1);
            // the launch shape gives a row the power of two of lanes that covers kmax words: an aligned launch has ph 0 in
            // every row and exactly kmax words, any other at most kmax (below: and some phase reaches it)
            REQUIRE(K <= unpack_max_row_words(row_bytes, false));
            if (ph == 0) REQUIRE(K == unpack_max_row_words(row_bytes, true));
            if (K > most) most = K;
            std::vector<int> owner((size_t)width, -1);  // (heap: a range outside the row is the sanitizer's)
            int next = 0;
            for (k = 0; k < K; ++k, ++nwords) {
                int n = 0;
                const int x0 = unpack_word<ES>(ph, width, k, &n);
                REQUIRE(x0 == next);  // ascending, disjoint, without a gap
                REQUIRE(n >= 1 && n <= 16 / ES);
                REQUIRE(x0 + n <= width);
                if (n == 16 / ES) REQUIRE((ph + x0 * ES) % 16 == 0);  // what the 16-byte store rests on
                for (int x = x0; x < x0 + n; ++x) owner[(size_t)x] = k;
                next = x0 + n;
            }
            REQUIRE(next == width);  // the whole row
            for (int x = 0; x < width; ++x) REQUIRE(owner[(size_t)x] >= 0);
        }
        // ... unless the row is one sample into a word: its last phase fills the first word and needs no further one
        ph = k = -1;
        REQUIRE(most == unpack_max_row_words(row_bytes, false) - (row_bytes % 16 >= 1 && row_bytes % 16 <= ES ? 1 : 0));
    }
    return nwords;
}

// the launch shape written out step by step: lanes per row from the most words of a row, workgroups capped per CU
static void shape_direct(int cus, bool aligned, long long row_bytes, long long nrows, int* lpr_shift, long long* blocks) {
    const int kmax = (int)((row_bytes + 15) / 16) + (aligned ? 0 : 1);
    int s = 0;
    while ((1 << s) < kmax && (1 << s) < 256) ++s;
    const int rows_per_block = 256 >> s;
    long long b = (nrows + rows_per_block - 1) / rows_per_block;
    if (b > (long long)cus * 8) b = (long long)cus * 8;
    *lpr_shift = s;
    *blocks = b;
}

int main() {
    const long w1 = words_of_rows<1>(), w2 = words_of_rows<2>();
    long shapes = 0;
    const int ES = 0, ph = 0, k = 0;  // (for REQUIRE's message)
    const long long rows[] = {1, 255, 256, 257, 1000000};
    const int widths[] = {1, 15, 16, 17, 32, 33, 70, 255, 256, 257, 4080, 4096, 4097, 8192, 32767, 65534};  // bytes of a row
    for (int cus : {1, 256})
        for (long long nrows : rows)
            for (int width : widths)
                for (int aligned = 0; aligned < 2; ++aligned, ++shapes) {
                    int s;
                    long long b;
                    shape_direct(cus, aligned != 0, width, nrows, &s, &b);
                    const UnpackShape sh = unpack_shape(cus, aligned != 0, width, nrows);
                    REQUIRE(sh.lpr_shift == s && sh.blocks == b);
                    REQUIRE(sh.lpr_shift >= 0 && sh.lpr_shift <= 8 && sh.blocks >= 1 && sh.blocks <= (long long)cus * kUnpackWorkgroupsPerCu);
                }
    static_assert(kUnpackLanes == 256 && kUnpackWorkgroupsPerCu == 8, "the *_unpack_geometry answers");
    printf("words8 %ld words16 %ld shapes %ld checks %ld\n", w1, w2, shapes, checks);
    return 0;
}
