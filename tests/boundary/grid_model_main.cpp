// The host model of the device grid finder (csrc/grid_model.cpp over csrc/grid_phases.h) stand-alone, for the address and
// undefined-behaviour sanitizers: batches of candidate lists read from a file -- the corpus of tests/grid_cases.py as
// tests/test_find_grids_model.py writes it, then lists of random garbage -- through mrgingham_amd_find_grids_host, every
// list's inputs and outputs on the heap at their exact sizes, so that a read behind a list or a write behind its indices is
// the sanitizer's.  Prints every status; the test compares them with the library's.
//
// file: batches of { int32 nlists, capacity, gridn, guard_bits; int32 counts[nlists]; int32 xy[nlists][capacity][2] }
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../include/mrgingham_amd.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <batches>\n", argv[0]);
        return 2;
    }
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    long nbatches = 0, nall = 0, by_status[7] = {0, 0, 0, 0, 0, 0, 0};  // 1, 0, -1 .. -5
    int32_t head[4];
    while (fread(head, sizeof(int32_t), 4, fp) == 4) {
        const int nlists = head[0], capacity = head[1], gridn = head[2], guard_bits = head[3];
        if (nlists < 0 || nlists > (1 << 20) || capacity < 0 || capacity > (1 << 16)) {
            fprintf(stderr, "bad batch header\n");
            return 2;
        }
        std::vector<int32_t> counts((size_t)nlists), xy((size_t)nlists * capacity * 2);
        if (fread(counts.data(), sizeof(int32_t), counts.size(), fp) != counts.size() ||
            fread(xy.data(), sizeof(int32_t), xy.size(), fp) != xy.size()) {
            fprintf(stderr, "short batch\n");
            return 2;
        }
        // one call per list, over copies of exactly its candidates and exactly its gridn^2 indices
        printf("batch %ld gridn %d:", nbatches, gridn);
        for (int l = 0; l < nlists; ++l) {
            const int32_t c = counts[l];
            const size_t keep = c < 0 ? 0 : (c > capacity ? (size_t)capacity : (size_t)c);
            const std::unique_ptr<int32_t[]> one(new int32_t[keep * 2]);  // (never NULL, also with nothing in it)
            memcpy(one.get(), xy.data() + (size_t)l * capacity * 2, keep * 2 * sizeof(int32_t));
            std::vector<int32_t> index((size_t)gridn * gridn, 12345);
            int32_t status = 99;
            // (capacity is what the list claims, keep what it has: a count above the capacity must be declined unread)
            const int rc = mrgingham_amd_find_grids_host(one.get(), &c, 1, capacity, gridn, guard_bits, index.data(), &status);
            if (rc != 0 || status > 1 || status < -5) {
                fprintf(stderr, "batch %ld list %d: rc %d status %d\n", nbatches, l, rc, (int)status);
                return 1;
            }
            for (int32_t v : index)
                if (status == 1 ? (v < 0 || v >= c) : v != -1) {
                    fprintf(stderr, "batch %ld list %d: status %d with index %d of %d\n", nbatches, l, (int)status, (int)v, (int)c);
                    return 1;
                }
            printf(" %d", (int)status);
            ++by_status[1 - status];
            ++nall;
        }
        printf("\n");
        ++nbatches;
    }
    fclose(fp);
    printf("lists %ld found %ld none %ld declined %ld %ld %ld %ld %ld\n", nall, by_status[0], by_status[1], by_status[2], by_status[3],
           by_status[4], by_status[5], by_status[6]);
    return 0;
}
