// The chunk size of the file-list loaders (mrgingham_amd/csrc/loader.h: loader_chunk_frames) as a stand-alone host
// program, built with -fsanitize=address,undefined by tests/test_files_plan.py: a table worked out by hand from the rule
// (half the budget over the bytes per frame, clamped to [1, nfiles], whole rounds of the host threads, the cap), then
// the rule's properties over seeded random arguments.  Exit status 0 and "ok <cases>" on stdout, or 1 and the first
// case that failed on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "loader.h"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd64() {  // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static uint32_t rnd(uint32_t n) { return (uint32_t)(rnd64() % n); }

// the properties every result has; `fit` is budget / 2 / bytes_per_frame, worked out by the caller
static bool check(const char* what, size_t budget, size_t per_frame, size_t fit, int nfiles, int nthreads, int cap) {
    const int got = mrg::loader_chunk_frames(budget, per_frame, nfiles, nthreads, cap);
    const char* bad = nullptr;
    if (got < 1 || got > nfiles) bad = "outside [1, nfiles]";
    else if (cap > 0 && got > cap) bad = "above the cap";
    else if ((size_t)got > (fit < 1 ? 1 : fit)) bad = "more frames than fit into half the budget";
    else if (got > nthreads && got != cap && got % nthreads) bad = "above nthreads, not the cap and not whole rounds of the threads";
    if (!bad) return true;
    fprintf(stderr, "%s: budget %zu, per frame %zu (fit %zu), nfiles %d, nthreads %d, cap %d -> %d: %s\n", what, budget, per_frame, fit,
            nfiles, nthreads, cap, got, bad);
    return false;
}

int main(int argc, char** argv) {
    const int ncases = argc > 1 ? atoi(argv[1]) : 4000;
    int done = 0;
    // fit, nfiles, nthreads, cap -> chunk
    static const int table[][5] = {{10, 7, 4, 0, 4},   {10, 100, 4, 0, 8}, {0, 5, 4, 0, 1},   {10, 3, 4, 0, 3},  {10, 100, 4, 2, 2},
                                   {100, 100, 16, 0, 96}, {4, 100, 4, 0, 4},  {10, 100, 1, 3, 3}, {10, 100, 4, 9, 8}};
    for (const auto& row : table)
        for (size_t per_frame : {(size_t)1, (size_t)24640, (size_t)25165824}) {
            // a budget that gives exactly this fit: 2 * fit * per_frame, and the same with the remainder that still does
            for (size_t budget : {2 * (size_t)row[0] * per_frame, 2 * (size_t)row[0] * per_frame + 2 * per_frame - 1}) {
                const int got = mrg::loader_chunk_frames(budget, per_frame, row[1], row[2], row[3]);
                if (got != row[4]) {
                    fprintf(stderr, "table: fit %d, nfiles %d, nthreads %d, cap %d -> %d, not %d\n", row[0], row[1], row[2], row[3], got, row[4]);
                    return 1;
                }
                if (!check("table", budget, per_frame, (size_t)row[0], row[1], row[2], row[3])) return 1;
                ++done;
            }
        }
    for (int c = 0; c < ncases; ++c) {
        const int nfiles = 1 + (int)rnd(c % 3 ? 200 : 100000), nthreads = 1 + (int)rnd(32);
        const int cap = rnd(3) == 0 ? 1 + (int)rnd(40) : rnd(5) == 0 ? -1 - (int)rnd(3) : 0;
        size_t budget, per_frame;
        switch (c % 4) {
        case 0:  // the loaders' range: up to 2 GiB over frames of up to 64 MiB
            budget = (size_t)(rnd64() % ((uint64_t)2 << 30));
            per_frame = 1 + (size_t)(rnd64() % ((uint64_t)64 << 20));
            break;
        case 1:  // small numbers: every branch of the clamp
            budget = rnd(400);
            per_frame = 1 + rnd(12);
            break;
        case 2:  // bytes per frame near SIZE_MAX / 2: nothing is multiplied, so nothing overflows
            budget = (size_t)rnd64();
            per_frame = SIZE_MAX / 2 - rnd(1000) + rnd(2000);
            break;
        default:  // anything
            budget = (size_t)rnd64();
            per_frame = 1 + (size_t)(rnd64() >> rnd(64));
        }
        if (!check("random", budget, per_frame, budget / 2 / per_frame, nfiles, nthreads, cap)) return 1;
        ++done;
    }
    printf("ok %d\n", done);
    return 0;
}
