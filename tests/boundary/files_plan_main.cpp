// The chunking policy of mrgingham_amd_find_boards_files (mrgingham_amd/csrc/files_plan.h) as a stand-alone host
// program, built with -fsanitize=address,undefined by tests/test_files_plan.py: seeded random key lists and chunk
// sizes, every property of the plan checked on each.  Exit status 0 and "ok <cases>" on stdout, or 1 and the first
// property that failed on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <vector>

#include "files_plan.h"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {  // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) % n);
}

#define REQUIRE(cond, what)                                                                            \
    do {                                                                                               \
        if (!(cond)) {                                                                                 \
            fprintf(stderr, "case %d (n %d, batch %d): %s\n", icase, n, batch, what);                  \
            return false;                                                                              \
        }                                                                                              \
    } while (0)

static bool check(int icase, const std::vector<int32_t>& key, int batch) {
    const int n = (int)key.size();
    // (exactly n entries, no slack: a write past the end is the sanitizer's to find)
    std::vector<int32_t> chunk((size_t)n, -7), slot((size_t)n, -7);
    int32_t nchunks = -7;
    REQUIRE(mrg::files_plan(key.data(), n, batch, chunk.data(), slot.data(), &nchunks) == 0, "the plan failed");
    REQUIRE(nchunks >= 0, "negative chunk count");
    std::vector<std::vector<int>> members((size_t)nchunks);
    for (int i = 0; i < n; ++i) {
        if (key[(size_t)i] < 0) {
            REQUIRE(chunk[(size_t)i] == -1 && slot[(size_t)i] == -1, "a file with a negative key was placed");
            continue;
        }
        REQUIRE(chunk[(size_t)i] >= 0 && chunk[(size_t)i] < nchunks, "a batched file has no chunk");
        members[(size_t)chunk[(size_t)i]].push_back(i);
    }
    std::map<int32_t, int> last_of_key;  // the last file of the key placed so far: order inside a key
    int prefix = 0;                      // the first batched file that the chunks so far have not placed
    std::vector<char> placed((size_t)n, 0);
    auto skip = [&]() { while (prefix < n && (key[(size_t)prefix] < 0 || placed[(size_t)prefix])) ++prefix; };
    skip();
    for (int c = 0; c < nchunks; ++c) {
        const std::vector<int>& m = members[(size_t)c];
        REQUIRE(!m.empty() && (int)m.size() <= batch, "a chunk is empty or longer than the batch");
        // every slot 0 .. size-1 exactly once, ascending with the list index
        for (size_t k = 0; k < m.size(); ++k) {
            REQUIRE(slot[(size_t)m[k]] == (int32_t)k, "slots are not the files of the chunk in list order");
            REQUIRE(key[(size_t)m[k]] == key[(size_t)m[0]], "a chunk mixes keys");
        }
        // creation order: the chunk belongs to the key of the lowest-index file not yet placed, and begins with that file
        REQUIRE(m[0] == prefix, "the chunk does not begin with the lowest-index file not yet placed");
        // ... and takes that key's NEXT files: none of the key between the last one placed and these, none skipped inside
        const int32_t k0 = key[(size_t)m[0]];
        int from = last_of_key.count(k0) ? last_of_key[k0] + 1 : 0;
        size_t at = 0;
        for (int i = from; i < n && at < m.size(); ++i)
            if (key[(size_t)i] == k0) {
                REQUIRE(m[at] == i, "the chunk skips a file of its key");
                ++at;
            }
        REQUIRE(at == m.size(), "the chunk holds a file of its key out of order");
        if ((int)m.size() < batch)
            for (int i = m.back() + 1; i < n; ++i) REQUIRE(key[(size_t)i] != k0, "a short chunk left files of its key behind");
        last_of_key[k0] = m.back();
        for (int i : m) placed[(size_t)i] = 1;
        // the final prefix: it grows with every chunk, and never shrinks
        const int before = prefix;
        skip();
        REQUIRE(prefix > before, "completing a chunk did not move the prefix of final files");
    }
    REQUIRE(prefix == n, "files are left over after the last chunk");
    return true;
}

int main(int argc, char** argv) {
    const int ncases = argc > 1 ? atoi(argv[1]) : 2000;
    int done = 0;
    // the fixed shapes first: empty, batch 1, batch >= n, one key, all negative
    const std::vector<int32_t> fixed[] = {{}, {5}, {-1}, {-1, -3, -2}, {4, 4, 4, 4, 4}, {1, 2, 1, 2, 1, 2, -1, 3}, {0, 2147483647, 0, 2147483647}};
    for (const auto& k : fixed)
        for (int batch : {1, 2, 3, 5, 8, 1000}) {
            if (!check(done, k, batch)) return 1;
            ++done;
        }
    for (int c = 0; c < ncases; ++c) {
        const int n = (int)rnd(70), nkeys = 1 + (int)rnd(6), negatives = (int)rnd(4);
        std::vector<int32_t> key((size_t)n);
        for (int32_t& k : key) k = negatives && rnd(8) == 0 ? -1 - (int32_t)rnd(3) : (int32_t)(rnd((uint32_t)nkeys) * 1000003u % 2147483647u);
        const int batch = rnd(4) == 0 ? n + (int)rnd(3) + 1 : 1 + (int)rnd(9);
        if (!check(done, key, batch)) return 1;
        ++done;
    }
    // bad arguments: refused, nothing written
    {
        int32_t k[2] = {1, 1}, ch[2] = {-7, -7}, sl[2] = {-7, -7}, nc = -7;
        if (mrg::files_plan(k, 2, 0, ch, sl, &nc) == 0 || mrg::files_plan(k, -1, 2, ch, sl, &nc) == 0 ||
            mrg::files_plan(nullptr, 2, 2, ch, sl, &nc) == 0 || mrg::files_plan(k, 2, 2, ch, sl, nullptr) == 0 || ch[0] != -7 ||
            sl[1] != -7 || nc != -7) {
            fprintf(stderr, "bad arguments were accepted, or something was written\n");
            return 1;
        }
    }
    printf("ok %d\n", done);
    return 0;
}
