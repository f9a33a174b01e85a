// The chunking policy of mrgingham_amd_find_boards_files as a function of its own (mrgingham_amd_files_plan), host only
// and free of every other header of the library, so that a stand-alone program can include it
// (tests/boundary/files_plan_main.cpp).
//
// key[i] >= 0: file i can share a chunk with the files of the same key (same frame size); key[i] < 0: the file is not
// batched (chunk_of_file[i] = slot_in_chunk[i] = -1).  Chunks are created in this order: the next chunk belongs to the
// key of the LOWEST-INDEX file not yet placed, and takes that key's next batch_frames files in list order (fewer when
// the key runs out).  Consequences:
//   - inside a key the files keep their list order, across chunks and inside one;
//   - chunk c holds the lowest-index batched file that chunks 0 .. c-1 left unplaced.  So when chunks are completed in
//     order, every completion moves the first unfinished batched file to the right: the files known to be final form a
//     prefix of the list that grows with every chunk and never shrinks (what the progress callback reports).
// Returns 0, or -1 (nothing written) for nfiles < 0, batch_frames < 1 or a NULL pointer that would be written through.
#pragma once
#include <stdint.h>

#include <unordered_map>
#include <vector>

namespace mrg {

inline int files_plan(const int32_t* key, int nfiles, int batch_frames, int32_t* chunk_of_file, int32_t* slot_in_chunk,
                      int32_t* nchunks) {
    if (nfiles < 0 || batch_frames < 1 || !nchunks || (nfiles > 0 && (!key || !chunk_of_file || !slot_in_chunk))) return -1;
    // next_same[i]: the next file of i's key, nfiles at the end of the key's list
    std::vector<int32_t> next_same((size_t)nfiles, nfiles);
    {
        std::unordered_map<int32_t, int32_t> last;  // key -> its last file so far
        for (int i = 0; i < nfiles; ++i) {
            chunk_of_file[i] = slot_in_chunk[i] = -1;
            if (key[i] < 0) continue;
            auto it = last.find(key[i]);
            if (it != last.end()) {
                next_same[(size_t)it->second] = i;
                it->second = i;
            } else {
                last.emplace(key[i], i);
            }
        }
    }
    int32_t c = 0;
    for (int lo = 0; lo < nfiles; ++lo) {
        if (key[lo] < 0 || chunk_of_file[lo] >= 0) continue;
        // lo is the lowest-index file not yet placed, hence the first unplaced file of its key
        int32_t slot = 0;
        for (int i = lo; i < nfiles && slot < batch_frames; i = next_same[(size_t)i]) {
            chunk_of_file[i] = c;
            slot_in_chunk[i] = slot++;
        }
        ++c;
    }
    *nchunks = c;
    return 0;
}

}  // namespace mrg
