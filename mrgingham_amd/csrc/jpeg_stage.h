// The staging images of the device entropy decoders (jpeg_huff.hip: one lane per restart interval; jpeg_huff_sync.hip:
// files without restart intervals), host only: which decoder takes a scanned file, where every file of a chunk lies in
// the chunk's image, and the bytes it puts there.  Both images are built alike,
//   records (one per file) | [interval image: quantisation tables, 64 uint16 per file] | Huffman tables |
//   [interval image: interval records] | padded streams || read-back area
// everything in front of `back` is uploaded, the read-back area behind it comes back from the device (one status byte
// per interval; one SyncWords per file).  All offsets are bytes into the image.  Nothing here knows the context or HIP:
// tests/boundary/jpeg_stage_main.cpp runs this text under the sanitizers.
#pragma once
#include <assert.h>
#include <string.h>

#include "jpeg.h"

namespace mrg {

// One file of a chunk, as the interval kernel sees it (64 bytes).
struct HuffFrame {
    uint64_t stream_off;      // its entropy-coded bytes (a multiple of 4; padded so that whole dwords can be read)
    uint32_t table_off;       // its ntables tables, JpegHuffTable each
    uint32_t interval_first;  // index of its first interval record and status byte
    int32_t nintervals;       // 0: the device does not take this file
    int32_t restart_interval, nmcu, ntables;
    JpegLaneGeom geom;
};
static_assert(sizeof(HuffFrame) == 64, "HuffFrame is laid out by hand in the staging image");

// One file of a chunk, as the sync kernels see it (80 bytes).
struct SyncFrame {
    uint64_t stream_off;  // its entropy-coded bytes (a multiple of 4; padded so that whole dwords can be read)
    uint32_t table_off;   // its ntables tables, JpegHuffTable each
    uint32_t rec_first;   // index of its first record
    uint32_t nsub, len, total, ntables;
    uint32_t frame;       // which coefficient area of the chunk is its own
    uint32_t unused[3];
    JpegLaneGeom geom;
};
static_assert(sizeof(SyncFrame) == 80, "SyncFrame is laid out by hand in the staging image");

// What the sync kernels keep per file (zeroed in front of round 0, read back behind the write pass).
struct SyncWords {
    uint32_t last_changed;  // the last update round (1 ..) that changed one of its records
    uint32_t flags;         // kReached / kError from the write pass, kScanReached / kNotConverged from the scan
};
constexpr uint32_t kReached = 1, kError = 2, kScanReached = 4, kNotConverged = 8;

// what a stream of len bytes takes in an image: whole dwords, and one more that a lane may read behind its last byte
inline size_t jpeg_stage_padded(size_t len) { return ((len + 3) & ~(size_t)3) + 4; }

enum class JpegRoute { kNone, kIntervals, kSync };  // which device decoder takes a file

// One file of a chunk on the host.
struct JpegStageFile {
    const uint8_t* data = nullptr;
    size_t nbytes = 0;
    JpegScan scan;
    int32_t status = -1;  // as planned: 0 the interval decoder takes it, -1 unreadable, -2 another size, -3 readable but not
                          // for the interval decoder (route kSync: the sync decoder takes it; kNone: the host has to)
    JpegRoute route = JpegRoute::kNone;
    int ntables = 0;
    const JpegHuffTable* tables[kJpegLaneTables] = {};  // (into scan)
    JpegLaneGeom geom;
    uint32_t len = 0;  // of its stream: up to the end of the last interval, or of the segment
    // where it lies in its route's image (jpeg_huff_lay_out, jpeg_sync_lay_out)
    int frame = 0, index = 0;  // route kSync: its place in the chunk (its coefficient area), and among the chunk's sync files
    uint32_t nitems = 0;  // intervals, or subsequences
    size_t item_first = 0, table_off = 0, stream_off = 0;
};

// Plans file j (data, nbytes set) of a chunk whose frames are width x height pixels in areas of blocks_h x blocks_w blocks.
// May throw std::bad_alloc (jpeg_scan).
inline void jpeg_stage_plan(JpegStageFile& j, int width, int height, int blocks_w, int blocks_h, int max_interval, bool sync) {
    j.status = -1;
    j.route = JpegRoute::kNone;
    j.ntables = 0;
    if (!j.data || jpeg_scan(j.data, j.nbytes, &j.scan)) return;
    const JpegScan& sc = j.scan;
    if (sc.info.width != width || sc.info.height != height || sc.info.blocks_w > blocks_w || sc.info.blocks_h > blocks_h) { j.status = -2; return; }
    j.status = -3;
    size_t end;
    if (sc.restart_interval) {
        if (sc.restart_interval > (unsigned)max_interval || j.nbytes >= 0xFFFFFFF0u) return;
        end = (size_t)sc.intervals.back();
        j.route = JpegRoute::kIntervals;
        j.status = 0;
    } else {
        if (!sync) return;
        end = jpeg_segment_end(j.data, j.nbytes, sc.entropy_begin);
        if (end - sc.entropy_begin >= kJpegSyncMaxStream) return;  // (an empty segment is taken: unreadable, as on the host)
        j.route = JpegRoute::kSync;
    }
    j.len = (uint32_t)(end - sc.entropy_begin);
    jpeg_lane_setup(sc, j.tables, &j.ntables, &j.geom, blocks_h, blocks_w);
}

// advances through an image region by region
struct JpegCarver {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t off = at;
        at += bytes;
        return off;
    }
};

struct JpegImageLayout {
    size_t quant = 0, tables = 0, items = 0, streams = 0;
    size_t back = 0, total = 0;  // the upload is [0, back), the read-back area [back, total)
    size_t nitems = 0;           // interval records and status bytes; sync records
    uint32_t most_items = 0;     // of one file
    int nfiles = 0;              // files of the route
};

// The part both images share: nrecords records of record_bytes, extra_bytes of the caller's, then per file of `route`
// (with nitems set) its tables, nitems x item_bytes item records, its padded stream.
inline JpegImageLayout jpeg_stage_lay_out(JpegStageFile* files, int n, JpegRoute route, size_t nrecords, size_t record_bytes,
                                          size_t extra_bytes, size_t item_bytes) {
    JpegImageLayout l;
    JpegCarver c;
    c.take(nrecords * record_bytes);
    l.quant = c.take(extra_bytes);
    l.tables = c.at;
    for (int i = 0; i < n; ++i) {
        JpegStageFile& j = files[i];
        if (j.route != route) continue;
        ++l.nfiles;
        j.table_off = c.take((size_t)j.ntables * sizeof(JpegHuffTable));
        j.item_first = l.nitems;
        l.nitems += j.nitems;
        if (j.nitems > l.most_items) l.most_items = j.nitems;
    }
    l.items = c.take(l.nitems * item_bytes);
    l.streams = c.at;
    for (int i = 0; i < n; ++i)
        if (files[i].route == route) files[i].stream_off = c.take(jpeg_stage_padded(files[i].len));
    l.back = l.total = c.at;
    return l;
}

// The interval image of a chunk of n files: a record and a quantisation table (zeros for a file that is not decoded) for
// EVERY file of the chunk; an interval record is two uint32, [begin, end) relative to the file's stream.
inline JpegImageLayout jpeg_huff_lay_out(JpegStageFile* files, int n) {
    for (int i = 0; i < n; ++i)
        if (files[i].route == JpegRoute::kIntervals) files[i].nitems = (uint32_t)(files[i].scan.intervals.size() / 2);
    JpegImageLayout l = jpeg_stage_lay_out(files, n, JpegRoute::kIntervals, (size_t)n, sizeof(HuffFrame), (size_t)n * 64 * sizeof(uint16_t),
                                           2 * sizeof(uint32_t));
    l.total = l.back + ((l.nitems + 3) & ~(size_t)3);
    return l;
}

// The sync image of the chunk's sync files, numbered in order, at S bytes per subsequence; the records of the rounds
// live on the device alone, in a scratch buffer: words | spec | two record buffers | starts.
struct JpegSyncLayout : JpegImageLayout {
    size_t d_spec = 0, d_bytes = 0;  // in the scratch buffer: where `spec` begins, and its size
};
inline JpegSyncLayout jpeg_sync_lay_out(JpegStageFile* files, int n, uint32_t S) {
    int nsync = 0;
    for (int i = 0; i < n; ++i) {
        if (files[i].route != JpegRoute::kSync) continue;
        files[i].frame = i;
        files[i].index = nsync++;
        files[i].nitems = (files[i].len + S - 1) / S;
    }
    JpegSyncLayout l;
    static_cast<JpegImageLayout&>(l) = jpeg_stage_lay_out(files, n, JpegRoute::kSync, (size_t)nsync, sizeof(SyncFrame), 0, 0);
    l.total = l.back + (size_t)nsync * sizeof(SyncWords);
    l.d_spec = ((size_t)nsync * sizeof(SyncWords) + 31) & ~(size_t)31;
    l.d_bytes = l.d_spec + 3 * l.nitems * sizeof(JpegSyncRecord) + l.nitems * sizeof(JpegSyncStart);
    return l;
}

// what both fills share: the tables the scan names and the stream with its zeroed pad
inline void jpeg_stage_fill_shared(char* image, const JpegStageFile& j) {
    for (int s = 0; s < j.ntables; ++s) memcpy(image + j.table_off + (size_t)s * sizeof(JpegHuffTable), j.tables[s], sizeof(JpegHuffTable));
    memcpy(image + j.stream_off, j.data + j.scan.entropy_begin, j.len);
    memset(image + j.stream_off + j.len, 0, jpeg_stage_padded(j.len) - j.len);
}

// Writes file i of the chunk into the interval image: every byte of the image that belongs to it, and nothing else (any
// thread, one per file).  A file of another route gets an empty record and a zero quantisation table.
inline void jpeg_huff_fill(char* image, size_t image_bytes, const JpegImageLayout& l, const JpegStageFile& j, int i, int blocks_h,
                           int pitch_blocks) {
    assert(l.total <= image_bytes);
    (void)image_bytes;
    HuffFrame fr;
    memset(&fr, 0, sizeof(fr));
    uint16_t* quant = (uint16_t*)(image + l.quant) + (size_t)i * 64;
    if (j.route != JpegRoute::kIntervals) {
        memset(quant, 0, 64 * sizeof(uint16_t));
        memcpy(image + (size_t)i * sizeof(HuffFrame), &fr, sizeof(fr));
        return;
    }
    const JpegScan& sc = j.scan;
    memcpy(quant, sc.info.quant, 64 * sizeof(uint16_t));
    fr.stream_off = j.stream_off;
    fr.table_off = (uint32_t)j.table_off;
    fr.interval_first = (uint32_t)j.item_first;
    fr.nintervals = (int32_t)j.nitems;
    fr.restart_interval = (int32_t)sc.restart_interval;
    fr.nmcu = sc.mcus_x * sc.mcus_y;
    fr.ntables = j.ntables;
    fr.geom = j.geom;
    fr.geom.blocks_h = blocks_h;
    fr.geom.pitch_blocks = pitch_blocks;
    memcpy(image + (size_t)i * sizeof(HuffFrame), &fr, sizeof(fr));
    jpeg_stage_fill_shared(image, j);
    uint32_t* iv = (uint32_t*)(image + l.items) + 2 * j.item_first;
    for (size_t q = 0; q < sc.intervals.size(); ++q) iv[q] = (uint32_t)(sc.intervals[q] - sc.entropy_begin);
    memset(image + l.back + j.item_first, 0, j.nitems);
}

// Writes sync file i (its index among the chunk's sync files) into the sync image, likewise.
inline void jpeg_sync_fill(char* image, size_t image_bytes, const JpegSyncLayout& l, const JpegStageFile& j, int i, int blocks_h,
                           int pitch_blocks) {
    assert(l.total <= image_bytes);
    (void)image_bytes;
    const JpegScan& sc = j.scan;
    SyncFrame fr;
    memset(&fr, 0, sizeof(fr));
    fr.stream_off = j.stream_off;
    fr.table_off = (uint32_t)j.table_off;
    fr.rec_first = (uint32_t)j.item_first;
    fr.nsub = j.nitems;
    fr.len = j.len;
    fr.total = (uint32_t)(sc.mcus_x * sc.mcus_y * sc.blocks_per_mcu);
    fr.ntables = (uint32_t)j.ntables;
    fr.frame = (uint32_t)j.frame;
    fr.geom = j.geom;
    fr.geom.blocks_h = blocks_h;
    fr.geom.pitch_blocks = pitch_blocks;
    memcpy(image + (size_t)i * sizeof(SyncFrame), &fr, sizeof(fr));
    jpeg_stage_fill_shared(image, j);
}

}  // namespace mrg
