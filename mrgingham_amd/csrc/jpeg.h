// Baseline JPEG for the file entry points, the command-line tool and the batch loader: what cv::imread(IMREAD_GRAYSCALE)
// gives for a grey or YCbCr file is the LUMA plane after libjpeg's default integer inverse DCT -- no colour conversion,
// no chroma upsampling.  Host only.  Two steps, so that the second can run on the device instead (jpeg_idct.hip):
//   jpeg_coefficients  marker parse + Huffman decode: the quantised luma coefficients of every 8x8 block;
//   jpeg_idct_host     dequantisation + the two-pass integer inverse DCT, bit for bit what the device kernel computes.
// Accepted: SOF0 / SOF1 (Huffman, sequential, 8 bit), 1 component or 3 taken as YCbCr (luma first, its sampling factors
// the frame's maxima), ONE scan, 8- or 16-bit quantisation tables, restart intervals.  Everything else -- progressive,
// arithmetic, lossless, 12 bit, 4 components, RGB (Adobe transform 0), several scans, DNL, sides above 32767 -- and every
// malformed stream (truncated data included: nothing is padded) is "unreadable".  Never reads or writes out of bounds,
// never sizes anything from an unchecked header field.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "jpeg_huff_lane.h"
#include "jpeg_huff_sync.h"

namespace mrg {

struct JpegInfo {
    int width = 0, height = 0;
    int blocks_w = 0, blocks_h = 0;  // luma blocks, padded to whole MCUs (4:2:0 at 31x33: 4 x 6)
    uint16_t quant[64] = {};         // the luma table, natural (row-major) order
};

// data[0..nbytes): the file.  coef (may be NULL: the header alone, up to and including SOS, is parsed and `info` filled)
// receives int16 [blocks_h][row_pitch_blocks][64], natural order inside a block, blocks in raster order (the MCU
// interleave is undone here); row_pitch_blocks <= 0 means blocks_w.  Every block of the file is written in full, nothing
// else is touched.  Returns 0; -1 unreadable (info may be partly filled); -2 the file is fine so far but
// coef_capacity (elements) or row_pitch_blocks is too small for it (info is complete, nothing decoded).
int jpeg_coefficients(const uint8_t* data, size_t nbytes, int16_t* coef, size_t coef_capacity, int row_pitch_blocks,
                      JpegInfo* info);

// What the marker parse of jpeg_coefficients finds, for a caller that decodes the entropy-coded data itself (the device:
// jpeg_huff.hip, one lane per restart interval through jpeg_huff_lane.h).
struct JpegScan {
    JpegInfo info;
    int ncomp = 0;                                 // 1 or 3
    int comp_h[3] = {}, comp_v[3] = {};            // blocks of component c in an MCU, across and down ([0]: 1, 1 when ncomp is 1)
    int td[3] = {}, ta[3] = {};                    // the DC / AC table component c decodes with: dc[td[c]], ac[ta[c]]
    int mcus_x = 0, mcus_y = 0, blocks_per_mcu = 0;
    unsigned restart_interval = 0;                 // MCUs per restart interval, 0: the file has none
    size_t entropy_begin = 0;                      // where the entropy-coded data begins
    JpegHuffTable dc[4], ac[4];
    // restart_interval != 0: [begin, end) byte offsets into the file of its ceil(mcus_x * mcus_y / restart_interval)
    // intervals, two entries each.  An interval ends at the first FF that is not followed by 00, or at the end of the
    // file; then any number of FF and D0 + (i & 7) must follow, or the file is unreadable; what follows the last
    // interval is not examined.  (Exactly what jpeg_coefficients walks over.)
    std::vector<uint64_t> intervals;
};

// The marker parse of jpeg_coefficients alone, and the restart intervals.  All acceptance rules above hold; the entropy-coded
// data is only searched for markers.  0, or -1: jpeg_coefficients calls the file unreadable as well (the converse does
// not hold: an interval may still fail to decode).
int jpeg_scan(const uint8_t* data, size_t nbytes, JpegScan* scan);

// A file without restart intervals, decoded as the device decodes it (jpeg_huff_sync.hip): the schedule of
// jpeg_huff_sync.h -- round 0, update rounds until one changes nothing, the scan, the write pass -- restated serially.
struct JpegSyncState {
    JpegScan scan;
    const uint8_t* stream = nullptr;  // the entropy-coded segment, up to its first marker (inside the caller's data)
    uint32_t len = 0, subsequence = 0, nsub = 0, total_blocks = 0;
    int ntables = 0;
    JpegHuffTable tables[kJpegLaneTables];
    JpegLaneGeom geom;
    std::vector<JpegSyncRecord> spec, cur;  // round 0; the last round's records
};

// What a lane needs of a scanned file: the tables its scan names (each once, at most kJpegLaneTables: tables[s] points
// into `sc`) and the geometry, for a coefficient area of blocks_h x pitch_blocks blocks.
void jpeg_lane_setup(const JpegScan& sc, const JpegHuffTable** tables, int* ntables, JpegLaneGeom* g, int blocks_h, int pitch_blocks);
// Where the entropy-coded segment that begins at sc.entropy_begin ends: the first FF that no 00 follows, or the end of the file.
size_t jpeg_segment_end(const uint8_t* data, size_t nbytes, size_t begin);

// Marker parse, the cut into subsequences of `subsequence` bytes (a multiple of 4 in 8..1024) and round 0.  0; -1 the
// file is unreadable; -3 it has restart intervals; -4 its stream is too long for a 32-bit bit offset.
int jpeg_sync_begin(const uint8_t* data, size_t nbytes, int subsequence, JpegSyncState* st);
// One update round over all records.  Returns whether any record changed.
bool jpeg_sync_round(JpegSyncState* st);
// The scan and the write pass over the records as they stand (only meaningful after a round that changed nothing): coef
// as for jpeg_coefficients, every block of the file written.  0, -1 unreadable, -2 coef_capacity / row_pitch_blocks too small.
int jpeg_sync_finish(const JpegSyncState& st, int16_t* coef, size_t coef_capacity, int row_pitch_blocks);
// The whole schedule with at most max_rounds changing rounds.  0 (coef and *info as jpeg_coefficients gives them), -1
// unreadable, -2 as above, -3 restart intervals / not converged within max_rounds, -4 too long (*rounds: -1 then).
int jpeg_sync_decode(const uint8_t* data, size_t nbytes, int subsequence, int max_rounds, int16_t* coef, size_t coef_capacity,
                     int row_pitch_blocks, JpegInfo* info, int* rounds, size_t* nsubsequences);

// The inverse DCT of every block into out (info.width x info.height bytes, dense); coef laid out as above.
void jpeg_idct_host(const int16_t* coef, int row_pitch_blocks, const JpegInfo& info, uint8_t* out);

}  // namespace mrg
