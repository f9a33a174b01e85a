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

// The inverse DCT of every block into out (info.width x info.height bytes, dense); coef laid out as above.
void jpeg_idct_host(const int16_t* coef, int row_pitch_blocks, const JpegInfo& info, uint8_t* out);

}  // namespace mrg
