// Image decoding for the file-based entry points and the command-line tool (the reference uses
// cv::imread; OpenCV is not available to this build): binary PGM (P5, 8 or 16 bit),
// non-interlaced PNG (8 or 16 bit; grey, grey+alpha, RGB, RGBA, 8-bit palette) via zlib, baseline
// JPEG (jpeg.h: sequential Huffman, one scan; the luma plane, byte for byte what libjpeg's default
// decoder gives cv::imread(IMREAD_GRAYSCALE); progressive, arithmetic and multi-scan files are
// unreadable), strip or tiled TIFF (tiff_layout and tiff_layout_tiled below have the subset; LZW through tiff_lzw.h) and
// Windows Bitmap (bmp_layout below; the pixels through bmp_pixels.h); binary PBM and PAM (pnm_header below; the pixels
// through pnm_pixels.h).  PNG, TIFF, BMP and Netpbm
// colour is reduced to grey with the fixed-point BT.601 weights
// (4899 R + 9617 G + 1868 B + 8192) >> 14; byte-identity with cv::imread on colour files is not
// claimed (its conversion depends on the codec build).
#pragma once
#include <stdint.h>

#include "../../include/mrgingham_amd.h"

#include <functional>
#include <vector>

namespace mrg {

struct Image {
    int w = 0, h = 0, depth = 0;  // depth 8 or 16
    std::vector<uint8_t> px8;
    std::vector<uint16_t> px16;
    std::vector<uint8_t> file;  // the undecoded file; an Image that is reused keeps its buffers (and their warm pages)
    // called by read_image right before px8 / px16 has to GROW beyond its capacity (arguments: the element counts about to
    // be needed): an owner that has page-locked the old storage (hipHostRegister) must let go of it before it is freed
    std::function<void(size_t n8, size_t n16)> before_grow;
};

bool read_image(const char* path, Image& im);
// What read_image would produce, from the file's header alone (nothing is decoded): width, height, bits (8 or 16) and
// kind -- 1 binary PGM, 2 PNG, 3 baseline JPEG (jpeg_coefficients' header parse, up to and including SOS), 4 TIFF
// (tiff_layout_tiled: the IFD and the strip or tile table), 5 BMP (bmp_layout), 6 binary PBM / PAM (pnm_header).  false for
// whatever read_image calls unreadable at header level: a missing or empty file, another format, a header that is cut
// short or breaks a rule (sides above 32767 included), a PGM shorter than its header promises.  A file that passes may
// still fail to decode.  Never throws, never sizes anything from an unchecked field.
bool probe_image(const char* path, int* width, int* height, int* bits, int* kind);
// The header of a binary PGM (P5) held in memory, whole or only its first nbytes: the one parser behind read_image's two
// PGM readers, probe_image and the batch loader (mrgingham_amd_read_pgms_batch).  0: a header that keeps the rules --
// "P5", three decimal numbers separated by white space and # comments, ONE byte after the last; sides 1 .. 32767, maxval
// 1 .. 65535 -- with *bits 8 (maxval < 256) or 16 and *payload_offset the byte the samples begin at (16-bit samples are
// big-endian pairs).  -1: not such a file, or a rule is broken.  kPgmHeaderCut: the bytes end inside the header -- of a
// whole file that is unreadable, of a file's first bytes it asks for more.  The payload is the caller's to check:
// a file is readable when it holds width * height * bits / 8 bytes from *payload_offset on.  Any output may be NULL.
constexpr int kPgmHeaderCut = -2;
int pgm_header(const uint8_t* data, size_t nbytes, int* width, int* height, int* bits, size_t* payload_offset);
// The host half of the PNG device route (mrgingham_amd_png_scanlines): decode_png's header and chunk rules, then the
// inflated, still filtered scanlines -- row y is scan[(rowbytes + 1) * y]: its filter byte, then rowbytes bytes -- into
// `scan` (NULL: sizes only).  0 taken; kPngNotTaken readable, but a palette file (the host decoder's alone: sizes are
// reported, nothing is inflated); -1 whatever decode_png rejects, a filter byte above 4 included; -2 scan_capacity
// below (rowbytes + 1) * height (sizes are still reported).  Never throws.
constexpr int kPngNotTaken = -3;
int png_scanlines(const uint8_t* data, size_t nbytes, uint8_t* scan, size_t scan_capacity, int* width, int* height, int* bits,
                  int* color_type);
// The one IFD parser behind read_image, probe_image and the batch loader (mrgingham_amd_tiff_layout has the contract and
// the subset): the first IFD of a classic TIFF held in memory, every field checked before anything is sized from it.
// 0 the device route takes the file; kTiffNotTaken readable, but the host decoder's alone (PackBits, Deflate, an LZW strip
// that decodes to more than lzw_max_strip bytes; <= 0 or above 1 MiB: 1 MiB); -1 unreadable; -2 capacity (strips) too
// small.  Never throws, allocates nothing.
constexpr int kTiffNotTaken = -3;
int tiff_layout(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, mrgingham_amd_tiff_info* info,
                mrgingham_amd_tiff_strip* strips, size_t capacity, size_t* nstrips);
// the same with Deflate files taken whose strips decode to at most deflate_max_strip bytes (<= 0: none, tiff_layout)
int tiff_layout_ex(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, int64_t deflate_max_strip, mrgingham_amd_tiff_info* info,
                   mrgingham_amd_tiff_strip* strips, size_t capacity, size_t* nstrips);
// the same with tiled files read (mrgingham_amd_tiff_layout_tiled): a strip file as tiff_layout_ex with *tile_width =
// *tile_length = 0; a tiled file one record per tile, row-major, rows = the tile's length; 0 for it only with a tile width
// that is a multiple of 16.  read_image, probe_image and the batch loader parse through this one.
int tiff_layout_tiled(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, int64_t deflate_max_strip, mrgingham_amd_tiff_info* info,
                      int32_t* tile_width, int32_t* tile_length, mrgingham_amd_tiff_strip* records, size_t capacity, size_t* nrecords);
// The one parser of a Windows Bitmap's headers and palette, behind read_image, probe_image and the batch loader
// (mrgingham_amd_bmp_layout has the contract and the subset).  `data` holds the file's first `have` bytes, file_size is
// the size of the whole file: the headers, the masks and the palette end by byte 1174 at the latest, so the first 4096
// bytes (or the whole of a shorter file) decide; the pixel array is checked against file_size alone.  0 the device route
// takes the file; kBmpNotTaken readable, but the host decoder's alone (RLE8) -- with have == file_size the stream has
// been walked, with fewer bytes only its header is judged; -1 unreadable.  Never throws, allocates nothing.
constexpr int kBmpNotTaken = -3;
int bmp_layout(const uint8_t* data, size_t have, size_t file_size, mrgingham_amd_bmp_info* info);
// The one parser of a binary Netpbm header (P4, P5, P7; P6 stays unreadable), behind read_image, probe_image and the batch loader
// (mrgingham_amd_pnm_header has the contract and the subset).  `data` holds the file's first `have` bytes, file_size is the
// size of the whole file, against which the raster of P4 / P7 is checked; P5 gets pgm_header's verdicts and outputs.
// 0; -1 unreadable; kPgmHeaderCut: the bytes end inside the header.  Never throws, allocates nothing.
int pnm_header(const uint8_t* data, size_t have, size_t file_size, mrgingham_amd_pnm_info* info);
// The IHDR fields of a PNG file as they stand, nothing judged (a routing hint: png_scanlines decides what is readable):
// returns the colour type byte, -1 for a file that does not begin with a PNG signature and a whole IHDR.
int png_header(const char* path, int* width, int* height, int* bits);
// the whole file into buf (false: missing, unreadable or empty)
bool read_file(const char* path, std::vector<uint8_t>& buf);
// 16 -> 8 bit the way the reference CLI does it: convertTo(CV_8U, 255./65535.) (mrgingham-from-image.cc:91)
void to_8bit(const Image& im, std::vector<uint8_t>& out);
// 16 -> 8 bit the way cv::imread(IMREAD_GRAYSCALE) without IMREAD_ANYDEPTH does it (the reference's file
// entry points, find_chessboard_corners.cc:637-639, mrgingham.cc:158-160): the high byte
void to_8bit_imread(const Image& im, std::vector<uint8_t>& out);

// 8-bit grey PNG (what the reference's --debug dumps are written with cv::imwrite)
bool write_png_gray8(const char* path, const uint8_t* px, int w, int h);

}  // namespace mrg
