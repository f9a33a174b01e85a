// See image_io.h.
#include "image_io.h"
#include "bayer_pixels.h"
#include "bmp_pixels.h"
#include "colour_pixels.h"
#include "jpeg.h"
#include "png_filter.h"
#include "pnm_pixels.h"
#include "raw_pixels.h"
#include "tiff_inflate.h"
#include "tiff_lzw.h"
#include "../../include/mrgingham_amd.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <cmath>
#include <memory>

namespace mrg {

// Largest side the library accepts anywhere (int16 coordinates, find_chessboard_corners.cc:91): checked
// BEFORE anything is allocated or indexed from a header field of an untrusted file.
constexpr int kMaxSide = 32767;

bool read_file(const char* path, std::vector<uint8_t>& buf) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (n <= 0) { fclose(f); return false; }
    buf.resize((size_t)n);
    const bool ok = fread(buf.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

static void about_to_hold(Image& im, size_t n8, size_t n16) {
    if (im.before_grow && (n8 > im.px8.capacity() || n16 > im.px16.capacity())) im.before_grow(n8, n16);
}

// The one parser of a binary PGM's header (image_io.h).
int pgm_header(const uint8_t* b, size_t nbytes, int* width, int* height, int* bits, size_t* payload_offset) {
    if (!b || nbytes < 2 || b[0] != 'P' || b[1] != '5') return -1;
    size_t p = 2;
    int v[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        for (;;) {
            while (p < nbytes && (b[p] == ' ' || b[p] == '\t' || b[p] == '\n' || b[p] == '\r')) ++p;
            if (p < nbytes && b[p] == '#') { while (p < nbytes && b[p] != '\n') ++p; continue; }
            break;
        }
        if (p >= nbytes) return kPgmHeaderCut;
        if (b[p] < '0' || b[p] > '9') return -1;
        long x = 0;
        while (p < nbytes && b[p] >= '0' && b[p] <= '9') { x = x * 10 + (b[p] - '0'); if (x > 1 << 30) return -1; ++p; }
        v[k] = (int)x;
    }
    if (p >= nbytes) return kPgmHeaderCut;  // (the last number may go on, and the single whitespace after it is part of the header)
    ++p;
    if (v[0] <= 0 || v[1] <= 0 || v[0] > kMaxSide || v[1] > kMaxSide || v[2] <= 0 || v[2] > 65535) return -1;
    if (width) *width = v[0];
    if (height) *height = v[1];
    if (bits) *bits = v[2] < 256 ? 8 : 16;
    if (payload_offset) *payload_offset = p;
    return 0;
}

static bool decode_pgm(const std::vector<uint8_t>& b, Image& im) {
    int w = 0, h = 0, bits = 0;
    size_t p = 0;
    if (pgm_header(b.data(), b.size(), &w, &h, &bits, &p) != 0) return false;
    const size_t n = (size_t)w * h;
    if (b.size() - p < n * (size_t)(bits / 8)) return false;
    im.w = w; im.h = h; im.depth = bits;
    if (bits == 8) {
        about_to_hold(im, n, 0);
        im.px8.assign(b.begin() + p, b.begin() + p + n);
    } else {
        about_to_hold(im, 0, n);
        im.px16.resize(n);
        for (size_t i = 0; i < n; ++i) im.px16[i] = (uint16_t)((b[p + 2 * i] << 8) | b[p + 2 * i + 1]);
    }
    return true;
}

static inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | (p[1] << 16) | (p[2] << 8) | p[3]; }

// The chunk walk of a PNG held in memory: the signature, IHDR first, once and 13 bytes long, sides within the library's
// limit (checked BEFORE anything is sized from them), IDAT chunks concatenated, PLTE kept, up to IEND.  ch: channels.
struct PngHead {
    int w = 0, h = 0, bits = 0, ctype = -1, ch = 0;
};

static bool png_chunks(const uint8_t* b, size_t nbytes, PngHead& hd, std::vector<uint8_t>* idat, std::vector<uint8_t>* plte) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (nbytes < 8 + 25 || memcmp(b, sig, 8)) return false;
    size_t p = 8;
    int interlace = 0;
    bool have_ihdr = false, have_idat = false;
    while (p + 12 <= nbytes) {
        const uint32_t len = be32(&b[p]);
        const char* type = (const char*)&b[p + 4];
        if (p + 12 + (size_t)len > nbytes) return false;
        const uint8_t* d = &b[p + 8];
        if (!memcmp(type, "IHDR", 4)) {
            // exactly one IHDR, first, 13 bytes; sides within the library's limit (a crafted header must
            // not size the buffers below)
            if (have_ihdr || p != 8 || len != 13) return false;
            const uint32_t uw = be32(d), uh = be32(d + 4);
            if (uw == 0 || uh == 0 || uw > (uint32_t)kMaxSide || uh > (uint32_t)kMaxSide) return false;
            hd.w = (int)uw; hd.h = (int)uh; hd.bits = d[8]; hd.ctype = d[9]; interlace = d[12];
            have_ihdr = true;
        } else if (!have_ihdr) return false;  // any other chunk before IHDR
        else if (!memcmp(type, "PLTE", 4)) { if (plte) plte->assign(d, d + len); }
        else if (!memcmp(type, "IDAT", 4)) { if (idat) idat->insert(idat->end(), d, d + len); have_idat = have_idat || len > 0; }
        else if (!memcmp(type, "IEND", 4)) break;
        p += 12 + (size_t)len;
    }
    if (!have_ihdr || !have_idat || interlace != 0 || (hd.bits != 8 && hd.bits != 16)) return false;
    switch (hd.ctype) {
        case 0: hd.ch = 1; break;
        case 2: hd.ch = 3; break;
        case 3: hd.ch = 1; if (hd.bits != 8) return false; break;
        case 4: hd.ch = 2; break;
        case 6: hd.ch = 4; break;
        default: return false;
    }
    return true;
}

int png_header(const char* path, int* width, int* height, int* bits) {
    if (!path) return -1;
    FILE* f = fopen(path, "rb");
    if (!f) return -1;
    uint8_t b[33];
    const size_t got = fread(b, 1, sizeof(b), f);
    fclose(f);
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (got != sizeof(b) || memcmp(b, sig, 8) || be32(&b[8]) != 13 || memcmp(&b[12], "IHDR", 4)) return -1;
    if (width) *width = (int)(be32(&b[16]) & 0x7fffffffu);
    if (height) *height = (int)(be32(&b[20]) & 0x7fffffffu);
    if (bits) *bits = b[24];
    return b[25];
}

int png_scanlines(const uint8_t* data, size_t nbytes, uint8_t* scan, size_t scan_capacity, int* width, int* height, int* bits,
                  int* color_type) {
    if (!data) return -1;
    try {
        PngHead hd;
        std::vector<uint8_t> idat;
        if (!png_chunks(data, nbytes, hd, scan ? &idat : nullptr, nullptr)) return -1;
        if (width) *width = hd.w;
        if (height) *height = hd.h;
        if (bits) *bits = hd.bits;
        if (color_type) *color_type = hd.ctype;
        if (hd.ctype == 3) return kPngNotTaken;
        if (!scan) return 0;
        const size_t rowb = (size_t)hd.w * hd.ch * hd.bits / 8, need = (rowb + 1) * (size_t)hd.h;
        if (scan_capacity < need) return -2;
        uLongf rawlen = (uLongf)need;
        if (uncompress(scan, &rawlen, idat.data(), (uLong)idat.size()) != Z_OK || rawlen != need) return -1;
        // the kernel never meets a filter type it has no predictor for
        for (int y = 0; y < hd.h; ++y)
            if (scan[(rowb + 1) * y] >= kPngFilters) return -1;
        return 0;
    } catch (...) {  // std::bad_alloc
        return -1;
    }
}

static bool decode_png(const std::vector<uint8_t>& b, Image& im) {
    PngHead hd;
    std::vector<uint8_t> idat, plte;
    if (!png_chunks(b.data(), b.size(), hd, &idat, &plte)) return false;
    const int w = hd.w, h = hd.h, bits = hd.bits, ctype = hd.ctype;
    const size_t bpp = (size_t)hd.ch * bits / 8, rowb = (size_t)w * bpp;
    std::vector<uint8_t> raw((rowb + 1) * (size_t)h);
    uLongf rawlen = (uLongf)raw.size();
    if (uncompress(raw.data(), &rawlen, idat.data(), (uLong)idat.size()) != Z_OK || rawlen != raw.size()) return false;
    std::vector<uint8_t> img(rowb * (size_t)h);
    for (int y = 0; y < h; ++y) {
        const uint8_t ft = raw[(rowb + 1) * y];
        if (ft >= kPngFilters) return false;
        const uint8_t* s = &raw[(rowb + 1) * y + 1];
        uint8_t* o = &img[rowb * y];
        const uint8_t* up = y ? o - rowb : nullptr;
        for (size_t i = 0; i < rowb; ++i) {
            const int a = i >= bpp ? o[i - bpp] : 0, bb = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
            o[i] = (uint8_t)(s[i] + png_predict(ft, a, bb, c));
        }
    }
    const size_t n = (size_t)w * h;
    im.w = w; im.h = h; im.depth = bits;
    if (bits == 8) {
        about_to_hold(im, n, 0);
        im.px8.resize(n);
        for (size_t i = 0; i < n; ++i) {
            const uint8_t* q = &img[i * bpp];
            if (ctype == 0 || ctype == 4) im.px8[i] = q[0];
            else if (ctype == 3) {
                if ((size_t)q[0] * 3 + 2 >= plte.size()) return false;
                im.px8[i] = (uint8_t)png_grey(plte[q[0] * 3], plte[q[0] * 3 + 1], plte[q[0] * 3 + 2]);
            } else im.px8[i] = (uint8_t)png_grey(q[0], q[1], q[2]);
        }
    } else {
        about_to_hold(im, 0, n);
        im.px16.resize(n);
        for (size_t i = 0; i < n; ++i) {
            const uint8_t* q = &img[i * bpp];
            auto s16 = [&](int k) { return (uint32_t)((q[2 * k] << 8) | q[2 * k + 1]); };
            im.px16[i] = (uint16_t)((ctype == 0 || ctype == 4) ? s16(0) : png_grey(s16(0), s16(1), s16(2)));
        }
    }
    return true;
}

// Baseline JPEG (jpeg.h): the luma plane, as cv::imread(IMREAD_GRAYSCALE) takes it from libjpeg.
static bool decode_jpeg(const std::vector<uint8_t>& b, Image& im) {
    JpegInfo info;
    if (jpeg_coefficients(b.data(), b.size(), nullptr, 0, 0, &info) != 0) return false;
    std::vector<int16_t> coef((size_t)info.blocks_w * info.blocks_h * 64);
    if (jpeg_coefficients(b.data(), b.size(), coef.data(), coef.size(), 0, &info) != 0) return false;
    const size_t n = (size_t)info.width * info.height;
    im.w = info.width; im.h = info.height; im.depth = 8;
    about_to_hold(im, n, 0);
    im.px8.resize(n);
    jpeg_idct_host(coef.data(), 0, info, im.px8.data());
    return true;
}

// ---- TIFF (image_io.h: tiff_layout has the subset)

namespace {

struct TiffEntry {
    bool present = false;
    uint32_t type = 0, count = 0;
    size_t at = 0;  // where the values lie in the file (checked: at + count * size <= nbytes)
};

struct TiffReader {
    const uint8_t* b;
    size_t n;
    bool be;
    uint32_t u16(size_t p) const { return be ? (uint32_t)(b[p] << 8 | b[p + 1]) : (uint32_t)(b[p + 1] << 8 | b[p]); }
    uint32_t u32(size_t p) const {
        return be ? ((uint32_t)b[p] << 24 | (uint32_t)b[p + 1] << 16 | (uint32_t)b[p + 2] << 8 | b[p + 3])
                  : ((uint32_t)b[p + 3] << 24 | (uint32_t)b[p + 2] << 16 | (uint32_t)b[p + 1] << 8 | b[p]);
    }
    // value i (< count) of an entry of type BYTE, SHORT or LONG
    uint32_t value(const TiffEntry& e, uint32_t i) const {
        return e.type == 1 ? b[e.at + i] : e.type == 3 ? u16(e.at + 2 * (size_t)i) : u32(e.at + 4 * (size_t)i);
    }
};

// the tags the reader looks at; every other tag of the IFD is passed over, whatever its type
enum { kTagWidth, kTagHeight, kTagBits, kTagCompression, kTagPhotometric, kTagFillOrder, kTagStripOffsets, kTagOrientation,
       kTagSamples, kTagRowsPerStrip, kTagStripByteCounts, kTagPlanar, kTagPredictor, kTagTileWidth, kTagTileLength,
       kTagTileOffsets, kTagTileByteCounts, kTagSampleFormat, kTags };
const uint16_t kTiffTagIds[kTags] = {256, 257, 258, 259, 262, 266, 273, 274, 277, 278, 279, 284, 317, 322, 323, 324, 325, 339};

}  // namespace

static int tiff_parse(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, int64_t deflate_max_strip, mrgingham_amd_tiff_info* info_out,
                      int32_t* tile_width, int32_t* tile_length, mrgingham_amd_tiff_strip* strips, size_t capacity, size_t* nstrips_out);

int tiff_layout(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, mrgingham_amd_tiff_info* info_out,
                mrgingham_amd_tiff_strip* strips, size_t capacity, size_t* nstrips_out) {
    return tiff_layout_ex(data, nbytes, lzw_max_strip, 0, info_out, strips, capacity, nstrips_out);
}

int tiff_layout_ex(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, int64_t deflate_max_strip, mrgingham_amd_tiff_info* info_out,
                   mrgingham_amd_tiff_strip* strips, size_t capacity, size_t* nstrips_out) {
    return tiff_parse(data, nbytes, lzw_max_strip, deflate_max_strip, info_out, nullptr, nullptr, strips, capacity, nstrips_out);
}

int tiff_layout_tiled(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, int64_t deflate_max_strip, mrgingham_amd_tiff_info* info_out,
                      int32_t* tile_width, int32_t* tile_length, mrgingham_amd_tiff_strip* records, size_t capacity, size_t* nrecords_out) {
    int32_t tw = 0, tl = 0;
    const int rc = tiff_parse(data, nbytes, lzw_max_strip, deflate_max_strip, info_out, &tw, &tl, records, capacity, nrecords_out);
    if (tile_width) *tile_width = tw;
    if (tile_length) *tile_length = tl;
    return rc;
}

// tile_width / tile_length NULL: tiff_layout_ex, to which any tile tag is unreadable; else tiff_layout_tiled
static int tiff_parse(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, int64_t deflate_max_strip, mrgingham_amd_tiff_info* info_out,
                      int32_t* tile_width, int32_t* tile_length, mrgingham_amd_tiff_strip* strips, size_t capacity, size_t* nstrips_out) {
    if (nstrips_out) *nstrips_out = 0;
    if (tile_width) *tile_width = 0;
    if (tile_length) *tile_length = 0;
    if (!data || nbytes < 8) return -1;
    TiffReader r{data, nbytes, false};
    if (data[0] == 'I' && data[1] == 'I') r.be = false;
    else if (data[0] == 'M' && data[1] == 'M') r.be = true;
    else return -1;
    if (r.u16(2) != 42) return -1;  // (43: BigTIFF)
    const uint64_t ifd = r.u32(4);
    if (ifd < 8 || ifd + 2 > nbytes) return -1;
    const uint64_t nent = r.u16((size_t)ifd);
    if (ifd + 2 + 12 * nent > nbytes) return -1;
    TiffEntry e[kTags];
    for (uint64_t k = 0; k < nent; ++k) {
        const size_t p = (size_t)(ifd + 2 + 12 * k);
        const uint32_t tag = r.u16(p);
        int t = -1;
        for (int i = 0; i < kTags; ++i)
            if (kTiffTagIds[i] == tag) t = i;
        if (t < 0) continue;
        TiffEntry& x = e[t];
        if (x.present) return -1;  // a tag twice
        x.present = true;
        x.type = r.u16(p + 2);
        x.count = r.u32(p + 4);
        if ((x.type != 1 && x.type != 3 && x.type != 4) || x.count == 0) return -1;
        // count * size in 64 bits: at most 2^34
        const uint64_t bytes = (uint64_t)x.count * (x.type == 1 ? 1u : x.type == 3 ? 2u : 4u);
        if (bytes <= 4) x.at = p + 8;
        else {
            const uint64_t off = r.u32(p + 8);
            if (off > nbytes || bytes > nbytes - off) return -1;
            x.at = (size_t)off;
        }
    }
    auto one = [&](int t, uint32_t dflt, bool* ok) -> uint32_t {  // a tag that holds one value
        if (!e[t].present) return dflt;
        if (e[t].count != 1) { *ok = false; return dflt; }
        return r.value(e[t], 0);
    };
    bool ok = true;
    const bool any_tile = e[kTagTileWidth].present || e[kTagTileLength].present || e[kTagTileOffsets].present || e[kTagTileByteCounts].present;
    // tiled: all four tile tags and neither strip tag; any other mixture is unreadable
    const bool tiled = tile_width && tile_length && e[kTagTileWidth].present && e[kTagTileLength].present && e[kTagTileOffsets].present &&
                       e[kTagTileByteCounts].present && !e[kTagStripOffsets].present && !e[kTagStripByteCounts].present;
    if (any_tile && !tiled) return -1;
    if (!e[kTagWidth].present || !e[kTagHeight].present || !e[kTagBits].present || !e[kTagPhotometric].present) return -1;
    if (!tiled && (!e[kTagStripOffsets].present || !e[kTagStripByteCounts].present)) return -1;
    const uint32_t w = one(kTagWidth, 0, &ok), h = one(kTagHeight, 0, &ok), spp = one(kTagSamples, 1, &ok);
    const uint32_t comp = one(kTagCompression, 1, &ok), photo = one(kTagPhotometric, 0, &ok), pred = one(kTagPredictor, 1, &ok);
    uint32_t rps = tiled ? 0 : one(kTagRowsPerStrip, 0xFFFFFFFFu, &ok);  // (RowsPerStrip in a tiled file is ignored)
    if (!ok || one(kTagFillOrder, 1, &ok) != 1 || one(kTagOrientation, 1, &ok) != 1 || one(kTagPlanar, 1, &ok) != 1 || !ok) return -1;
    if (w == 0 || h == 0 || w > (uint32_t)kMaxSide || h > (uint32_t)kMaxSide || spp < 1 || spp > 4) return -1;
    if (e[kTagBits].count != spp) return -1;
    const uint32_t bits = r.value(e[kTagBits], 0);
    for (uint32_t i = 1; i < spp; ++i)
        if (r.value(e[kTagBits], i) != bits) return -1;
    if (bits != 8 && bits != 16) return -1;
    if (e[kTagSampleFormat].present) {
        if (e[kTagSampleFormat].count > spp) return -1;
        for (uint32_t i = 0; i < e[kTagSampleFormat].count; ++i)
            if (r.value(e[kTagSampleFormat], i) != 1) return -1;
    }
    if (photo > 2 || (photo == 2 && spp < 3)) return -1;
    if (comp != 1 && comp != 5 && comp != 32773 && comp != 8 && comp != 32946) return -1;
    if (pred != 1 && pred != 2) return -1;
    uint32_t tw = 0, tl = 0, across = 0;
    if (tiled) {
        tw = one(kTagTileWidth, 0, &ok);
        tl = one(kTagTileLength, 0, &ok);
        if (!ok || tw == 0 || tl == 0 || tw > (uint32_t)kMaxSide || tl > (uint32_t)kMaxSide) return -1;
        across = (w + tw - 1) / tw;
        rps = tl;
    } else {
        if (rps == 0) return -1;
        if (rps > h) rps = h;
    }
    // (tiles: at most 32767 x 32767 of them)
    const uint32_t ns = tiled ? across * ((h + tl - 1) / tl) : (h + rps - 1) / rps;
    const TiffEntry& eoff = e[tiled ? kTagTileOffsets : kTagStripOffsets];
    const TiffEntry& ecnt = e[tiled ? kTagTileByteCounts : kTagStripByteCounts];
    if (eoff.count != ns || ecnt.count != ns) return -1;
    // a tile decodes to its full size whatever the image keeps of it: the rules below hold per tile
    const uint64_t rowb = (uint64_t)(tiled ? tw : w) * spp * (bits / 8);
    const bool deflate = comp == 8 || comp == 32946;
    bool taken = comp == 1 || comp == 5 || (deflate && deflate_max_strip > 0);
    if (tiled && tw % 16 != 0) taken = false;  // (a lane's 16 pixels lie in one tile: tiff_finish_tiles_kernel)
    if (deflate_max_strip > (int64_t)kTiffInflateMaxStrip) deflate_max_strip = (int64_t)kTiffInflateMaxStrip;
    if (lzw_max_strip <= 0 || lzw_max_strip > (int64_t)kTiffLzwMaxStrip20) lzw_max_strip = (int64_t)kTiffLzwMaxStrip20;
    for (uint32_t i = 0; i < ns; ++i) {
        const uint64_t off = r.value(eoff, i), cnt = r.value(ecnt, i);
        const uint32_t first = tiled ? (i / across) * tl : i * rps, rows = tiled ? tl : h - first < rps ? h - first : rps;
        if (off > nbytes || cnt > nbytes - off) return -1;
        if (comp == 1 && cnt < rows * rowb) return -1;
        // (a code is at least 9 bits and gives fewer than 4096 bytes: a strip that cannot hold its rows is refused before
        // anything is sized for them)
        if (comp == 5 && (cnt * 8 / 9 + 1) * 4096 < rows * rowb) return -1;
        if (comp == 32773 && cnt * 64 < rows * rowb) return -1;                       // (two bytes give at most 128)
        if (deflate && (cnt + 1) * 1040 < rows * rowb) return -1;  // (Deflate: below 1032 to 1)
        if (comp == 5 && rows * rowb > (uint64_t)lzw_max_strip) taken = false;
        // (and not with more bytes than any zlib stream of its rows needs: a block need not give a byte, tiff_inflate.h)
        if (deflate && taken && (rows * rowb > (uint64_t)deflate_max_strip || cnt > tiff_inflate_max_bytes(rows * rowb))) taken = false;
        if (strips && i < capacity) strips[i] = mrgingham_amd_tiff_strip{(int64_t)off, (int64_t)cnt, (int32_t)first, (int32_t)rows};
    }
    if (info_out)
        *info_out = mrgingham_amd_tiff_info{(int32_t)w, (int32_t)h, (int32_t)bits, (int32_t)spp, (int32_t)photo, (int32_t)comp,
                                            (int32_t)pred, r.be ? 1 : 0};
    if (nstrips_out) *nstrips_out = ns;
    if (tiled) { *tile_width = (int32_t)tw; *tile_length = (int32_t)tl; }
    if (strips && capacity < ns) return -2;
    return taken ? 0 : kTiffNotTaken;
}

// one decoded row (file bytes, rowb of them) to grey samples: value order, predictor 2 undone, WhiteIsZero inverted, the
// first sample or png_grey of the first three -- the steps of tiff_finish_kernel (tiff_decode.hip)
template <class T>
static void tiff_finish_row(const uint8_t* s, const mrgingham_amd_tiff_info& ti, T* o) {
    constexpr uint32_t mask = sizeof(T) == 1 ? 255u : 65535u;
    const int spp = ti.samples, nc = ti.photometric == 2 ? 3 : 1;
    uint32_t acc[3] = {0, 0, 0};
    for (int x = 0; x < ti.width; ++x) {
        uint32_t v[3] = {0, 0, 0};
        for (int c = 0; c < nc; ++c) {
            const uint8_t* q = s + ((size_t)x * spp + c) * sizeof(T);
            uint32_t raw = sizeof(T) == 1 ? q[0] : ti.big_endian ? (uint32_t)(q[0] << 8 | q[1]) : (uint32_t)(q[1] << 8 | q[0]);
            if (ti.predictor == 2) raw = acc[c] = (acc[c] + raw) & mask;
            v[c] = ti.photometric == 0 ? mask - raw : raw;
        }
        o[x] = (T)(nc == 3 ? png_grey(v[0], v[1], v[2]) : v[0]);
    }
}

// PackBits, row by row (a run never crosses the end of its row): exactly rows * rowb bytes, or false
static bool tiff_unpackbits(const uint8_t* s, size_t ns, uint8_t* o, size_t rowb, size_t rows) {
    size_t p = 0;
    for (size_t y = 0; y < rows; ++y) {
        size_t x = 0;
        while (x < rowb) {
            if (p >= ns) return false;
            const int c = (int8_t)s[p++];
            if (c == -128) continue;
            const size_t run = c >= 0 ? (size_t)c + 1 : (size_t)(1 - c);
            if (run > rowb - x) return false;
            if (c >= 0) {
                if (run > ns - p) return false;
                memcpy(o + y * rowb + x, s + p, run);
                p += run;
            } else {
                if (p >= ns) return false;
                memset(o + y * rowb + x, s[p++], run);
            }
            x += run;
        }
    }
    return true;
}

// one compressed strip or tile (compression 5, 32773, 8 or 32946) to exactly rows x rowb bytes, or false
static bool tiff_decompress(const mrgingham_amd_tiff_info& ti, const uint8_t* src, const mrgingham_amd_tiff_strip& st, size_t rowb,
                            std::vector<uint8_t>& raw, std::unique_ptr<TiffLzwHostTable>& tab) {
    const size_t need = rowb * (size_t)st.rows;
    // (the decoders count in 32 bits: a strip of 4 GiB or more is refused before anything is sized for it)
    if (need > 0xFFFFFFFFull || (uint64_t)st.nbytes > 0xFFFFFFFFull) return false;
    raw.resize(need);
    if (ti.compression == 5) {
        if (!tab) tab.reset(new TiffLzwHostTable);
        return tiff_lzw_decode(src, (uint32_t)st.nbytes, raw.data(), (uint32_t)need, *tab) == kTiffLzwOk;
    }
    if (ti.compression == 32773) return tiff_unpackbits(src, (size_t)st.nbytes, raw.data(), rowb, (size_t)st.rows);
    uLongf got = (uLongf)need;
    return uncompress(raw.data(), &got, src, (uLong)st.nbytes) == Z_OK && got == need;
}

static bool decode_tiff(const std::vector<uint8_t>& b, Image& im) {
    mrgingham_amd_tiff_info ti;
    size_t ns = 0;
    int32_t tw = 0, tl = 0;
    int rc = tiff_layout_tiled(b.data(), b.size(), 0, 0, &ti, &tw, &tl, nullptr, 0, &ns);
    if (rc != 0 && rc != kTiffNotTaken) return false;
    std::vector<mrgingham_amd_tiff_strip> strips(ns);
    rc = tiff_layout_tiled(b.data(), b.size(), 0, 0, &ti, &tw, &tl, strips.data(), ns, &ns);
    if (rc != 0 && rc != kTiffNotTaken) return false;
    const size_t bpp = (size_t)ti.samples * (ti.bits / 8), rowb = (size_t)(tw ? tw : ti.width) * bpp, n = (size_t)ti.width * ti.height;
    im.w = ti.width; im.h = ti.height; im.depth = ti.bits;
    if (ti.bits == 8) { about_to_hold(im, n, 0); im.px8.resize(n); }
    else { about_to_hold(im, 0, n); im.px16.resize(n); }
    std::vector<uint8_t> raw;
    std::unique_ptr<TiffLzwHostTable> tab;
    const size_t across = tw ? ((size_t)ti.width + tw - 1) / tw : 1;
    for (size_t i = 0; i < strips.size(); ++i) {
        const mrgingham_amd_tiff_strip& st = strips[i];
        const uint8_t* rows = b.data() + st.offset;
        if (ti.compression != 1) {
            if (!tiff_decompress(ti, rows, st, rowb, raw, tab)) return false;
            rows = raw.data();
        }
        // a tile: its rows inside the image, of each the columns inside the image; the predictor restarts at the tile's left edge
        const size_t x0 = tw ? (i % across) * (size_t)tw : 0;
        mrgingham_amd_tiff_info part = ti;
        if (tw && (size_t)ti.width - x0 < (size_t)tw) part.width = (int32_t)((size_t)ti.width - x0);
        else if (tw) part.width = tw;
        for (int y = 0; y < st.rows && st.first_row + y < ti.height; ++y) {
            const size_t at = ((size_t)st.first_row + y) * ti.width + x0;
            if (ti.bits == 8) tiff_finish_row<uint8_t>(rows + rowb * y, part, &im.px8[at]);
            else tiff_finish_row<uint16_t>(rows + rowb * y, part, &im.px16[at]);
        }
    }
    return true;
}

// ---- Windows Bitmap (image_io.h: bmp_layout; include/mrgingham_amd.h has the subset)

// The RLE8 stream s[0, n) of a bottom-up file, from bfOffBits to the end of the file: the walk that decides whether it
// keeps the rules and, with out != NULL (w * h bytes the caller has filled with lut[0]), the decoder.
static bool bmp_rle8(const uint8_t* s, size_t n, int w, int h, const uint8_t* lut, uint8_t* out) {
    size_t p = 0;
    int x = 0, y = 0;  // (y counts from the bottom row)
    for (;;) {
        if (n - p < 2) return y >= h - 1;  // no end-of-bitmap: fine once the last row was begun
        const int c = s[p], v = s[p + 1];
        p += 2;
        if (c > 0) {  // an encoded run
            if (y >= h || c > w - x) return false;
            if (out) memset(out + (size_t)(h - 1 - y) * w + x, lut[v], (size_t)c);
            x += c;
        } else if (v == 0) {  // end of line
            x = 0;
            if (y < h) ++y;
        } else if (v == 1) {  // end of bitmap
            return true;
        } else if (v == 2) {  // delta
            if (n - p < 2) return false;
            x += s[p];
            y += s[p + 1];
            p += 2;
            if (x > w || y > h) return false;
        } else {  // an absolute run, padded to even
            if (y >= h || v > w - x || n - p < (size_t)v) return false;
            if (out)
                for (int i = 0; i < v; ++i) out[(size_t)(h - 1 - y) * w + x + i] = lut[s[p + i]];
            x += v;
            p += (size_t)v + (v & 1);
            if (p > n) p = n;  // (the pad byte of a run that ends the file)
        }
    }
}

int bmp_layout(const uint8_t* b, size_t have, size_t file_size, mrgingham_amd_bmp_info* info_out) {
    if (!b || have > file_size || have < 14 + 40 || b[0] != 'B' || b[1] != 'M') return -1;
    auto u16 = [&](size_t p) { return (uint32_t)(b[p] | b[p + 1] << 8); };
    auto u32 = [&](size_t p) { return (uint32_t)b[p] | (uint32_t)b[p + 1] << 8 | (uint32_t)b[p + 2] << 16 | (uint32_t)b[p + 3] << 24; };
    const uint64_t off = u32(10), hsize = u32(14);
    // (12: the core header, 64: OS/2 -- other field widths)
    if (hsize != 40 && hsize != 52 && hsize != 56 && hsize != 108 && hsize != 124) return -1;
    if (14 + hsize > have) return -1;
    const int32_t w = (int32_t)u32(18), hraw = (int32_t)u32(22);
    const uint32_t planes = u16(26), bits = u16(28), comp = u32(30), used = u32(46);
    if (planes != 1 || w < 1 || w > kMaxSide || hraw == INT32_MIN) return -1;
    const bool top_down = hraw < 0;
    const int32_t h = top_down ? -hraw : hraw;
    if (h < 1 || h > kMaxSide) return -1;
    uint64_t pal = 14 + hsize;  // where the palette begins
    if (comp == 0) {
        if (bits != 1 && bits != 4 && bits != 8 && bits != 24 && bits != 32) return -1;
    } else if (comp == 1) {
        if (bits != 8 || top_down) return -1;
    } else if (comp == 3) {
        if (bits != 32) return -1;
        // the masks: behind a 40-byte header, inside a longer one (at the same place)
        if (hsize == 40) pal += 12;
        if (pal > have) return -1;
        if (u32(54) != 0x00FF0000u || u32(58) != 0x0000FF00u || u32(62) != 0x000000FFu) return -1;
    } else {
        return -1;
    }
    mrgingham_amd_bmp_info bi;
    memset(&bi, 0, sizeof(bi));
    bi.width = w; bi.height = h; bi.bits = (int32_t)bits; bi.compression = (int32_t)comp; bi.top_down = top_down ? 1 : 0;
    bi.row_bytes = (int32_t)((((uint64_t)w * bits + 31) / 32) * 4);
    bi.payload_offset = (int64_t)off;
    if (bits <= 8) {
        const uint64_t most = (uint64_t)1 << bits, n = used ? used : most;
        if (n > most) return -1;
        const uint64_t end = pal + 4 * n;  // (at most 14 + 124 + 12 + 1024)
        if (end > file_size || end > off) return -1;
        if (end > have) return -1;  // (a caller that holds fewer than the first 4096 bytes of the file)
        for (uint64_t i = 0; i < n; ++i) {
            const uint8_t* q = b + pal + 4 * i;
            bi.lut[i] = (uint8_t)png_grey(q[2], q[1], q[0]);
        }
        bi.lut_identity = 1;
        for (uint64_t i = 0; i < most; ++i)
            if (bi.lut[i] != i) bi.lut_identity = 0;
    } else if (off < pal) {
        return -1;  // (the pixel array inside the headers)
    }
    if (off > file_size) return -1;
    int rc = 0;
    if (comp == 1) {
        rc = kBmpNotTaken;
        if (have == file_size && !bmp_rle8(b + off, (size_t)(file_size - off), w, h, bi.lut, nullptr)) return -1;
    } else if ((uint64_t)bi.row_bytes * (uint64_t)h > file_size - off) {
        return -1;
    }
    if (info_out) *info_out = bi;
    return rc;
}

static bool decode_bmp(const std::vector<uint8_t>& b, Image& im) {
    mrgingham_amd_bmp_info bi;
    const int rc = bmp_layout(b.data(), b.size(), b.size(), &bi);
    if (rc != 0 && rc != kBmpNotTaken) return false;
    const int w = bi.width, h = bi.height;
    const size_t n = (size_t)w * h;
    im.w = w; im.h = h; im.depth = 8;
    about_to_hold(im, n, 0);
    if (rc == kBmpNotTaken) {
        im.px8.assign(n, bi.lut[0]);
        return bmp_rle8(b.data() + bi.payload_offset, b.size() - (size_t)bi.payload_offset, w, h, bi.lut, im.px8.data());
    }
    im.px8.resize(n);
    const uint8_t* lut = bi.bits == 8 && bi.lut_identity ? nullptr : bi.lut;
    for (int y = 0; y < h; ++y) {
        const uint8_t* row = b.data() + bi.payload_offset + (size_t)bi.row_bytes * (size_t)(bi.top_down ? y : h - 1 - y);
        uint8_t* o = &im.px8[(size_t)w * y];
        for (int x0 = 0; x0 < w; x0 += 16) {
            const int k = w - x0 < 16 ? w - x0 : 16;
            uint32_t d[4];
            bmp_pixels_any(row, bi.row_bytes, bi.bits, lut, x0, k, d);
            for (int p = 0; p < k; ++p) o[x0 + p] = (uint8_t)(d[p >> 2] >> (8 * (p & 3)));
        }
    }
    return true;
}

// ---- binary Netpbm beyond P5 (image_io.h: pnm_header; include/mrgingham_amd.h has the subset)

// P7: the lines behind the magic.  A line ends at '\n'; blanks, tabs and a '\r' may surround its words.
static int pam_header(const uint8_t* b, size_t have, mrgingham_amd_pnm_info& pi) {
    auto blank = [](uint8_t c) { return c == ' ' || c == '\t' || c == '\r'; };
    size_t p = 2;
    long field[4] = {-1, -1, -1, -1};  // WIDTH, HEIGHT, DEPTH, MAXVAL
    static const char* const kField[4] = {"WIDTH", "HEIGHT", "DEPTH", "MAXVAL"};
    bool first_line = true, tupltype_seen = false, bw = false;
    for (;;) {
        size_t e = p;
        while (e < have && b[e] != '\n') ++e;
        if (e >= have) return kPgmHeaderCut;  // (the line may go on)
        size_t s = p, t = e;
        while (s < t && blank(b[s])) ++s;
        while (t > s && blank(b[t - 1])) --t;
        p = e + 1;
        if (first_line) {  // nothing but the magic on line 1
            if (s != t) return -1;
            first_line = false;
            continue;
        }
        if (s == t || b[s] == '#') continue;
        size_t k = s;
        while (k < t && !blank(b[k])) ++k;
        const size_t nword = k - s;
        auto word = [&](const char* name) { return nword == strlen(name) && !memcmp(b + s, name, nword); };
        while (k < t && blank(b[k])) ++k;  // the value: b[k, t)
        if (word("ENDHDR")) {
            if (k != t) return -1;
            break;
        }
        if (word("TUPLTYPE")) {
            if (!tupltype_seen) bw = t - k >= 13 && !memcmp(b + k, "BLACKANDWHITE", 13);
            tupltype_seen = true;
            continue;
        }
        int which = -1;
        for (int i = 0; i < 4; ++i)
            if (word(kField[i])) which = i;
        if (which < 0 || field[which] >= 0 || k == t) return -1;
        long x = 0;
        for (; k < t; ++k) {
            if (b[k] < '0' || b[k] > '9') return -1;
            x = x * 10 + (b[k] - '0');
            if (x > 1 << 30) return -1;
        }
        field[which] = x;
    }
    for (int i = 0; i < 4; ++i)
        if (field[i] < 0) return -1;
    if (field[0] < 1 || field[0] > kMaxSide || field[1] < 1 || field[1] > kMaxSide || field[2] < 1 || field[2] > 4 || field[3] < 1 ||
        field[3] > 65535)
        return -1;
    if (bw && (field[2] > 2 || field[3] != 1)) return -1;
    pi.width = (int32_t)field[0]; pi.height = (int32_t)field[1]; pi.channels = (int32_t)field[2];
    pi.bits = field[3] < 256 ? 8 : 16;
    pi.black_and_white = bw ? 1 : 0;
    pi.payload_offset = (int64_t)p;
    return 0;
}

int pnm_header(const uint8_t* b, size_t have, size_t file_size, mrgingham_amd_pnm_info* info_out) {
    // (P6 stays unreadable: tests/test_pgm_header.py pins such a file, as tests/test_image_io.py pins P2; PAM depth 3 carries R G B)
    if (!b || have > file_size || have < 2 || b[0] != 'P' || (b[1] != '4' && b[1] != '5' && b[1] != '7')) return -1;
    mrgingham_amd_pnm_info pi;
    memset(&pi, 0, sizeof(pi));
    pi.magic = b[1] - '0';
    pi.channels = 1;
    if (pi.magic == 5) {  // pgm_header's verdicts and outputs: the payload is the caller's to measure
        size_t off = 0;
        const int rc = pgm_header(b, have, &pi.width, &pi.height, &pi.bits, &off);
        if (rc) return rc;
        pi.payload_offset = (int64_t)off;
        pi.row_bytes = pi.width * (pi.bits / 8);
        if (info_out) *info_out = pi;
        return 0;
    }
    if (pi.magic == 7) {
        const int rc = pam_header(b, have, pi);
        if (rc) return rc;
    } else {
        // P4: two numbers; white space and comments as in pgm_header
        constexpr int nv = 2;
        size_t p = 2;
        long v[2] = {0, 0};
        for (int k = 0; k < nv; ++k) {
            for (;;) {
                while (p < have && (b[p] == ' ' || b[p] == '\t' || b[p] == '\n' || b[p] == '\r')) ++p;
                if (p < have && b[p] == '#') { while (p < have && b[p] != '\n') ++p; continue; }
                break;
            }
            if (p >= have) return kPgmHeaderCut;
            if (b[p] < '0' || b[p] > '9') return -1;
            long x = 0;
            while (p < have && b[p] >= '0' && b[p] <= '9') { x = x * 10 + (b[p] - '0'); if (x > 1 << 30) return -1; ++p; }
            v[k] = x;
        }
        if (p >= have) return kPgmHeaderCut;  // (the last number may go on, and the single white-space byte after it is part of the header)
        if (b[p] != ' ' && b[p] != '\t' && b[p] != '\n' && b[p] != '\r') return -1;
        ++p;
        if (v[0] < 1 || v[1] < 1 || v[0] > kMaxSide || v[1] > kMaxSide) return -1;
        pi.width = (int32_t)v[0]; pi.height = (int32_t)v[1];
        pi.bits = 1;
        pi.channels = 1;
        pi.payload_offset = (int64_t)p;
    }
    const uint64_t rowb = pi.bits == 1 ? ((uint64_t)pi.width + 7) / 8 : (uint64_t)pi.width * (uint64_t)pi.channels * (uint64_t)(pi.bits / 8);
    pi.row_bytes = (int32_t)rowb;  // (at most 32767 * 4 * 2)
    if ((uint64_t)pi.payload_offset > file_size || rowb * (uint64_t)pi.height > file_size - (uint64_t)pi.payload_offset) return -1;
    if (info_out) *info_out = pi;
    return 0;
}

template <int BITS, int CH, bool BW>
static void pnm_rows(const uint8_t* base, long long limit, const mrgingham_amd_pnm_info& pi, Image& im) {
    constexpr int NP = PnmSpan<BITS, CH>::kPixels;
    const int w = pi.width;
    for (int y = 0; y < pi.height; ++y) {
        const long long row_off = (long long)y * pi.row_bytes;
        for (int x0 = 0; x0 < w; x0 += NP) {
            const int k = w - x0 < NP ? w - x0 : NP;
            uint32_t d[4];
            pnm_pixels<BITS, CH, BW>(base, limit, row_off, x0, k, d);
            if constexpr (BITS == 16) {
                uint16_t* o = &im.px16[(size_t)w * y + x0];
                for (int p = 0; p < k; ++p) o[p] = (uint16_t)(d[p >> 1] >> (16 * (p & 1)));
            } else {
                uint8_t* o = &im.px8[(size_t)w * y + x0];
                for (int p = 0; p < k; ++p) o[p] = (uint8_t)(d[p >> 2] >> (8 * (p & 3)));
            }
        }
    }
}

// P4, P7 (P5 keeps decode_pgm): every word of every row through pnm_pixels.h, the text the device runs
static bool decode_pnm(const std::vector<uint8_t>& b, Image& im) {
    mrgingham_amd_pnm_info pi;
    if (pnm_header(b.data(), b.size(), b.size(), &pi) != 0) return false;
    const size_t n = (size_t)pi.width * pi.height;
    im.w = pi.width; im.h = pi.height; im.depth = pi.bits == 16 ? 16 : 8;
    if (pi.bits == 16) { about_to_hold(im, 0, n); im.px16.resize(n); }
    else { about_to_hold(im, n, 0); im.px8.resize(n); }
    const uint8_t* base = b.data() + pi.payload_offset;
    const long long limit = (long long)(b.size() - (size_t)pi.payload_offset);
#define MRG_PNM_ROWS(B, C, W)                                                   \
    if (pi.bits == B && pi.channels == C && (pi.black_and_white != 0) == W) {   \
        pnm_rows<B, C, W>(base, limit, pi, im);                                 \
        return true;                                                            \
    }
    MRG_PNM_ROWS(1, 1, false)
    MRG_PNM_ROWS(8, 1, false) MRG_PNM_ROWS(8, 2, false) MRG_PNM_ROWS(8, 3, false) MRG_PNM_ROWS(8, 4, false)
    MRG_PNM_ROWS(16, 1, false) MRG_PNM_ROWS(16, 2, false) MRG_PNM_ROWS(16, 3, false) MRG_PNM_ROWS(16, 4, false)
    MRG_PNM_ROWS(8, 1, true) MRG_PNM_ROWS(8, 2, true)
#undef MRG_PNM_ROWS
    return false;
}

// 8-bit binary PGM, the format a calibration run usually feeds the tool: the pixels go from the file straight into
// px8 -- no copy of the whole file in between (a 12 MB image: one pass over memory less per image).  Returns 1 = done,
// 0 = not such a file (the general path decides), -1 = such a file, but broken.
static int read_pgm8_direct(const char* path, Image& im) {
    FILE* f = fopen(path, "rb");
    if (!f) return -1;
    uint8_t head[128];
    const size_t got = fread(head, 1, sizeof(head), f);
    int rc = 0, w = 0, h = 0, bits = 0;
    size_t p = 0;
    // (a header with a long comment does not fit the 128 bytes, a 16-bit file is not this function's: the general path takes them)
    if (got >= 8 && pgm_header(head, got, &w, &h, &bits, &p) == 0 && bits == 8) {
        const size_t n = (size_t)w * h;
        im.w = w; im.h = h; im.depth = 8;
        about_to_hold(im, n, 0);
        im.px8.resize(n);
        const size_t have = got - p < n ? got - p : n;
        memcpy(im.px8.data(), head + p, have);
        rc = fread(im.px8.data() + have, 1, n - have, f) == n - have ? 1 : -1;
    }
    fclose(f);
    return rc;
}

bool read_image(const char* path, Image& im) {
    // never throws: the callers are extern "C" entry points and detached worker threads
    try {
        const int direct = read_pgm8_direct(path, im);
        if (direct != 0) return direct > 0;
        std::vector<uint8_t>& b = im.file;
        if (!read_file(path, b) || b.size() < 8) return false;
        if (b[0] == 'P' && b[1] == '5') return decode_pgm(b, im);
        if (b[0] == 'P' && (b[1] == '4' || b[1] == '7')) return decode_pnm(b, im);
        if (b[0] == 0x89 && b[1] == 'P') return decode_png(b, im);
        if (b[0] == 0xFF && b[1] == 0xD8) return decode_jpeg(b, im);
        if ((b[0] == 'I' && b[1] == 'I') || (b[0] == 'M' && b[1] == 'M')) return decode_tiff(b, im);
        if (b[0] == 'B' && b[1] == 'M') return decode_bmp(b, im);
        return false;
    } catch (...) {  // std::bad_alloc / length_error on a file that claims more than can be held
        return false;
    }
}

// The header checks of decode_pgm / read_pgm8_direct, decode_pnm, decode_png, decode_jpeg, decode_tiff and decode_bmp without the decoding.  PGM,
// the other binary Netpbm files, PNG and uncompressed BMP keep what they need in front: only the first kProbeBytes of such a file are read (a PGM whose comments push the
// header beyond them is read whole); a JPEG is read whole, its tables may lie anywhere before SOS, and so is a TIFF.
bool probe_image(const char* path, int* width, int* height, int* bits, int* kind) {
    constexpr size_t kProbeBytes = 4096;
    if (!path) return false;
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    struct Close { FILE* f; ~Close() { fclose(f); } } close_it{f};
    try {
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        fseek(f, 0, SEEK_SET);
        if (size < 8) return false;
        std::vector<uint8_t> b((size_t)size < kProbeBytes ? (size_t)size : kProbeBytes);
        bool ok = fread(b.data(), 1, b.size(), f) == b.size();
        auto rest = [&]() {  // the whole file
            const size_t have = b.size();
            b.resize((size_t)size);
            return fread(b.data() + have, 1, b.size() - have, f) == b.size() - have;
        };
        int w = 0, h = 0, d = 0, k = 0;
        if (ok && b[0] == 'P' && b[1] == '5') {
            k = 1;
            size_t p = 0;
            int rc = pgm_header(b.data(), b.size(), &w, &h, &d, &p);
            if (rc == kPgmHeaderCut && b.size() < (size_t)size) {  // the header may go on
                ok = rest();
                if (ok) rc = pgm_header(b.data(), b.size(), &w, &h, &d, &p);
            }
            ok = ok && rc == 0 && (size_t)size - p >= (size_t)w * h * (d / 8);
        } else if (ok && b[0] == 'P' && (b[1] == '4' || b[1] == '7')) {
            k = 6;
            mrgingham_amd_pnm_info pi{};
            int rc = pnm_header(b.data(), b.size(), (size_t)size, &pi);
            if (rc == kPgmHeaderCut && b.size() < (size_t)size) {  // the header may go on
                ok = rest();
                if (ok) rc = pnm_header(b.data(), b.size(), (size_t)size, &pi);
            }
            ok = ok && rc == 0;
            w = pi.width; h = pi.height; d = pi.bits == 16 ? 16 : 8;
        } else if (ok && b[0] == 0x89 && b[1] == 'P') {
            k = 2;
            static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
            // decode_png: the signature, then IHDR first, 13 bytes long and whole
            ok = (size_t)size >= 8 + 25 && b.size() >= 8 + 25 && !memcmp(b.data(), sig, 8) && be32(&b[8]) == 13 && !memcmp(&b[12], "IHDR", 4);
            if (ok) {
                const uint8_t* dd = &b[16];
                const uint32_t uw = be32(dd), uh = be32(dd + 4);
                const int pbits = dd[8], ctype = dd[9], interlace = dd[12];
                ok = uw != 0 && uh != 0 && uw <= (uint32_t)kMaxSide && uh <= (uint32_t)kMaxSide && interlace == 0 &&
                     (pbits == 8 || pbits == 16) && (ctype == 0 || ctype == 2 || ctype == 4 || ctype == 6 || (ctype == 3 && pbits == 8));
                w = (int)uw; h = (int)uh; d = pbits;
            }
        } else if (ok && b[0] == 0xFF && b[1] == 0xD8) {
            k = 3;
            ok = b.size() == (size_t)size || rest();
            JpegInfo info;
            ok = ok && jpeg_coefficients(b.data(), b.size(), nullptr, 0, 0, &info) == 0;
            w = info.width; h = info.height; d = 8;
        } else if (ok && ((b[0] == 'I' && b[1] == 'I') || (b[0] == 'M' && b[1] == 'M'))) {
            k = 4;
            ok = b.size() == (size_t)size || rest();  // (the IFD may lie anywhere, behind the strips as well)
            mrgingham_amd_tiff_info ti{};
            if (ok) {
                int32_t tw = 0, tl = 0;
                const int rc = tiff_layout_tiled(b.data(), b.size(), 0, 0, &ti, &tw, &tl, nullptr, 0, nullptr);
                ok = rc == 0 || rc == kTiffNotTaken;
            }
            w = ti.width; h = ti.height; d = ti.bits;
        } else if (ok && b[0] == 'B' && b[1] == 'M') {
            k = 5;
            // the headers, the masks and the palette lie in the first bytes; the stream of an RLE8 file is walked whole
            mrgingham_amd_bmp_info bi{};
            int rc = bmp_layout(b.data(), b.size(), (size_t)size, &bi);
            if (rc == kBmpNotTaken && b.size() < (size_t)size) rc = rest() ? bmp_layout(b.data(), b.size(), b.size(), &bi) : -1;
            ok = rc == 0 || rc == kBmpNotTaken;
            w = bi.width; h = bi.height; d = 8;
        } else {
            ok = false;
        }
        if (!ok) return false;
        if (width) *width = w;
        if (height) *height = h;
        if (bits) *bits = d;
        if (kind) *kind = k;
        return true;
    } catch (...) {  // std::bad_alloc on a file too large to hold
        return false;
    }
}

bool write_png_gray8(const char* path, const uint8_t* px, int w, int h) {
    if (!path || !px || w <= 0 || h <= 0) return false;
    try {
        std::vector<uint8_t> raw((size_t)(w + 1) * h);
        for (int y = 0; y < h; ++y) {
            raw[(size_t)(w + 1) * y] = 0;  // filter type "none"
            memcpy(&raw[(size_t)(w + 1) * y + 1], px + (size_t)w * y, (size_t)w);
        }
        uLongf clen = compressBound((uLong)raw.size());
        std::vector<uint8_t> comp(clen);
        if (compress2(comp.data(), &clen, raw.data(), (uLong)raw.size(), 3) != Z_OK) return false;
        FILE* f = fopen(path, "wb");
        if (!f) return false;
        auto chunk = [&](const char* type, const uint8_t* d, uint32_t n) {
            uint8_t hdr[8] = {(uint8_t)(n >> 24), (uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n,
                              (uint8_t)type[0], (uint8_t)type[1], (uint8_t)type[2], (uint8_t)type[3]};
            uLong crc = crc32(0L, hdr + 4, 4);
            if (n) crc = crc32(crc, d, n);
            const uint8_t tail[4] = {(uint8_t)(crc >> 24), (uint8_t)(crc >> 16), (uint8_t)(crc >> 8), (uint8_t)crc};
            fwrite(hdr, 1, 8, f);
            if (n) fwrite(d, 1, n, f);
            fwrite(tail, 1, 4, f);
        };
        static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
        fwrite(sig, 1, 8, f);
        const uint8_t ihdr[13] = {(uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w,
                                  (uint8_t)(h >> 24), (uint8_t)(h >> 16), (uint8_t)(h >> 8), (uint8_t)h, 8, 0, 0, 0, 0};
        chunk("IHDR", ihdr, 13);
        chunk("IDAT", comp.data(), (uint32_t)clen);
        chunk("IEND", nullptr, 0);
        const bool ok = !ferror(f);
        fclose(f);
        return ok;
    } catch (...) {
        return false;
    }
}

void to_8bit_imread(const Image& im, std::vector<uint8_t>& out) {
    out.resize(im.px16.size());
    for (size_t k = 0; k < out.size(); ++k) out[k] = (uint8_t)(im.px16[k] >> 8);
}

void to_8bit(const Image& im, std::vector<uint8_t>& out) {
    out.resize(im.px16.size());
    for (size_t k = 0; k < out.size(); ++k) {
        const long r = lrint((double)im.px16[k] * (255. / 65535.));
        out[k] = (uint8_t)(r < 0 ? 0 : r > 255 ? 255 : r);
    }
}

}  // namespace mrg

extern "C" int mrgingham_amd_pgm_header(const uint8_t* data, size_t nbytes, int* width, int* height, int* bits, size_t* payload_offset) {
    return mrg::pgm_header(data, nbytes, width, height, bits, payload_offset);
}

extern "C" int mrgingham_amd_pnm_header(const uint8_t* data, size_t nbytes, mrgingham_amd_pnm_info* info) {
    return mrg::pnm_header(data, nbytes, nbytes, info);
}

extern "C" int64_t mrgingham_amd_raw_row_bytes(int width, int format) {
    if (!mrg::raw_format_ok(format) || width < 1 || width > 32767) return -1;
    return mrg::raw_min_row_bytes(width, format);
}

// a packed camera frame on the host: every word of every row through raw_pixels.h, the text the device runs
extern "C" int mrgingham_amd_raw_unpack_image(const uint8_t* payload, size_t nbytes, int width, int height, int64_t row_bytes, int format,
                                              uint16_t* out, int stride) {
    if (!payload || !out || !mrg::raw_format_ok(format) || width < 1 || height < 1 || width > 32767 || height > 32767 || stride < width)
        return MRGINGHAM_AMD_ERR_ARG;
    const int64_t rmin = mrg::raw_min_row_bytes(width, format);
    if (row_bytes < rmin || row_bytes > ((int64_t)1 << 40) || (uint64_t)nbytes < (uint64_t)((int64_t)(height - 1) * row_bytes + rmin))
        return MRGINGHAM_AMD_ERR_ARG;
    const long long limit = nbytes > (size_t)INT64_MAX ? INT64_MAX : (long long)nbytes;
    for (int y = 0; y < height; ++y) {
        uint16_t* o = out + (size_t)y * (size_t)stride;
        for (int x0 = 0; x0 < width; x0 += 8) {
            const int k = width - x0 < 8 ? width - x0 : 8;
            uint32_t d[4];
            mrg::raw_pixels_any(payload, limit, (long long)y * row_bytes, format, x0, k, d);
            for (int p = 0; p < k; ++p) o[x0 + p] = (uint16_t)(d[p >> 1] >> (16 * (p & 1)));
        }
    }
    return 0;
}

// a Bayer mosaic to grey on the host: every word of every row through bayer_pixels.h, the text the device runs
extern "C" int mrgingham_amd_bayer_grey_image(const void* mosaic, int bits, int width, int height, int64_t stride, int pattern, void* out,
                                              int64_t out_stride) {
    if (!mosaic || !out || !mrg::bayer_pattern_ok(pattern) || (bits != 8 && bits != 16) || width < 2 || height < 2 || width > 32767 ||
        height > 32767 || stride < width || out_stride < width || stride > ((int64_t)1 << 40) || out_stride > ((int64_t)1 << 40))
        return MRGINGHAM_AMD_ERR_ARG;
    if (bits == 8)
        mrg::bayer_grey_rows<1>((const uint8_t*)mosaic, width, height, stride, pattern, (uint8_t*)out, out_stride);
    else
        mrg::bayer_grey_rows<2>((const uint8_t*)mosaic, width, height, stride, pattern, (uint8_t*)out, out_stride);
    return 0;
}

// a colour frame to grey on the host: every word of every row through colour_pixels.h, the text the device runs
extern "C" int mrgingham_amd_colour_grey_image(const void* image, int bits, int format, int width, int height, int64_t stride, int64_t plane_pitch,
                                               void* out, int64_t out_stride) {
    if (!image || !out || (bits != 8 && bits != 16) || !mrg::colour_format_ok(format, bits) || width < 1 || height < 1 || width > 32767 ||
        height > 32767)
        return MRGINGHAM_AMD_ERR_ARG;
    const int layout = mrg::colour_layout(format);
    if (layout != mrg::kColourPlanar) plane_pitch = 0;  // (read for the planar formats only)
    if (stride < (int64_t)mrg::colour_row_samples(layout) * width || out_stride < width || stride > ((int64_t)1 << 40) ||
        out_stride > ((int64_t)1 << 40) || plane_pitch < 0 || plane_pitch > ((int64_t)1 << 40))
        return MRGINGHAM_AMD_ERR_ARG;
    mrg::colour_grey_rows_any((const uint8_t*)image, bits, format, width, height, stride, plane_pitch, (uint8_t*)out, out_stride);
    return 0;
}

extern "C" int mrgingham_amd_bmp_layout(const uint8_t* data, size_t nbytes, mrgingham_amd_bmp_info* info) {
    return mrg::bmp_layout(data, nbytes, nbytes, info);
}

extern "C" int mrgingham_amd_tiff_layout(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, mrgingham_amd_tiff_info* info,
                                         mrgingham_amd_tiff_strip* strips, size_t capacity, size_t* nstrips) {
    return mrg::tiff_layout(data, nbytes, lzw_max_strip, info, strips, capacity, nstrips);
}

extern "C" int mrgingham_amd_tiff_layout_ex(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, int64_t deflate_max_strip,
                                            mrgingham_amd_tiff_info* info, mrgingham_amd_tiff_strip* strips, size_t capacity, size_t* nstrips) {
    return mrg::tiff_layout_ex(data, nbytes, lzw_max_strip, deflate_max_strip, info, strips, capacity, nstrips);
}

extern "C" int mrgingham_amd_tiff_layout_tiled(const uint8_t* data, size_t nbytes, int64_t lzw_max_strip, int64_t deflate_max_strip,
                                               mrgingham_amd_tiff_info* info, int32_t* tile_width, int32_t* tile_length,
                                               mrgingham_amd_tiff_strip* records, size_t capacity, size_t* nrecords) {
    return mrg::tiff_layout_tiled(data, nbytes, lzw_max_strip, deflate_max_strip, info, tile_width, tile_length, records, capacity, nrecords);
}

extern "C" int mrgingham_amd_png_scanlines(const uint8_t* data, size_t nbytes, uint8_t* scan, size_t scan_capacity, int* width,
                                           int* height, int* bits, int* color_type) {
    return mrg::png_scanlines(data, nbytes, scan, scan_capacity, width, height, bits, color_type);
}
