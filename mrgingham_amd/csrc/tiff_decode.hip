// TIFF on the device: the LZW strips of a batch of files decoded one lane per strip (tiff_lzw.h, the host decoder's text),
// Deflate strips likewise (tiff_inflate.h, zlib's contract) -- one scheduling loop, tiff_codec_lanes, over a decoder policy --,
// the rows put into value order, predictor 2 undone and the samples reduced to grey -- one row loop, tiff_finish_rows, behind
// tiff_finish_kernel (strips) and tiff_finish_tiles_kernel (tiles) --, and the batch loader that reads the files straight
// into page-locked staging.  See include/mrgingham_amd.h for the contract of the entry points and DESIGN.md sections 4.14 and
// 4.15 for the schedule and the numbers, section 4.16 for tiled files (tiles one lane each), section 4.17 for the shared bodies.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "ctx.h"
#include "image_io.h"
#include "loader.h"
#include "png_filter.h"
#include "tiff_inflate.h"
#include "tiff_lzw.h"

using namespace mrg;

namespace {

// ---- the schedule (mrgingham_amd_tiff_geometry)
// LZW: at most kLzwLanes lanes in flight, whatever the batch: strip s is lane s % lanes' k-th.  Every lane has a table of
// 4096 dwords in context scratch, interleaved by lane: kLzwLanes x 16 KiB = 256 MiB bounds the table scratch.
constexpr int kLzwLanes = 16384;
constexpr int kLzwBlock = 64;      // one wave per workgroup: a wave runs as long as its longest strip, a workgroup no longer
static_assert((size_t)kLzwLanes * kTiffLzwCodes * sizeof(uint32_t) == (size_t)256 << 20, "the table scratch bound stated in the header");
// Deflate: the same schedule with more lanes.  Every lane has kTiffInflateWords 16-bit words (decode tables and the
// code-length work area) in context scratch, interleaved by lane: kInflateLanes x 2560 bytes = 320 MiB bounds that scratch.
// A lane waits for memory at nearly every symbol, so the launch lives on the number of lanes in flight: measured on 98304
// strips of 8 KiB, 16384 lanes took 100 ms, 32768 61 ms, 65536 49 ms, 131072 35 ms.
constexpr int kInflateLanes = 131072;
constexpr int kInflateBlock = 64;
static_assert((size_t)kInflateLanes * kTiffInflateWords * sizeof(uint16_t) == (size_t)320 << 20, "the table scratch bound stated in the header");
enum { kCodecNone = 0, kCodecLzw = 1, kCodecDeflate = 2 };
// finish: a wave per row, a lane per kSegPx pixels of it, kStepPx pixels per step of the wave
constexpr int kSegPx = 16;
constexpr int kWave = 64;
constexpr int kStepPx = kSegPx * kWave;
constexpr int kFinishBlock = 256;

// One lane per strip slot (frame * strips_pitch + index), behind a memset of `status`: the strip table of every frame against
// what the two kernels below rely on -- strips in row order, rps = the first strip's rows each (the last one the rest),
// every strip inside its file's area, an uncompressed strip long enough for its rows, an LZW or Deflate strip decoding to
// at most 1 MiB, a Deflate strip of no more bytes than tiff_inflate_max_bytes allows (they bound its lane's work).  A lane that finds a fault in its frame's counts or in its own strip stores -1 into status[f] (every such lane
// the same value): the frame is zero-filled.
// Tiled files (tile_w > 0; rowb is then the bytes of a TILE's row): as many records as tiles, record i the tile i in
// row-major order, first_row = (i / across) * tile_l and rows = tile_l, what it decodes to; the same rules on its place in
// the file and on its decoded bytes, tile_l x rowb.
// record_ok is that rule on one record, strip or tile: the rows it must hold, its place in the file's area, and `need`, the
// bytes it decodes to, against its codec's limits.
__device__ inline bool record_ok(const mrgingham_amd_tiff_strip& t, int first_row, int rows, unsigned long long need, long long file_pitch,
                                 int codec) {
    return t.first_row == first_row && t.rows == rows && t.offset >= 0 && t.nbytes >= 0 && t.offset <= file_pitch &&
           t.nbytes <= file_pitch - t.offset && t.nbytes <= 0xFFFFFFFFll &&
           (codec == kCodecLzw       ? need <= kTiffLzwMaxStrip20
            : codec == kCodecDeflate ? need <= kTiffInflateMaxStrip && (unsigned long long)t.nbytes <= tiff_inflate_max_bytes(need)
                                     : (unsigned long long)t.nbytes >= need);
}

__global__ void tiff_check_kernel(const mrgingham_amd_tiff_strip* strips, int strips_pitch, const int32_t* nstrips, int nframes,
                                  int height, uint32_t rowb, long long file_pitch, int codec, int tile_w, int tile_l, int across, int down,
                                  int32_t* status) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (long long)nframes * strips_pitch) return;
    const int f = (int)(s / strips_pitch), i = (int)(s - (long long)f * strips_pitch);
    const mrgingham_amd_tiff_strip* t = strips + (long long)f * strips_pitch;
    const int ns = nstrips[f];
    bool ok = ns >= 1 && ns <= strips_pitch;
    if (ok && tile_w > 0) {
        ok = (long long)ns == (long long)across * down;
        if (ok && i < ns) ok = record_ok(t[i], (i / across) * tile_l, tile_l, (unsigned long long)tile_l * rowb, file_pitch, codec);
    } else if (ok) {
        const int rps = t[0].rows;
        ok = rps >= 1 && rps <= height && (long long)(ns - 1) * rps < height && (long long)ns * rps >= height;
        if (ok && i < ns) {
            const int first = i * rps, rows = height - first < rps ? height - first : rps;
            ok = record_ok(t[i], first, rows, (unsigned long long)rows * rowb, file_pitch, codec);
        }
    }
    if (!ok) status[f] = -1;
}

// What tiff_codec_lanes needs of a decoder: the element of a lane's table in context scratch, the table as the decoder's
// text takes it (one lane's words, at a stride of the lanes in flight), and the decoder.
struct TiffLzwLane {
    using Word = uint32_t;
    using Table = TiffLzwPackedTable;
    static __device__ __forceinline__ int decode(const uint8_t* src, uint32_t nsrc, uint8_t* out, uint32_t nout, Table& tab) {
        return tiff_lzw_decode(src, nsrc, out, nout, tab);
    }
};
struct TiffInflateLane {
    using Word = uint16_t;
    using Table = TiffInflateStridedTable;
    static __device__ __forceinline__ int decode(const uint8_t* src, uint32_t nsrc, uint8_t* out, uint32_t nout, Table& tab) {
        return tiff_inflate_decode(src, nsrc, out, nout, tab);
    }
};

// One lane per strip, lanes looping over the strips of the batch (strip slot s = frame * strips_pitch + index).  A lane
// reads src[0, nbytes) of its strip, writes the rows x rowb bytes of its strip in `raw` (frame f at raw + f*raw_pitch,
// rows dense) and keeps its table at table[lane + i * lanes]: the bounds are arguments of the decoder and were checked
// against the file's area and the frame by tiff_check_kernel, and a copy never reaches before the strip's own first byte.
// A rule broken: the lane stops, leaves the reason in strip_status and marks broken[f] (tiff_verdict_kernel).
// lane, lanes: this lane of the launch and how many there are.  The kernels form them: read in here, blockDim.x compiled to
// a choice between two words of the implicit arguments and a vector load, where the kernel's own read is one scalar word.
// TILED: rowb is the bytes of a tile's row, and tile i of frame f decodes to raw + f*raw_pitch + i * rows*rowb -- dense and
// tile-major, every tile rows = tile_l long (tiff_check_kernel), so a lane still writes its own tile's bytes alone.
template <class CODEC, bool TILED>
__device__ __forceinline__ void tiff_codec_lanes(uint32_t lane, uint32_t lanes, const uint8_t* files, long long file_pitch,
                                                 const mrgingham_amd_tiff_strip* strips, int strips_pitch, const int32_t* nstrips, int nframes,
                                                 uint32_t rowb, uint8_t* raw, long long raw_pitch, typename CODEC::Word* table, int32_t* status,
                                                 int32_t* strip_status, int32_t* broken) {
    typename CODEC::Table tab{table + lane, lanes};
    const long long total = (long long)nframes * strips_pitch;
    for (long long s = lane; s < total; s += lanes) {
        const int f = (int)(s / strips_pitch), i = (int)(s - (long long)f * strips_pitch);
        int rc = 0;
        if (status[f] == 0 && i < nstrips[f]) {  // (status: only tiff_check_kernel's verdict is read here; lanes write `broken`)
            const mrgingham_amd_tiff_strip st = strips[s];
            const long long at = TILED ? (long long)i * ((long long)st.rows * rowb) : (long long)st.first_row * rowb;
            rc = CODEC::decode(files + f * file_pitch + st.offset, (uint32_t)st.nbytes, raw + f * raw_pitch + at, (uint32_t)st.rows * rowb, tab);
            if (rc) broken[f] = 1;
        }
        if (strip_status) strip_status[s] = rc;
    }
}

template <bool TILED>
__global__ __launch_bounds__(kLzwBlock) void tiff_lzw_kernel(const uint8_t* files, long long file_pitch,
                                                             const mrgingham_amd_tiff_strip* strips, int strips_pitch,
                                                             const int32_t* nstrips, int nframes, uint32_t rowb, uint8_t* raw,
                                                             long long raw_pitch, uint32_t* table, int32_t* status,
                                                             int32_t* strip_status, int32_t* broken) {
    tiff_codec_lanes<TiffLzwLane, TILED>(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, files, file_pitch, strips, strips_pitch,
                                         nstrips, nframes, rowb, raw, raw_pitch, table, status, strip_status, broken);
}

// (flatten: with two instantiations the compiler would otherwise leave the decoder a function of its own and call it;
// inlined, the strip instantiation is the kernel it was before there were tiles.)
template <bool TILED>
__global__ __launch_bounds__(kInflateBlock) __attribute__((flatten)) void tiff_inflate_kernel(const uint8_t* files, long long file_pitch,
                                                                     const mrgingham_amd_tiff_strip* strips, int strips_pitch,
                                                                     const int32_t* nstrips, int nframes, uint32_t rowb, uint8_t* raw,
                                                                     long long raw_pitch, uint16_t* table, int32_t* status,
                                                                     int32_t* strip_status, int32_t* broken) {
    tiff_codec_lanes<TiffInflateLane, TILED>(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, files, file_pitch, strips,
                                             strips_pitch, nstrips, nframes, rowb, raw, raw_pitch, table, status, strip_status, broken);
}

// behind the LZW or Deflate launch: a frame with a broken strip gets status -1
__global__ void tiff_verdict_kernel(const int32_t* broken, int nframes, int32_t* status) {
    const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (f < nframes && broken[f]) status[f] = -1;
}

__device__ inline uint32_t load_dword(const uint8_t* __restrict__ src, long long off, long long limit) {
    if (off + 4 <= limit) return *(const uint32_t*)(src + off);
    uint32_t v = 0;  // the last dword of the last frame may end behind the buffer: its bytes one by one
    for (int i = 0; i < 4; ++i)
        if (off + i < limit) v |= (uint32_t)src[off + i] << (8 * i);
    return v;
}

__device__ inline uint32_t byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

// The row loop of both finish kernels: a grid-stride loop of waves over the rows of all frames.  Lane l of the wave takes
// pixels [x0 + 16 l, x0 + 16 l + 16) of the step that begins at x0: it loads the aligned dwords that cover them (guarded by
// `limit`, the end of the buffer), puts 16-bit samples into value order and, for predictor 2, sums them up per channel; the
// sums of the lanes to its left come from a shuffle scan over the wave, the sums of the steps before from `carry` -- a
// prefix sum modulo 2^BITS, exact in any order.  Then WhiteIsZero is inverted, and the first sample or png_grey of the first
// three is stored: 16 samples in one or two 16-byte stores where the address allows it, sample by sample at a row's
// unaligned head and tail.  A frame whose status is not 0 is zero-filled.
// Strips (!TILED; tile_w, tile_l and across are not read): the bytes of row y of frame f lie at `src` + f*src_pitch + y*rowb
// (from_raw: the LZW / Deflate launch's output) or inside the strip that holds the row (the file's own bytes, at any byte
// address).
// TILED differs in where a lane's bytes come from and in how far the sums of predictor 2 reach.  tile_w is a multiple of
// kSegPx, so the segment of a lane lies in ONE tile: tile i = (y / tile_l) * across + xs / tile_w, its row y % tile_l, at
// `src` + f*src_pitch + i * tile_l*rowb (from_raw: the codec launch's dense, tile-major output; rowb is a TILE's row) or at
// the record's offset inside the file's bytes, at any byte address (tiff_check_kernel: the whole padded tile lies inside the
// file's area).  A tile is padded to its full width, so the last lane of a row loads padding, never another tile's bytes;
// those pixels are computed and never stored.  Predictor 2 restarts at every tile's left edge: the scan over the wave is
// SEGMENTED -- a lane adds the sum from d lanes to its left only when that lane lies in the same tile (lane - d >= l0,
// the tile's first lane of this step) -- and `carry` applies only to lanes whose tile began before x0 (l0 < 0); the carry
// handed on is the last lane's inclusive sum, with the old carry where that lane's tile reaches back past x0.  (The strip
// form, carry + shuffle(sum), is not this one with l0 = -1: the two are equal only because carry is the same in every lane.)
template <int BITS, int SPP, bool TILED>
__device__ __forceinline__ void tiff_finish_rows(const uint8_t* __restrict__ src, long long src_pitch, long long limit,
                                                 const mrgingham_amd_tiff_strip* __restrict__ strips, int strips_pitch, int from_raw,
                                                 int width, int height, long long nrows, int tile_w, int tile_l, int across, int rgb,
                                                 int invert, int predictor2, int big_endian, void* __restrict__ out, long long frame_pitch,
                                                 int stride, const int32_t* __restrict__ status) {
    constexpr int ES = BITS / 8, BPP = SPP * ES, NC = SPP >= 3 ? 3 : 1, SEGB = kSegPx * BPP, ND = SEGB / 4;
    constexpr uint32_t MASK = BITS == 8 ? 255u : 65535u;
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
    // rowb: the bytes of a row of what a record holds, an image row or a tile's
    const long long nwaves = (long long)gridDim.x * (kFinishBlock / kWave), rowb = (long long)(TILED ? tile_w : width) * BPP;
    for (long long row = (long long)blockIdx.x * (kFinishBlock / kWave) + wave; row < nrows; row += nwaves) {
        const long long f = row / height;
        const int y = (int)(row - f * height);
        const bool dead = status[f] != 0;
        // strips: the row's first byte in `src`; tiles: the row's first byte inside each of its tiles, records t[0, across)
        const mrgingham_amd_tiff_strip* t = strips + f * strips_pitch;
        const int ty = TILED ? y / tile_l : 0;
        long long row_off;
        if constexpr (TILED) {
            row_off = (long long)(y - ty * tile_l) * rowb;
            t += (long long)ty * across;
        } else {
            row_off = f * src_pitch + (long long)y * rowb;
            if (!from_raw && !dead) {  // (tiff_check_kernel: strip i holds rows [i*rps, i*rps + rows), all of them inside the file's area)
                const int i = y / t[0].rows;
                row_off = f * src_pitch + t[i].offset + (long long)(y - t[i].first_row) * rowb;
            }
        }
        uint32_t carry[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) carry[c] = 0;
        for (int x0 = 0; x0 < width; x0 += kStepPx) {
            const int xs = x0 + lane * kSegPx, nx = width - xs;
            // the tile of this lane's segment and that tile's first lane of this step; below 0: the tile began in a step before
            const int tx = TILED ? xs / tile_w : 0, l0 = TILED ? tx * (tile_w / kSegPx) - x0 / kSegPx : 0;
            uint32_t v[kSegPx][NC], acc[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] = 0;
            if (!dead && nx > 0) {
                long long first;
                if constexpr (TILED) {
                    // (nx > 0: tx < across, a record tiff_check_kernel has seen)
                    const long long tile_off = from_raw ? ((long long)ty * across + tx) * (rowb * tile_l) : t[tx].offset;
                    first = f * src_pitch + tile_off + row_off + (long long)(xs - tx * tile_w) * BPP;
                } else {
                    first = row_off + (long long)xs * BPP;
                }
                const long long first4 = first & ~3ll;
                const int shift = 8 * (int)(first & 3);
                uint32_t w[ND + 1], in[ND];
#pragma unroll
                for (int i = 0; i <= ND; ++i) w[i] = load_dword(src, first4 + 4 * i, limit);
#pragma unroll
                for (int i = 0; i < ND; ++i) in[i] = (uint32_t)(((((unsigned long long)w[i + 1]) << 32) | w[i]) >> shift);
#pragma unroll
                for (int p = 0; p < kSegPx; ++p) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const int b = (p * SPP + c) * ES;
                        uint32_t s;
                        if constexpr (BITS == 8) s = byte_of(in, b);
                        else s = big_endian ? byte_of(in, b) << 8 | byte_of(in, b + 1) : byte_of(in, b + 1) << 8 | byte_of(in, b);
                        // (pixels behind the row's end are computed from whatever follows and never stored: they sit in the
                        // row's last lane, to the right of everything their sums could reach)
                        if (predictor2) s = acc[c] += s;
                        v[p][c] = s;
                    }
                }
            } else {
#pragma unroll
                for (int p = 0; p < kSegPx; ++p)
#pragma unroll
                    for (int c = 0; c < NC; ++c) v[p][c] = 0;
            }
            if (predictor2) {  // (uniform over the wave)
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    uint32_t s = nx > 0 ? acc[c] : 0;
                    const uint32_t own = s;
#pragma unroll
                    for (int d = 1; d < kWave; d <<= 1) {
                        const uint32_t u = __shfl_up(s, d, kWave);
                        if (lane >= d && (!TILED || lane - d >= l0)) s += u;
                    }
                    uint32_t before;
                    if constexpr (TILED) {
                        const uint32_t reach = l0 < 0 ? carry[c] : 0u;
                        before = s - own + reach;
                        carry[c] = __shfl(s + reach, kWave - 1, kWave);
                    } else {
                        before = s - own + carry[c];
                        carry[c] += __shfl(s, kWave - 1, kWave);
                    }
#pragma unroll
                    for (int p = 0; p < kSegPx; ++p) v[p][c] += before;
                }
            }
            if (nx <= 0) continue;
            uint32_t grey[kSegPx];
#pragma unroll
            for (int p = 0; p < kSegPx; ++p) {
                uint32_t q[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    q[c] = v[p][c] & MASK;
                    if (invert) q[c] = MASK - q[c];
                }
                uint32_t g = q[0];
                if constexpr (NC == 3) {
                    if (rgb) g = png_grey(q[0], q[1], q[2]);
                }
                grey[p] = dead ? 0u : g;
            }
            if (BITS == 8) {
                uint8_t* o = (uint8_t*)out + f * frame_pitch + (long long)y * stride + xs;
                if (nx >= kSegPx && ((uintptr_t)o & 15) == 0) {
                    uint32_t d[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) d[i] = grey[4 * i] | grey[4 * i + 1] << 8 | grey[4 * i + 2] << 16 | grey[4 * i + 3] << 24;
                    *(uint4*)o = make_uint4(d[0], d[1], d[2], d[3]);
                } else {
#pragma unroll
                    for (int p = 0; p < kSegPx; ++p)
                        if (p < nx) o[p] = (uint8_t)grey[p];
                }
            } else {
                uint16_t* o = (uint16_t*)out + f * frame_pitch + (long long)y * stride + xs;
                if (nx >= kSegPx && ((uintptr_t)o & 15) == 0) {
                    uint32_t d[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) d[i] = (grey[2 * i] & 0xFFFFu) | grey[2 * i + 1] << 16;
                    *(uint4*)o = make_uint4(d[0], d[1], d[2], d[3]);
                    *(uint4*)(o + 8) = make_uint4(d[4], d[5], d[6], d[7]);
                } else {
#pragma unroll
                    for (int p = 0; p < kSegPx; ++p)
                        if (p < nx) o[p] = (uint16_t)grey[p];
                }
            }
        }
    }
}

template <int BITS, int SPP>
__global__ __launch_bounds__(kFinishBlock) void tiff_finish_kernel(const uint8_t* __restrict__ src, long long src_pitch, long long limit,
                                                                   const mrgingham_amd_tiff_strip* __restrict__ strips, int strips_pitch,
                                                                   int from_raw, int width, int height, long long nrows, int rgb,
                                                                   int invert, int predictor2, int big_endian, void* __restrict__ out,
                                                                   long long frame_pitch, int stride, const int32_t* __restrict__ status) {
    tiff_finish_rows<BITS, SPP, false>(src, src_pitch, limit, strips, strips_pitch, from_raw, width, height, nrows, 0, 0, 0, rgb, invert,
                                       predictor2, big_endian, out, frame_pitch, stride, status);
}

template <int BITS, int SPP>
__global__ __launch_bounds__(kFinishBlock) void tiff_finish_tiles_kernel(const uint8_t* __restrict__ src, long long src_pitch, long long limit,
                                                                         const mrgingham_amd_tiff_strip* __restrict__ strips, int strips_pitch,
                                                                         int from_raw, int width, int height, long long nrows, int tile_w,
                                                                         int tile_l, int across, int rgb, int invert, int predictor2,
                                                                         int big_endian, void* __restrict__ out, long long frame_pitch,
                                                                         int stride, const int32_t* __restrict__ status) {
    tiff_finish_rows<BITS, SPP, true>(src, src_pitch, limit, strips, strips_pitch, from_raw, width, height, nrows, tile_w, tile_l, across, rgb,
                                      invert, predictor2, big_endian, out, frame_pitch, stride, status);
}

bool tiff_info_ok(const mrgingham_amd_tiff_info& t) {
    return t.width >= 1 && t.height >= 1 && t.width <= 32767 && t.height <= 32767 && (t.bits == 8 || t.bits == 16) && t.samples >= 1 &&
           t.samples <= 4 && t.photometric >= 0 && t.photometric <= 2 && (t.photometric != 2 || t.samples >= 3) &&
           (t.compression == 1 || t.compression == 5 || t.compression == 8 || t.compression == 32946) && (t.predictor == 1 || t.predictor == 2) && (t.big_endian == 0 || t.big_endian == 1);
}

int lzw_lanes_of(const mrgingham_amd_ctx* ctx) { return ctx->tiff_lzw_lanes > 0 ? ctx->tiff_lzw_lanes : kLzwLanes; }
int inflate_lanes_of(const mrgingham_amd_ctx* ctx) { return ctx->tiff_deflate_lanes > 0 ? ctx->tiff_deflate_lanes : kInflateLanes; }
int codec_of(const mrgingham_amd_tiff_info& t) { return t.compression == 5 ? kCodecLzw : t.compression == 1 ? kCodecNone : kCodecDeflate; }

template <int N>
using Int = std::integral_constant<int, N>;

// checked arguments -> the launches; grows the LZW / Deflate scratch.  tile_w == tile_l == 0: strip files.
int launch_tiff_decode(mrgingham_amd_ctx* ctx, const uint8_t* d_files, int64_t file_pitch, const mrgingham_amd_tiff_strip* d_strips,
                       int strips_pitch, const int32_t* d_nstrips, int nframes, const mrgingham_amd_tiff_info& ti, int tile_w, int tile_l,
                       void* d_out, int64_t frame_pitch, int stride, int32_t* d_status, int32_t* d_strip_status, hipStream_t s) {
    const int width = ti.width, height = ti.height, bpp = ti.samples * ti.bits / 8;
    const bool tiled = tile_w > 0;
    const int across = tiled ? (width + tile_w - 1) / tile_w : 0, down = tiled ? (height + tile_l - 1) / tile_l : 0;
    // the bytes of a row of what a lane decodes: an image row, or a tile's
    const uint32_t rowb = (uint32_t)(tiled ? tile_w : width) * bpp;
    const int codec = codec_of(ti);
    const bool lzw = codec == kCodecLzw, from_raw = codec != kCodecNone;
    const unsigned frame_blocks = (unsigned)((nframes + 63) / 64);
    const long long slots = (long long)nframes * strips_pitch;
    MRG_HIP_CHECK(hipMemsetAsync(d_status, 0, (size_t)nframes * sizeof(int32_t), s));
    hipLaunchKernelGGL(tiff_check_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, d_strips, strips_pitch, d_nstrips, nframes, height,
                       rowb, (long long)file_pitch, codec, tile_w, tile_l, across, down, d_status);
    const uint8_t* src = d_files;
    long long src_pitch = file_pitch;
    if (from_raw) {
        static_assert(kLzwBlock == kInflateBlock, "one rounding of the lanes for both");
        static_assert(kTiffLzwMaxStrip20 == kTiffInflateMaxStrip, "one limit on a tile's decoded bytes");
        long long raw_bytes = (long long)rowb * height;
        if (tiled) {
            // across * down tiles of tile_l x rowb bytes each.  Tiles of more than 1 MiB, or more tiles than strips_pitch
            // records: tiff_check_kernel calls every frame dead, no lane decodes and no row is read -- nothing to hold
            const long long tile_bytes = (long long)rowb * tile_l, tiles = (long long)across * down;
            raw_bytes = tile_bytes > (long long)kTiffLzwMaxStrip20 || tiles > strips_pitch ? 16 : tiles * tile_bytes;
        }
        const long long raw_pitch = (raw_bytes + 15) & ~15ll;
        const int most = lzw ? lzw_lanes_of(ctx) : inflate_lanes_of(ctx);
        long long lanes = (slots + kLzwBlock - 1) / kLzwBlock * kLzwBlock;
        if (lanes > most) lanes = most;
        int rc;
        if ((rc = ensure(ctx, ctx->tiff_raw, (size_t)nframes * (size_t)raw_pitch))) return rc;
        if (lzw) rc = ensure(ctx, ctx->tiff_table, (size_t)lanes * kTiffLzwCodes * sizeof(uint32_t));
        else rc = ensure(ctx, ctx->tiff_inflate_table, (size_t)lanes * kTiffInflateWords * sizeof(uint16_t));
        if (rc) return rc;
        if ((rc = ensure(ctx, ctx->tiff_broken, (size_t)nframes * sizeof(int32_t)))) return rc;
        MRG_HIP_CHECK(hipMemsetAsync(ctx->tiff_broken.p, 0, (size_t)nframes * sizeof(int32_t), s));
        // the one codec launch: the kernel of this codec and layout, and its table
        auto decode = [&](auto kernel, auto* table) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)(lanes / kLzwBlock)), dim3(kLzwBlock), 0, s, d_files, (long long)file_pitch, d_strips,
                               strips_pitch, d_nstrips, nframes, rowb, (uint8_t*)ctx->tiff_raw.p, raw_pitch, table, d_status, d_strip_status,
                               (int32_t*)ctx->tiff_broken.p);
        };
        if (lzw) decode(tiled ? tiff_lzw_kernel<true> : tiff_lzw_kernel<false>, (uint32_t*)ctx->tiff_table.p);
        else decode(tiled ? tiff_inflate_kernel<true> : tiff_inflate_kernel<false>, (uint16_t*)ctx->tiff_inflate_table.p);
        hipLaunchKernelGGL(tiff_verdict_kernel, dim3(frame_blocks), dim3(64), 0, s, (const int32_t*)ctx->tiff_broken.p, nframes, d_status);
        src = (const uint8_t*)ctx->tiff_raw.p;
        src_pitch = raw_pitch;
    }
    const long long nrows = (long long)nframes * height, limit = (long long)nframes * src_pitch;
    int cus = 0;
    MRG_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    // sized to the device: eight workgroups of 256 lanes fill a CU
    long long blocks = (nrows + kFinishBlock / kWave - 1) / (kFinishBlock / kWave);
    if (blocks > (long long)cus * 8) blocks = (long long)cus * 8;
    // the one finish launch; tile_args: what tiff_finish_tiles_kernel takes between nrows and rgb, nothing for strips
    auto finish = [&](auto kernel, auto... tile_args) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kFinishBlock), 0, s, src, src_pitch, limit, d_strips, strips_pitch,
                           from_raw ? 1 : 0, width, height, nrows, tile_args..., ti.photometric == 2 ? 1 : 0, ti.photometric == 0 ? 1 : 0,
                           ti.predictor == 2 ? 1 : 0, ti.big_endian, d_out, (long long)frame_pitch, stride, (const int32_t*)d_status);
    };
    auto finish_of = [&](auto bits, auto samples) {
        constexpr int B = decltype(bits)::value, C = decltype(samples)::value;
        if (tiled) finish(tiff_finish_tiles_kernel<B, C>, tile_w, tile_l, across);
        else finish(tiff_finish_kernel<B, C>);
    };
    auto by_samples = [&](auto bits) {
        switch (ti.samples) {
            case 1: finish_of(bits, Int<1>{}); break;
            case 2: finish_of(bits, Int<2>{}); break;
            case 3: finish_of(bits, Int<3>{}); break;
            default: finish_of(bits, Int<4>{}); break;
        }
    };
    if (ti.bits == 8) by_samples(Int<8>{});
    else by_samples(Int<16>{});
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

// what makes two files of a chunk share a launch: the fields of the kernels' arguments, the tile sizes among them (0 and 0
// for strips)
uint64_t launch_key(const mrgingham_amd_tiff_info& t, int tile_w, int tile_l) {
    return (uint64_t)t.samples | (uint64_t)t.photometric << 4 | (uint64_t)codec_of(t) << 8 | (uint64_t)t.predictor << 12 |
           (uint64_t)t.big_endian << 16 | (uint64_t)tile_w << 20 | (uint64_t)tile_l << 36;
}

bool tile_sizes_ok(int tile_w, int tile_l) {
    if (tile_w == 0 && tile_l == 0) return true;
    return tile_w >= kSegPx && tile_l >= 1 && tile_w <= 32767 && tile_l <= 32767 && tile_w % kSegPx == 0;
}

// ---- the loader's decision on one file
// kind: -1 failed, 0 decoded on the host (its samples lie in its area), 1 the device's (its bytes lie in its area, its
// records in its slot of the table); status: what the caller's h_status gets for now; tile: a tiled file's tile width and
// length, 0 and 0 for strips; nrecords: the strips or tiles of a device file, 0 otherwise.
struct TiffTile { int32_t w = 0, l = 0; };
struct TiffRoute {
    int kind = -1;
    int32_t status = -1;
    mrgingham_amd_tiff_info info{};
    TiffTile tile;
    int32_t nrecords = 0;
};
struct TiffHostBuffers { std::vector<uint8_t> file; Image im; };  // a host thread's own, reused from file to file

// Reads `name` straight into `dst` (its area of the staging, `area` bytes), parses it into `records` (`height` of them) and
// says who decodes it; a file for the host is decoded here, into `dst`.
TiffRoute route_tiff_file(const char* name, uint8_t* dst, size_t area, mrgingham_amd_tiff_strip* records, int width, int height, int bits,
                          int64_t max_strip, int64_t deflate_strip, TiffHostBuffers& t) {
    const size_t px_bytes = (size_t)width * height * (bits / 8);
    TiffRoute r;
    try {
        size_t ns = 0;
        int head = -1;
        bool staged = false;
        FILE* f = fopen(name, "rb");
        if (f) {
            // the file straight into its area (one that has grown since it was measured, or is too large: the host's)
            const size_t got = fread(dst, 1, area, f);
            const bool whole = got < area || fgetc(f) == EOF;
            fclose(f);
            if (whole) {
                staged = true;
                head = tiff_layout_tiled(dst, got, max_strip, deflate_strip, &r.info, &r.tile.w, &r.tile.l, records, (size_t)height, &ns);
            } else if (read_file(name, t.file)) {
                head = tiff_layout_tiled(t.file.data(), t.file.size(), max_strip, deflate_strip, &r.info, &r.tile.w, &r.tile.l, nullptr, 0, &ns);
                if (head == 0) head = kTiffNotTaken;
            }
        }
        // (-2: more strips than rows of THIS batch's frames -- a file of another height; or a tiled file with more
        // tiles than rows, which a slot has no records for: the host decoder's)
        if (head == -2 && r.tile.w > 0 && r.info.height == height) head = kTiffNotTaken;
        // (and so does one whose tiles are mostly padding: the device holds every tile of a chunk decoded, the host
        // decoder one tile; four times what the samples of a frame of four channels take, and 1 MiB, pass)
        if (head == 0 && r.tile.w > 0 &&
            (uint64_t)ns * r.tile.w * r.tile.l * r.info.samples * (r.info.bits / 8) > 16 * (uint64_t)px_bytes + (1u << 20))
            head = kTiffNotTaken;
        if (head == 0 || head == kTiffNotTaken || head == -2) {
            if (r.info.width != width || r.info.height != height || r.info.bits != bits) r.status = -2;
            else if (head == 0 && staged) {
                r.nrecords = (int32_t)ns;
                r.kind = 1;
                r.status = 0;  // (an LZW or Deflate strip may still break a rule: known when the chunk has passed the stream)
            } else if (head != -2 && read_image(name, t.im) && t.im.depth == bits && t.im.w == width && t.im.h == height) {
                // the device route does not take it: the host decoder's samples
                memcpy(dst, bits == 8 ? (const void*)t.im.px8.data() : (const void*)t.im.px16.data(), px_bytes);
                r.kind = 0;
                r.status = 0;
            }
        }
    } catch (...) {  // std::bad_alloc on a file too large to hold
        r = TiffRoute{};
    }
    return r;
}

}  // namespace

extern "C" {

int mrgingham_amd_tiff_inflate_lanes(void) { return kInflateLanes; }

void mrgingham_amd_tiff_geometry(int* lzw_lanes, int* segment_pixels, int* step_pixels) {
    if (lzw_lanes) *lzw_lanes = kLzwLanes;
    if (segment_pixels) *segment_pixels = kSegPx;
    if (step_pixels) *step_pixels = kStepPx;
}

int mrgingham_amd_tiff_decode_batch_tiled(mrgingham_amd_ctx* ctx, const uint8_t* d_files, int64_t file_pitch,
                                          const mrgingham_amd_tiff_strip* d_records, int records_pitch, const int32_t* d_nrecords,
                                          int nframes, const mrgingham_amd_tiff_info* info, int tile_width, int tile_length, void* d_out,
                                          int64_t frame_pitch, int stride, int32_t* d_status, int32_t* d_strip_status, void* stream) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (!info || nframes < 0 || records_pitch < 1 || frame_pitch < 0 || file_pitch < 0 ||
        (nframes > 0 && (!d_files || !d_records || !d_nrecords || !d_out || !d_status)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad TIFF batch descriptor");
    if (!tiff_info_ok(*info) || stride < info->width)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "TIFF batch: sides 1..32767, 8 or 16 bits, 1..4 samples, photometric 0..2, compression 1, 5, 8 or 32946, predictor 1 or 2, stride >= width");
    if (!tile_sizes_ok(tile_width, tile_length))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "TIFF batch: tile width and length both 0 (strips), or a width that is a multiple of 16 and a length, 1..32767 each");
    if ((file_pitch & 15) || ((uintptr_t)d_files & 15) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_nrecords & 3) || ((uintptr_t)d_status & 3) ||
        ((uintptr_t)d_strip_status & 3) || (info->bits == 16 && ((uintptr_t)d_out & 1)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "TIFF batch: files 16-byte aligned, file_pitch a multiple of 16; 16-bit frames 2-byte aligned");
    if (nframes == 0) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    return launch_tiff_decode(ctx, d_files, file_pitch, d_records, records_pitch, d_nrecords, nframes, *info, tile_width, tile_length, d_out,
                              frame_pitch, stride, d_status, d_strip_status, (hipStream_t)stream);  // (the stream used as given: NULL is HIP's default stream)
}

int mrgingham_amd_tiff_decode_batch(mrgingham_amd_ctx* ctx, const uint8_t* d_files, int64_t file_pitch,
                                    const mrgingham_amd_tiff_strip* d_strips, int strips_pitch, const int32_t* d_nstrips, int nframes,
                                    const mrgingham_amd_tiff_info* info, void* d_out, int64_t frame_pitch, int stride, int32_t* d_status,
                                    int32_t* d_strip_status, void* stream) {
    return mrgingham_amd_tiff_decode_batch_tiled(ctx, d_files, file_pitch, d_strips, strips_pitch, d_nstrips, nframes, info, 0, 0, d_out,
                                                 frame_pitch, stride, d_status, d_strip_status, stream);
}

int mrgingham_amd_read_tiffs_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height, int bits,
                                   void* d_out, int64_t frame_pitch, int stride, int nthreads, int32_t* h_status) {
    const size_t es = bits == 8 ? 1 : bits == 16 ? 2 : 0;
    int rc = check_file_batch(ctx, "TIFF", filenames, nfiles, width, height, es, d_out, frame_pitch, stride, h_status);
    if (rc) return rc;
    if (nfiles == 0) return 0;
    fb_drain(ctx);
    const CallerDevice caller_device_;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    nthreads = host_threads(nthreads);
    uint8_t* const out = (uint8_t*)d_out;

    // Every file of a chunk gets ONE area of the staging: the largest file of the list, or the decoded samples where those
    // are more (a file the host decodes leaves them there).  A file much larger than the samples of a frame of four
    // channels -- hardly a TIFF of this size -- does not size the areas: it keeps the host decoder.
    const size_t px_bytes = (size_t)width * height * es;
    const size_t file_limit = 4 * px_bytes + 16 * (size_t)height + 65536;
    std::vector<size_t> fsize((size_t)nfiles, 0);
    for_files(ctx->pool, nthreads, nfiles, [&](int i) {
        FILE* f = fopen(filenames[i], "rb");
        if (!f) return;
        if (fseek(f, 0, SEEK_END) == 0) {
            const long n = ftell(f);
            if (n > 0) fsize[(size_t)i] = (size_t)n;
        }
        fclose(f);
    });
    size_t largest = px_bytes;
    for (size_t n : fsize)
        if (n <= file_limit && n > largest) largest = n;
    const size_t area = (largest + 15) & ~(size_t)15;
    const size_t per_file = area + (size_t)height * sizeof(mrgingham_amd_tiff_strip) + 2 * sizeof(int32_t);
    const int chunk = loader_chunk_frames(ctx->jpeg_coef_budget, per_file, nfiles, nthreads, ctx->tiff_chunk_frames);
    // a slot, page-locked and on the device alike: the files' areas | their strip tables, `height` records each | their
    // strip counts | (device -> host) their status words
    const size_t off_strips = (size_t)chunk * area, off_ns = off_strips + (size_t)chunk * height * sizeof(mrgingham_amd_tiff_strip),
                 off_status = off_ns + (size_t)chunk * sizeof(int32_t), slot_bytes = off_status + (size_t)chunk * sizeof(int32_t);
    hipStream_t s = ctx->pix;
    const int64_t max_strip = ctx->tiff_lzw_max_strip, deflate_strip = ctx->tiff_deflate ? ctx->tiff_deflate_max_strip : 0;
    struct InSlot { int f0 = 0, n = 0; std::vector<TiffRoute> file; } in_slot[2];  // per slot, the files of its chunk
    auto stage = [&](int k, int f0, int n) -> int {
        uint8_t* const pin = (uint8_t*)ctx->loader_slot[k].pin.p;
        mrgingham_amd_tiff_strip* const h_strips = (mrgingham_amd_tiff_strip*)(pin + off_strips);
        int32_t* const h_ns = (int32_t*)(pin + off_ns);
        InSlot& S = in_slot[k];
        S.f0 = f0; S.n = n;
        S.file.assign((size_t)n, TiffRoute{});
        // 1. every file: who decodes it
        for_files<TiffHostBuffers>(ctx->pool, nthreads, n, [&](int i, TiffHostBuffers& t) {
            const TiffRoute r = route_tiff_file(filenames[f0 + i], pin + (size_t)i * area, area, h_strips + (size_t)i * height, width, height, bits,
                                                max_strip, deflate_strip, t);
            h_ns[i] = r.nrecords;
            h_status[f0 + i] = r.status;
            S.file[(size_t)i] = r;
        });
        // 2. The host threads wrote file i's records at a pitch of `height`, the most a file can have.  The launches get a dense
        // table: the records moved down to a pitch of the chunk's largest strip count (i * P <= i * height: ascending i never
        // overwrites what is still to move), so that the lanes of the LZW launch, which take slot after slot, meet no runs of
        // empty slots -- a pitch of `height` would leave most lanes idle and stack the strips on the others.
        int P = 1;
        for (int i = 0; i < n; ++i)
            if (h_ns[i] > P) P = h_ns[i];
        for (int i = 1; i < n && P < height; ++i)
            if (h_ns[i] > 0) memmove(h_strips + (size_t)i * P, h_strips + (size_t)i * height, (size_t)h_ns[i] * sizeof(mrgingham_amd_tiff_strip));
        // 3. three uploads (areas; tables; counts)
        uint8_t* const dev = (uint8_t*)ctx->loader_slot[k].dev.p;
        MRG_HIP_CHECK(hipMemcpyAsync(dev, pin, (size_t)n * area, hipMemcpyHostToDevice, s));
        MRG_HIP_CHECK(hipMemcpyAsync(dev + off_strips, pin + off_strips, (size_t)n * P * sizeof(mrgingham_amd_tiff_strip), hipMemcpyHostToDevice, s));
        MRG_HIP_CHECK(hipMemcpyAsync(dev + off_ns, pin + off_ns, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        MRG_HIP_CHECK(hipMemsetAsync(dev + off_status, 0, (size_t)n * sizeof(int32_t), s));
        // 4. one launch sequence per run of files of one kind and one set of fields
        auto same = [&](int a, int b) {
            const TiffRoute &A = S.file[(size_t)a], &B = S.file[(size_t)b];
            return A.kind == B.kind && (A.kind != 1 || launch_key(A.info, A.tile.w, A.tile.l) == launch_key(B.info, B.tile.w, B.tile.l));
        };
        for (int i = 0; i < n;) {
            int e = i + 1;
            while (e < n && same(i, e)) ++e;
            const TiffRoute& R = S.file[(size_t)i];
            if (R.kind == 1) {
                int lrc;
                if ((lrc = launch_tiff_decode(ctx, dev + (size_t)i * area, (int64_t)area, (const mrgingham_amd_tiff_strip*)(dev + off_strips) + (size_t)i * P,
                                              P, (const int32_t*)(dev + off_ns) + i, e - i, R.info, R.tile.w, R.tile.l,
                                              out +(size_t)(f0 + i) * frame_pitch * es, frame_pitch, stride, (int32_t*)(dev + off_status) + i, nullptr, s)))
                    return lrc;
            } else if (R.kind == 0) {
                for (int q = i; q < e; ++q)
                    MRG_HIP_CHECK(hipMemcpy2DAsync(out + (size_t)(f0 + q) * frame_pitch * es, (size_t)stride * es, dev + (size_t)q * area,
                                                   (size_t)width * es, (size_t)width * es, (size_t)height, hipMemcpyDeviceToDevice, s));
            } else {
                for (int q = i; q < e; ++q) MRG_HIP_CHECK(zero_frame(d_out, f0 + q, frame_pitch, stride, width, height, es, s));
            }
            i = e;
        }
        MRG_HIP_CHECK(hipMemcpyAsync(pin + off_status, dev + off_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        return 0;
    };
    // the chunk has passed the stream: the verdicts of the device's files (their frames are zero-filled already)
    auto finish = [&](int k) -> int {
        const InSlot& S = in_slot[k];
        const int32_t* st = (const int32_t*)((const uint8_t*)ctx->loader_slot[k].pin.p + off_status);
        for (int i = 0; i < S.n; ++i)
            if (S.file[(size_t)i].kind == 1 && st[i] != 0) h_status[S.f0 + i] = -1;
        return 0;
    };
    // the chunk slots are shared with the other loaders (ctx.h: loader_slot)
    return loader_ring(ctx, nfiles, chunk, slot_bytes, slot_bytes, stage, nullptr, finish);
}

}  // extern "C"
