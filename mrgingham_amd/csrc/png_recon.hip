// PNG on the device: the row filters undone and the samples reduced to grey, from the scanlines a host thread has inflated
// (image_io.cpp: png_scanlines), and the batch loader that keeps host threads, the upload and the kernel busy side by
// side.  See include/mrgingham_amd.h for the contract of the entry points and DESIGN.md section 4.12 for the schedule
// and what bounds the kernel.
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "ctx.h"
#include "image_io.h"
#include "loader.h"
#include "png_filter.h"

using namespace mrg;

namespace {

constexpr int kRows = 256;   // R: rows of a frame in flight = lanes of the workgroup that takes the frame
constexpr int kSegPx = 16;   // S: pixels of a row a lane reconstructs per step

__device__ inline uint32_t load_scan_dword(const uint8_t* __restrict__ scan, long long off, long long limit) {
    if (off + 4 <= limit) return *(const uint32_t*)(scan + off);
    uint32_t v = 0;  // the last dword of the last frame may end behind the buffer: its bytes one by one
    for (int i = 0; i < 4; ++i)
        if (off + i < limit) v |= (uint32_t)scan[off + i] << (8 * i);
    return v;
}

__device__ inline uint32_t byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

// One workgroup per frame, lane j takes rows j, j + R, j + 2R, ...  A byte needs the byte one pixel to its left, the byte
// above and the byte above that one, so the rows advance as a wavefront: lane j reconstructs segment k (S pixels) of its
// b-th row at step b * max(nseg, R) + j + k, one step behind the lane above it, and a workgroup barrier ends every
// step.  What a lane carries from segment to segment -- the pixel to the left and the one above it -- stays in
// registers; the reconstructed segment goes to the lane below through LDS, slot[step & 1][quad][lane] (written in step t,
// read in step t + 1, written again in step t + 2: one barrier between any two of them; consecutive lanes hold
// consecutive 16-byte words, so every ds_read_b128 / ds_write_b128 of a wave is one contiguous run).  Only the rows of
// lane R - 1 are read a whole round later, by lane 0: they go through `rowbuf`, one padded row per workgroup in global
// memory (the barrier orders its store and its load: both sit in the workgroup's own CU).  A lane stores nothing but its
// S grey samples: the reconstructed colour bytes never reach memory.
// The filtered bytes of a segment begin at any byte address: the lane loads the aligned dwords that cover them (guarded
// by `scan_limit`, the end of the last frame) and shifts.  Bytes of the last segment beyond the row are computed from
// whatever follows and never stored.  The filter type was checked on the host (0 .. 4).
template <int BITS, int CH>
__global__ __launch_bounds__(kRows) void png_recon_kernel(const uint8_t* __restrict__ scan, long long scan_pitch, long long scan_limit,
                                                          int width, int height, void* __restrict__ out, long long frame_pitch,
                                                          int stride, uint8_t* rowbuf, long long rowpad) {
    constexpr int BPP = CH * BITS / 8, NQ = BPP, ND = NQ * 4, SEGB = kSegPx * BPP;
    __shared__ uint4 slot[2][NQ][kRows];
    const int j = threadIdx.x, f = blockIdx.x;
    const long long rowb = (long long)width * BPP, frame_off = (long long)f * scan_pitch;
    const int nseg = (width + kSegPx - 1) / kSegPx;
    const int M = nseg > kRows ? nseg : kRows;
    const int rounds = (height + kRows - 1) / kRows;
    const int nsteps = (rounds - 1) * M + (height - 1 - (rounds - 1) * kRows) + nseg;  // (at most 128 * 2048 + 255 + 2048)
    uint8_t* const myrow = rowbuf + (long long)f * rowpad;
    int k = -j, y = j, ft = 0;  // this step: segment k of row y (k outside [0, nseg) or y >= height: nothing)
    uint32_t a[BPP] = {}, c[BPP] = {};
    for (int t = 0; t < nsteps; ++t) {
        const int buf = t & 1;
        if (k >= 0 && k < nseg && y < height) {
            const long long row_off = frame_off + (rowb + 1) * y;
            if (k == 0) {
                ft = scan[row_off];
#pragma unroll
                for (int q = 0; q < BPP; ++q) a[q] = c[q] = 0;
            }
            const long long first = row_off + 1 + (long long)k * SEGB, first4 = first & ~3ll;
            const int shift = 8 * (int)(first & 3);
            uint32_t w[ND + 1], in[ND], up[ND], cur[ND];
#pragma unroll
            for (int i = 0; i <= ND; ++i) w[i] = load_scan_dword(scan, first4 + 4 * i, scan_limit);
#pragma unroll
            for (int i = 0; i < ND; ++i) in[i] = (uint32_t)(((((unsigned long long)w[i + 1]) << 32) | w[i]) >> shift);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                uint4 u = make_uint4(0, 0, 0, 0);
                if (y > 0) u = j > 0 ? slot[buf ^ 1][q][j - 1] : *(const uint4*)(myrow + (long long)k * SEGB + q * 16);
                up[4 * q] = u.x; up[4 * q + 1] = u.y; up[4 * q + 2] = u.z; up[4 * q + 3] = u.w;
            }
#pragma unroll
            for (int i = 0; i < ND; ++i) cur[i] = 0;
            uint32_t grey[kSegPx];
#pragma unroll
            for (int p = 0; p < kSegPx; ++p) {
                uint32_t px[BPP];
#pragma unroll
                for (int q = 0; q < BPP; ++q) {
                    const int i = p * BPP + q;
                    const uint32_t above = byte_of(up, i);
                    const uint32_t v = (byte_of(in, i) + (uint32_t)png_predict_select(ft, (int)a[q], (int)above, (int)c[q])) & 255u;
                    c[q] = above;
                    a[q] = v;
                    px[q] = v;
                    cur[i >> 2] |= v << (8 * (i & 3));
                }
                // grey: the first channel, or the weighted colour channels; alpha is ignored; 16-bit samples are big-endian pairs
                if constexpr (BITS == 8 && CH < 3) grey[p] = px[0];
                else if constexpr (BITS == 8) grey[p] = png_grey(px[0], px[1], px[2]);
                else if constexpr (CH < 3) grey[p] = px[0] << 8 | px[1];
                else grey[p] = png_grey(px[0] << 8 | px[1], px[2] << 8 | px[3], px[4] << 8 | px[5]);
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const uint4 v = make_uint4(cur[4 * q], cur[4 * q + 1], cur[4 * q + 2], cur[4 * q + 3]);
                slot[buf][q][j] = v;
                if (j == kRows - 1) *(uint4*)(myrow + (long long)k * SEGB + q * 16) = v;
            }
            const int x0 = k * kSegPx, nx = width - x0;
            if (BITS == 8) {
                uint8_t* o = (uint8_t*)out + (long long)f * frame_pitch + (long long)y * stride + x0;
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
                uint16_t* o = (uint16_t*)out + (long long)f * frame_pitch + (long long)y * stride + x0;
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
        if (++k == M) {
            k = 0;
            y += kRows;
        }
        __syncthreads();
    }
}

template <int BITS, int CH>
void launch_one(const uint8_t* d_scan, int64_t scan_pitch, long long limit, int nframes, int width, int height, void* d_out,
                int64_t frame_pitch, int stride, uint8_t* rowbuf, long long rowpad, hipStream_t s) {
    hipLaunchKernelGGL((png_recon_kernel<BITS, CH>), dim3((unsigned)nframes), dim3(kRows), 0, s, d_scan, (long long)scan_pitch, limit,
                       width, height, d_out, (long long)frame_pitch, stride, rowbuf, rowpad);
}

// checked arguments -> the launch; grows the row scratch
int launch_png_recon(mrgingham_amd_ctx* ctx, const uint8_t* d_scan, int64_t scan_pitch, int nframes, int width, int height, int bits,
                     int color_type, void* d_out, int64_t frame_pitch, int stride, hipStream_t s) {
    const int bpp = png_bpp(bits, color_type);
    const long long rowb = (long long)width * bpp;
    const long long rowpad = (long long)((width + kSegPx - 1) / kSegPx) * kSegPx * bpp;  // whole segments: a multiple of 16
    const long long limit = (long long)(nframes - 1) * scan_pitch + (rowb + 1) * height;
    const int rc = ensure(ctx, ctx->png_row, (size_t)nframes * (size_t)rowpad);
    if (rc) return rc;
    uint8_t* rowbuf = (uint8_t*)ctx->png_row.p;
#define MRG_PNG_CASE(B, C) launch_one<B, C>(d_scan, scan_pitch, limit, nframes, width, height, d_out, frame_pitch, stride, rowbuf, rowpad, s)
    const int ch = bpp * 8 / bits;
    if (bits == 8) {
        if (ch == 1) MRG_PNG_CASE(8, 1); else if (ch == 2) MRG_PNG_CASE(8, 2); else if (ch == 3) MRG_PNG_CASE(8, 3); else MRG_PNG_CASE(8, 4);
    } else {
        if (ch == 1) MRG_PNG_CASE(16, 1); else if (ch == 2) MRG_PNG_CASE(16, 2); else if (ch == 3) MRG_PNG_CASE(16, 3); else MRG_PNG_CASE(16, 4);
    }
#undef MRG_PNG_CASE
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

void mrgingham_amd_png_reconstruct_geometry(int* rows_in_flight, int* segment_pixels) {
    if (rows_in_flight) *rows_in_flight = kRows;
    if (segment_pixels) *segment_pixels = kSegPx;
}

int mrgingham_amd_png_reconstruct_batch(mrgingham_amd_ctx* ctx, const uint8_t* d_scan, int64_t scan_pitch, int nframes, int width,
                                        int height, int bits, int color_type, void* d_out, int64_t frame_pitch, int stride,
                                        void* stream) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (nframes < 0 || width < 0 || height < 0 || stride < width || frame_pitch < 0 || scan_pitch < 0 || (nframes > 0 && (!d_scan || !d_out)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad PNG scanline batch descriptor");
    if (width > 32767 || height > 32767)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "frames larger than 32767 pixels per side are not supported");
    const int bpp = png_bpp(bits, color_type);
    if (!bpp) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "PNG scanlines: 8 or 16 bits, colour type 0, 2, 4 or 6");
    if (scan_pitch < ((int64_t)width * bpp + 1) * height || ((uintptr_t)d_scan & 3) || (bits == 16 && ((uintptr_t)d_out & 1)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "PNG scanlines: 4-byte aligned, scan_pitch at least (width*bpp + 1)*height; 16-bit frames 2-byte aligned");
    if (nframes == 0 || width == 0 || height == 0) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    return launch_png_recon(ctx, d_scan, scan_pitch, nframes, width, height, bits, color_type, d_out, frame_pitch, stride,
                            (hipStream_t)stream);  // (the stream used as given: NULL is HIP's default stream)
}

int mrgingham_amd_read_pngs_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height, int bits,
                                  void* d_out, int64_t frame_pitch, int stride, int nthreads, int32_t* h_status) {
    const size_t es = bits == 8 ? 1 : bits == 16 ? 2 : 0;
    int rc = check_file_batch(ctx, "PNG", filenames, nfiles, width, height, es, d_out, frame_pitch, stride, h_status);
    if (rc) return rc;
    if (nfiles == 0) return 0;
    fb_drain(ctx);
    const CallerDevice caller_device_;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    nthreads = host_threads(nthreads);
    uint8_t* const out = (uint8_t*)d_out;

    // every file of a chunk gets ONE area of the staging, sized for the widest pixel the headers of this size and depth
    // announce (a palette file's host-decoded bytes fit any area: width * height < (width + 1) * height)
    std::vector<int> file_bpp((size_t)nfiles, 1);
    for_files(ctx->pool, nthreads, nfiles, [&](int i) {
        int w = 0, h = 0, b = 0;
        const int ct = png_header(filenames[i], &w, &h, &b);
        if (ct >= 0 && w == width && h == height && b == bits) file_bpp[(size_t)i] = png_bpp(b, ct);
    });
    const int most_bpp = *std::max_element(file_bpp.begin(), file_bpp.end());
    const size_t area = (((size_t)width * most_bpp + 1) * height + 15) & ~(size_t)15;
    const int chunk = loader_chunk_frames(ctx->jpeg_coef_budget, area, nfiles, nthreads, ctx->png_chunk_frames);
    hipStream_t s = ctx->pix;
    std::vector<int> kind((size_t)chunk);  // per file of the chunk: its colour type, 3 = decoded on the host, -1 = failed
    struct Buffers { std::vector<uint8_t> file; Image im; };
    auto stage = [&](int k, int f0, int n) -> int {
        uint8_t* h_scan = (uint8_t*)ctx->loader_slot[k].pin.p;
        for_files<Buffers>(ctx->pool, nthreads, n, [&](int i, Buffers& t) {
            int32_t st = -1;
            int w = 0, h = 0, b = 0, ct = -1;
            uint8_t* dst = h_scan + (size_t)i * area;
            try {
                if (read_file(filenames[f0 + i], t.file)) {
                    const int head = png_scanlines(t.file.data(), t.file.size(), nullptr, 0, &w, &h, &b, &ct);
                    if (head == 0 || head == kPngNotTaken) {
                        if (w != width || h != height || b != bits) st = -2;
                        else if (head == 0) st = png_scanlines(t.file.data(), t.file.size(), dst, area, &w, &h, &b, &ct) == 0 ? 0 : -1;
                        else if (read_image(filenames[f0 + i], t.im) && t.im.depth == 8 && t.im.w == width && t.im.h == height) {
                            memcpy(dst, t.im.px8.data(), (size_t)width * height);  // the device route does not take it: the host decoder's bytes
                            st = 0;
                        }
                    }
                }
            } catch (...) {  // std::bad_alloc on a file too large to hold
                st = -1;
            }
            kind[(size_t)i] = st == 0 ? ct : -1;
            h_status[f0 + i] = st;
        });
        // one upload, one launch per run of files of one colour type; failed files: zeros
        uint8_t* dev = (uint8_t*)ctx->loader_slot[k].dev.p;
        MRG_HIP_CHECK(hipMemcpyAsync(dev, h_scan, (size_t)n * area, hipMemcpyHostToDevice, s));
        for (int i = 0; i < n;) {
            int e = i + 1;
            while (e < n && kind[(size_t)e] == kind[(size_t)i]) ++e;
            uint8_t* o = out + (size_t)(f0 + i) * frame_pitch * es;
            if (kind[(size_t)i] == 3) {
                for (int q = i; q < e; ++q)
                    MRG_HIP_CHECK(hipMemcpy2DAsync(out + (size_t)(f0 + q) * frame_pitch * es, (size_t)stride, dev + (size_t)q * area, (size_t)width,
                                                   (size_t)width, (size_t)height, hipMemcpyDeviceToDevice, s));
            } else if (kind[(size_t)i] >= 0) {
                int rc;
                if ((rc = launch_png_recon(ctx, dev + (size_t)i * area, (int64_t)area, e - i, width, height, bits, kind[(size_t)i], o, frame_pitch, stride, s)))
                    return rc;
            } else {
                for (int q = i; q < e; ++q) MRG_HIP_CHECK(zero_frame(d_out, f0 + q, frame_pitch, stride, width, height, es, s));
            }
            i = e;
        }
        return 0;
    };
    // the chunk slots are shared with the other loaders (ctx.h: loader_slot)
    return loader_ring(ctx, nfiles, chunk, (size_t)chunk * area, (size_t)chunk * area, stage, nullptr, nullptr);
}

}  // extern "C"
