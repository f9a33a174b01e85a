// Baseline JPEG on the device: the inverse DCT of the luma blocks a host thread has entropy-decoded (jpeg.cpp), and the
// batch loader that keeps host threads, the upload and the kernel busy side by side.  See include/mrgingham_amd.h for the
// contract of the three entry points and DESIGN.md section 4.10 for the layout and what bounds the kernel.
#include <string.h>

#include <algorithm>

#include "ctx.h"
#include "image_io.h"
#include "jpeg.h"
#include "jpeg_idct8.h"
#include "loader.h"

using namespace mrg;

namespace {

constexpr int kBlocksPerGroup = 32;  // blocks of one block row a workgroup of 256 lanes takes: 8 lanes per block
// dwords between the transpose tiles of neighbouring blocks in LDS: 64 + 8, so that the column accesses (dword
// [j][k] of lane k, ds_read_b32 / ds_write_b32: 32 banks, conflicts within a 32-lane half) of the four blocks of a half
// fall on 4 x 8 different banks
constexpr int kTilePitch = 72;

// Eight lanes take one block.  Lane r loads row r of the quantised coefficients (16 bytes: a wave reads 1 KiB in one
// piece) and dequantises it; the eight lanes transpose the block through LDS so that lane k holds column k for pass 1,
// transpose the result back the same way (each lane overwrites exactly the dwords it has just read: no barrier in
// between), and lane r runs pass 2 on row r and stores its 8 pixels as one 8-byte word -- the eight blocks of a wave
// lie side by side, so a wave writes 64-byte runs.  Blocks cut by `width`, or rows that are not 8-byte aligned, are
// stored byte by byte.  The products c * q are taken in 32 bits like every other product here; where the compiler
// picks the 24-bit multiplier for them it is exact, because c (int16) and q (uint16) both fit 24 signed bits and
// |c * q| < 2^31.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, long long coef_pitch,
                                                        const uint16_t* __restrict__ quant, int frame0, int width, int height,
                                                        int blocks_w, uint8_t* __restrict__ out, long long frame_pitch,
                                                        int stride) {
    __shared__ __attribute__((aligned(16))) uint16_t sq[64];
    __shared__ __attribute__((aligned(16))) uint32_t tile[kBlocksPerGroup * kTilePitch];
    const int t = threadIdx.x, r = t & 7, blk = t >> 3;
    const int f = frame0 + blockIdx.z, by = blockIdx.y;
    const int bx = blockIdx.x * kBlocksPerGroup + blk;
    if (t < 64) sq[t] = quant[(long long)f * 64 + t];
    // (the grid covers ceil(height / 8) block rows: padding rows of blocks are never read)
    const bool live = bx < blocks_w && bx * 8 < width;
    uint4 raw = make_uint4(0, 0, 0, 0);
    if (live) raw = *(const uint4*)(coef + (long long)f * coef_pitch + ((long long)by * blocks_w + bx) * 64 + r * 8);
    __syncthreads();
    const uint4 qraw = *(const uint4*)(sq + r * 8);
    const uint32_t cw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[4] = {qraw.x, qraw.y, qraw.z, qraw.w};
    uint32_t d[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        d[2 * i] = (uint32_t)(int32_t)(int16_t)(cw[i] & 0xFFFFu) * (qw[i] & 0xFFFFu);
        d[2 * i + 1] = (uint32_t)((int32_t)cw[i] >> 16) * (qw[i] >> 16);
    }
    uint32_t* mine = tile + blk * kTilePitch;
    *(uint4*)(mine + r * 8) = make_uint4(d[0], d[1], d[2], d[3]);
    *(uint4*)(mine + r * 8 + 4) = make_uint4(d[4], d[5], d[6], d[7]);
    __syncthreads();
    int32_t o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = mine[j * 8 + r];  // lane r is column r now
    jpeg_idct8<11>(d, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) mine[j * 8 + r] = (uint32_t)o[j];
    __syncthreads();
    const uint4 lo = *(const uint4*)(mine + r * 8), hi = *(const uint4*)(mine + r * 8 + 4);
    d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w;
    d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
    jpeg_idct8<18>(d, o);
    const int y = by * 8 + r;
    if (!live || y >= height) return;
    uint32_t px[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int32_t v = o[k] + 128;
        px[k] = (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
    uint8_t* p = out + (long long)f * frame_pitch + (long long)y * stride + bx * 8;
    const int nx = width - bx * 8;
    if (nx >= 8 && ((uintptr_t)p & 7) == 0) {
        *(uint2*)p = make_uint2(px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24),
                                px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24));
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < nx) p[k] = (uint8_t)px[k];
    }
}

int check_idct_args(mrgingham_amd_ctx* ctx, const int16_t* d_coef, int64_t coef_pitch, const uint16_t* d_quant, int nframes,
                    int width, int height, int blocks_w, int blocks_h, const uint8_t* d_out, int64_t frame_pitch, int stride) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (nframes < 0 || width < 0 || height < 0 || blocks_w < 0 || blocks_h < 0 || stride < width || frame_pitch < 0 || coef_pitch < 0 ||
        (nframes > 0 && (!d_coef || !d_quant || !d_out)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad JPEG coefficient batch descriptor");
    return check_coef_area(ctx, d_coef, coef_pitch, width, height, blocks_w, blocks_h);
}

}  // namespace

namespace mrg {

int check_coef_area(mrgingham_amd_ctx* ctx, const int16_t* d_coef, int64_t coef_pitch, int width, int height, int blocks_w, int blocks_h) {
    if (width > 32767 || height > 32767)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "frames larger than 32767 pixels per side are not supported");
    // (an MCU is at most 32 pixels wide and high: 4100 blocks cover the padding of the largest frame)
    if (blocks_w > 4100 || blocks_h > 4100 || (long long)blocks_w * 8 < width || (long long)blocks_h * 8 < height)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "blocks_w x blocks_h does not cover width x height");
    if (coef_pitch < (int64_t)blocks_w * blocks_h * 64 || (coef_pitch & 7) || ((uintptr_t)d_coef & 15))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "coefficients: 16-byte aligned, coef_pitch a multiple of 8 and at least blocks_w*blocks_h*64");
    return 0;
}

void launch_jpeg_idct(const int16_t* d_coef, int64_t coef_pitch, const uint16_t* d_quant, int nframes, int width, int height,
                      int blocks_w, uint8_t* d_out, int64_t frame_pitch, int stride, hipStream_t s) {
    const int bw = (width + 7) / 8, bh = (height + 7) / 8;
    for_frame_slabs(nframes, [&](int f0, unsigned n) {
        const dim3 grid((unsigned)((bw + kBlocksPerGroup - 1) / kBlocksPerGroup), (unsigned)bh, n);
        hipLaunchKernelGGL(jpeg_idct_kernel, grid, dim3(256), 0, s, d_coef, (long long)coef_pitch, d_quant, f0, width, height,
                           blocks_w, d_out, (long long)frame_pitch, stride);
    });
}

}  // namespace mrg

extern "C" {

int mrgingham_amd_jpeg_coefficients(const uint8_t* data, size_t nbytes, int16_t* coef, size_t coef_capacity, uint16_t* quant,
                                    int* width, int* height, int* blocks_w, int* blocks_h) {
    if (!data) return -1;
    JpegInfo info;
    int rc = jpeg_coefficients(data, nbytes, nullptr, 0, 0, &info);
    if (rc) return -1;
    if (width) *width = info.width;
    if (height) *height = info.height;
    if (blocks_w) *blocks_w = info.blocks_w;
    if (blocks_h) *blocks_h = info.blocks_h;
    if (quant) memcpy(quant, info.quant, sizeof(info.quant));
    if (!coef) return 0;
    rc = jpeg_coefficients(data, nbytes, coef, coef_capacity, 0, &info);
    return rc;
}

int mrgingham_amd_jpeg_idct_batch(mrgingham_amd_ctx* ctx, const int16_t* d_coef, int64_t coef_pitch, const uint16_t* d_quant,
                                  int nframes, int width, int height, int blocks_w, int blocks_h, uint8_t* d_out,
                                  int64_t frame_pitch, int stride, void* stream) {
    const int rc = check_idct_args(ctx, d_coef, coef_pitch, d_quant, nframes, width, height, blocks_w, blocks_h, d_out, frame_pitch, stride);
    if (rc) return rc;
    if (nframes == 0 || width == 0 || height == 0) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    launch_jpeg_idct(d_coef, coef_pitch, d_quant, nframes, width, height, blocks_w, d_out, frame_pitch, stride,
                     (hipStream_t)stream);  // (the stream used as given: NULL is HIP's default stream)
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

int mrgingham_amd_read_jpegs_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height,
                                   uint8_t* d_out, int64_t frame_pitch, int stride, int nthreads, int32_t* h_status) {
    int rc = check_file_batch(ctx, "JPEG", filenames, nfiles, width, height, 1, d_out, frame_pitch, stride, h_status);
    if (rc) return rc;
    if (nfiles == 0) return 0;
    fb_drain(ctx);
    const CallerDevice caller_device_;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    nthreads = host_threads(nthreads);

    // every file of the batch is decoded into ONE block geometry, the largest any sampling gives this size (luma factors
    // 1 .. 4: MCUs of 8 .. 32 pixels), so that a chunk is one kernel launch; the blocks a file does not have lie outside
    // width x height and are never read
    auto padded = [](int side) {
        int most = 0;
        for (int h = 1; h <= 4; ++h) most = std::max(most, (side + 8 * h - 1) / (8 * h) * h);
        return most;
    };
    const int bw = padded(width), bh = padded(height);
    const size_t per_frame = (size_t)bw * bh * 64;  // elements
    const int chunk = loader_chunk_frames(ctx->jpeg_coef_budget, per_frame * sizeof(int16_t), nfiles, nthreads, ctx->jpeg_chunk_frames);
    if (ctx->jpeg_entropy)  // files with restart intervals are Huffman-decoded on the device (jpeg_huff.hip)
        return read_jpegs_device_entropy(ctx, filenames, nfiles, width, height, d_out, frame_pitch, stride, nthreads, h_status, bw, bh, chunk);
    const size_t coef_bytes = (size_t)chunk * per_frame * sizeof(int16_t), slot_bytes = coef_bytes + (size_t)chunk * 64 * sizeof(uint16_t);
    hipStream_t s = ctx->pix;
    auto stage = [&](int k, int f0, int n) -> int {
        int16_t* h_coef = (int16_t*)ctx->loader_slot[k].pin.p;
        uint16_t* h_quant = (uint16_t*)((char*)h_coef + coef_bytes);
        for_files<std::vector<uint8_t>>(ctx->pool, nthreads, n, [&](int i, std::vector<uint8_t>& file) {
            int32_t st = -1;
            JpegInfo info;
            try {
                if (read_file(filenames[f0 + i], file) && jpeg_coefficients(file.data(), file.size(), nullptr, 0, 0, &info) == 0) {
                    if (info.width != width || info.height != height) st = -2;
                    else if (jpeg_coefficients(file.data(), file.size(), h_coef + (size_t)i * per_frame, per_frame, bw, &info) == 0) st = 0;
                }
            } catch (...) {  // std::bad_alloc on a file too large to hold
                st = -1;
            }
            if (st == 0) memcpy(h_quant + (size_t)i * 64, info.quant, sizeof(info.quant));
            h_status[f0 + i] = st;
        });
        // one upload (coefficients | tables, laid out alike on both sides), one launch
        char* dev = (char*)ctx->loader_slot[k].dev.p;
        if (n == chunk) {
            MRG_HIP_CHECK(hipMemcpyAsync(dev, h_coef, slot_bytes, hipMemcpyHostToDevice, s));
        } else {  // the last, shorter chunk: not the unused coefficient slots in between
            MRG_HIP_CHECK(hipMemcpyAsync(dev, h_coef, (size_t)n * per_frame * sizeof(int16_t), hipMemcpyHostToDevice, s));
            MRG_HIP_CHECK(hipMemcpyAsync(dev + coef_bytes, h_quant, (size_t)n * 64 * sizeof(uint16_t), hipMemcpyHostToDevice, s));
        }
        launch_jpeg_idct((const int16_t*)dev, (int64_t)per_frame, (const uint16_t*)(dev + coef_bytes), n, width, height, bw,
                         d_out + (size_t)f0 * frame_pitch, frame_pitch, stride, s);
        MRG_HIP_CHECK(hipGetLastError());
        return 0;
    };
    return loader_ring(ctx, nfiles, chunk, slot_bytes, slot_bytes, stage,
                       zero_failed_frames(ctx, d_out, frame_pitch, stride, width, height, 1, h_status), nullptr);  // failed files: zeros afterwards
}

}  // extern "C"
