// Windows Bitmap on the device: the pixel array of a file as it lies on disk -- rows bottom-up or top-down, padded to four
// bytes, palette indices of 1, 4 or 8 bits or B G R (X) samples -- to uint8 grey frames with a row stride, and the batch
// loader that reads the pixel arrays straight into page-locked staging.  The pixels themselves are bmp_pixels.h, the text
// the host decoder runs.  See include/mrgingham_amd.h for the contract of the entry points and DESIGN.md section 4.18 for
// the byte model and the numbers.
#include <stdio.h>
#include <string.h>

#include "bmp_pixels.h"
#include "ctx.h"
#include "image_io.h"
#include "loader.h"

using namespace mrg;

namespace {

constexpr int kLanes = 256;
constexpr int kWorkgroupsPerCu = 8;  // eight workgroups of 256 lanes fill a CU

// A grid-stride loop over the rows of all frames; a row is taken by 2^lpr_shift lanes of a workgroup (256 >> lpr_shift
// rows side by side), lane l by the words l, l + lanes, ... of the DESTINATION row: consecutive lanes store consecutive
// 16-byte words.  Word k of a row whose destination begins `ph` bytes behind a 16-byte boundary holds the pixels
// [16k - ph, 16k - ph + 16) that lie inside the row; a whole word is one 16-byte store (its address is a multiple of 16 by
// construction), the head and the tail of a row go out sample by sample.
template <int BITS, bool LUT>
__global__ __launch_bounds__(kLanes) void bmp_unpack_kernel(const uint8_t* __restrict__ payload, long long payload_pitch,
                                                            const uint8_t* __restrict__ lut, int rowb, int width, int height,
                                                            long long nrows, int top_down, uint8_t* __restrict__ out,
                                                            long long frame_pitch, long long stride, int lpr_shift) {
    const int lanes = 1 << lpr_shift, l = (int)threadIdx.x & (lanes - 1), sub = (int)threadIdx.x >> lpr_shift;
    const long long rows_per_step = (long long)gridDim.x * (kLanes >> lpr_shift);
    for (long long row = (long long)blockIdx.x * (kLanes >> lpr_shift) + sub; row < nrows; row += rows_per_step) {
        const long long f = row / height;
        const int y = (int)(row - f * height);
        const uint8_t* src = payload + f * payload_pitch + (long long)(top_down ? y : height - 1 - y) * rowb;
        const uint8_t* table = LUT ? lut + 256 * f : nullptr;
        uint8_t* dst = out + f * frame_pitch + (long long)y * stride;
        const int ph = (int)((uintptr_t)dst & 15);
        const int K = (ph + width + 15) >> 4;
        for (int k = l; k < K; k += lanes) {
            int x0 = 16 * k - ph, hi = x0 + 16;
            if (x0 < 0) x0 = 0;
            if (hi > width) hi = width;
            const int n = hi - x0;
            uint32_t d[4];
            bmp_pixels<BITS, LUT>(src, rowb, table, x0, n, d);
            uint8_t* o = dst + x0;
            if (n == 16) {
                *(uint4*)o = make_uint4(d[0], d[1], d[2], d[3]);
            } else {
#pragma unroll
                for (int p = 0; p < 15; ++p)
                    if (p < n) o[p] = (uint8_t)(d[p >> 2] >> (8 * (p & 3)));
            }
        }
    }
}

// checked arguments -> the launch
int launch_bmp_unpack(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, const uint8_t* d_lut, int nframes, int width,
                      int height, int bits, int top_down, int lut_identity, uint8_t* d_out, int64_t frame_pitch, int stride, hipStream_t s) {
    const int rowb = (int)((((long long)width * bits + 31) / 32) * 4);
    const long long nrows = (long long)nframes * height;
    // the lanes of a row: the power of two that covers its words (one more than width / 16 where a row can begin inside a word)
    const bool aligned = !((uintptr_t)d_out & 15) && !(frame_pitch & 15) && !(stride & 15);
    const int kmax = (width + 15) / 16 + (aligned ? 0 : 1);
    int lpr_shift = 0;
    while ((1 << lpr_shift) < kmax && (1 << lpr_shift) < kLanes) ++lpr_shift;
    const int rows_per_block = kLanes >> lpr_shift;
    int cus = 0;
    MRG_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    long long blocks = (nrows + rows_per_block - 1) / rows_per_block;  // sized to the device
    if (blocks > (long long)cus * kWorkgroupsPerCu) blocks = (long long)cus * kWorkgroupsPerCu;
#define MRG_BMP_LAUNCH(B, L)                                                                                                         \
    hipLaunchKernelGGL((bmp_unpack_kernel<B, L>), dim3((unsigned)blocks), dim3(kLanes), 0, s, d_payload, (long long)payload_pitch, d_lut, \
                       rowb, width, height, nrows, top_down ? 1 : 0, d_out, (long long)frame_pitch, (long long)stride, lpr_shift)
    switch (bits) {
        case 1: MRG_BMP_LAUNCH(1, true); break;
        case 4: MRG_BMP_LAUNCH(4, true); break;
        case 8:
            if (lut_identity) MRG_BMP_LAUNCH(8, false);
            else MRG_BMP_LAUNCH(8, true);
            break;
        case 24: MRG_BMP_LAUNCH(24, false); break;
        default: MRG_BMP_LAUNCH(32, false); break;
    }
#undef MRG_BMP_LAUNCH
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

// what a host thread of the loader keeps from file to file
struct BmpThread {
    std::vector<uint8_t> head;
    Image im;
};

constexpr size_t kHeadBytes = 4096;  // (what probe_image reads first: the headers, the masks and the palette lie inside)

// the file opened, its first bytes in `head`, its layout: the open file (the caller's to close) with *rc = bmp_layout's
// value, or NULL
FILE* open_bmp(const char* name, std::vector<uint8_t>& head, mrgingham_amd_bmp_info* bi, int* rc) {
    FILE* f = fopen(name, "rb");
    if (!f) return nullptr;
    long size = -1;
    if (fseek(f, 0, SEEK_END) == 0) size = ftell(f);
    if (size < 0 || fseek(f, 0, SEEK_SET) != 0) {
        fclose(f);
        return nullptr;
    }
    head.resize((size_t)size < kHeadBytes ? (size_t)size : kHeadBytes);
    if (fread(head.data(), 1, head.size(), f) != head.size()) {
        fclose(f);
        return nullptr;
    }
    *rc = bmp_layout(head.data(), head.size(), (size_t)size, bi);
    return f;
}

// how a file of the list reaches its frame
struct BmpFile {
    int8_t route = 0;  // 0 failed (h_status says how), 1 its pixel array through the kernel, 2 decoded by a host thread
    int8_t bits = 0, top_down = 0, lut_identity = 0;
    int32_t row_bytes = 0;
    bool same_launch(const BmpFile& o) const {
        return route == 1 && o.route == 1 && bits == o.bits && top_down == o.top_down && lut_identity == o.lut_identity;
    }
};

}  // namespace

extern "C" {

void mrgingham_amd_bmp_unpack_geometry(int* lanes_per_workgroup, int* max_workgroups_per_cu) {
    if (lanes_per_workgroup) *lanes_per_workgroup = kLanes;
    if (max_workgroups_per_cu) *max_workgroups_per_cu = kWorkgroupsPerCu;
}

int mrgingham_amd_bmp_unpack_batch(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, const uint8_t* d_lut, int nframes,
                                   int width, int height, int bits, int top_down, int lut_identity, uint8_t* d_out, int64_t frame_pitch,
                                   int stride, void* stream) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (nframes < 0 || width < 0 || height < 0 || stride < width || frame_pitch < 0 || payload_pitch < 0 || (nframes > 0 && (!d_payload || !d_out)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad BMP payload batch descriptor");
    if (width > 32767 || height > 32767)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "frames larger than 32767 pixels per side are not supported");
    if (bits != 1 && bits != 4 && bits != 8 && bits != 24 && bits != 32) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "BMP payloads: 1, 4, 8, 24 or 32 bits");
    const int64_t rowb = (((int64_t)width * bits + 31) / 32) * 4;
    if ((payload_pitch & 15) || payload_pitch < rowb * height || ((uintptr_t)d_payload & 15))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "BMP payloads: 16-byte aligned, payload_pitch a multiple of 16 and at least row_bytes*height");
    if (nframes > 0 && !d_lut && bits <= 8 && !(bits == 8 && lut_identity))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "BMP payloads: palette depths need their grey tables");
    if (nframes == 0 || width == 0 || height == 0) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    return launch_bmp_unpack(ctx, d_payload, payload_pitch, d_lut, nframes, width, height, bits, top_down, lut_identity, d_out, frame_pitch, stride,
                             (hipStream_t)stream);  // (the stream used as given: NULL is HIP's default stream)
}

int mrgingham_amd_read_bmps_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height, uint8_t* d_out,
                                  int64_t frame_pitch, int stride, int nthreads, int32_t* h_status) {
    int rc = check_file_batch(ctx, "BMP", filenames, nfiles, width, height, 1, d_out, frame_pitch, stride, h_status);
    if (rc) return rc;
    if (nfiles == 0) return 0;
    fb_drain(ctx);
    const CallerDevice caller_device_;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    nthreads = host_threads(nthreads);
    hipStream_t s = ctx->pix;
    const bool unpack = ctx->bmp_unpack != 0;
    const size_t npx = (size_t)width * height;

    // the headers first: what every file is, and with that the one size of the staging areas
    std::vector<BmpFile> file((size_t)nfiles);
    try {
        for_files<BmpThread>(ctx->pool, nthreads, nfiles, [&](int i, BmpThread& t) {
            int32_t st = -1;
            try {
                mrgingham_amd_bmp_info bi;
                int head = -1;
                if (FILE* f = open_bmp(filenames[i], t.head, &bi, &head)) {
                    fclose(f);
                    if (head == 0 || head == kBmpNotTaken) {
                        if (bi.width != width || bi.height != height) st = -2;
                        else {
                            st = 0;
                            BmpFile& b = file[(size_t)i];
                            b.route = unpack && head == 0 ? 1 : 2;
                            b.bits = (int8_t)bi.bits; b.top_down = (int8_t)bi.top_down; b.lut_identity = (int8_t)bi.lut_identity;
                            b.row_bytes = bi.row_bytes;
                        }
                    }
                }
            } catch (...) {  // std::bad_alloc
                st = -1;
            }
            h_status[i] = st;
        });
    } catch (...) {
        return fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "out of host memory");
    }
    // every file of a chunk gets one area of the staging, a multiple of 16 bytes: its pixel array lies there as in the
    // file (a host-decoded file: its grey samples, dense); the grey tables of the chunk lie in front, 256 bytes each
    size_t area = 16;
    for (const BmpFile& b : file) {
        const size_t need = b.route == 1 ? (size_t)b.row_bytes * height : b.route == 2 ? npx : 0;
        if (((need + 15) & ~(size_t)15) > area) area = (need + 15) & ~(size_t)15;
    }
    const int chunk = loader_chunk_frames(ctx->jpeg_coef_budget, area + 256, nfiles, nthreads, ctx->bmp_chunk_frames);
    const size_t lut_bytes = (size_t)chunk * 256;
    auto stage = [&](int k, int f0, int n) -> int {
        uint8_t* h_lut = (uint8_t*)ctx->loader_slot[k].pin.p;
        uint8_t* h_pay = h_lut + lut_bytes;
        for_files<BmpThread>(ctx->pool, nthreads, n, [&](int i, BmpThread& t) {
            const BmpFile& b = file[(size_t)(f0 + i)];
            if (b.route == 0) return;
            bool ok = false;
            uint8_t* dst = h_pay + (size_t)i * area;
            try {
                if (b.route == 2) {
                    ok = read_image(filenames[f0 + i], t.im) && t.im.depth == 8 && t.im.w == width && t.im.h == height;
                    if (ok) memcpy(dst, t.im.px8.data(), npx);
                } else {
                    mrgingham_amd_bmp_info bi;
                    int head = -1;
                    if (FILE* f = open_bmp(filenames[f0 + i], t.head, &bi, &head)) {
                        // (the file the first pass saw)
                        if (head == 0 && bi.width == width && bi.height == height && bi.bits == b.bits && bi.top_down == b.top_down &&
                            bi.lut_identity == b.lut_identity) {
                            memcpy(h_lut + 256 * (size_t)i, bi.lut, 256);
                            // the pixels behind the headers, then the rest of the array straight from the file
                            const size_t need = (size_t)bi.row_bytes * height, off = (size_t)bi.payload_offset;
                            size_t have = 0;
                            if (off < t.head.size()) {
                                have = t.head.size() - off < need ? t.head.size() - off : need;
                                memcpy(dst, t.head.data() + off, have);
                            }
                            ok = have == need || (fseek(f, (long)(off + have), SEEK_SET) == 0 && fread(dst + have, 1, need - have, f) == need - have);
                        }
                        fclose(f);
                    }
                }
            } catch (...) {  // std::bad_alloc
                ok = false;
            }
            if (!ok) h_status[f0 + i] = -1;
        });
        uint8_t* d_lut = (uint8_t*)ctx->loader_slot[k].dev.p;
        uint8_t* d_pay = d_lut + lut_bytes;
        MRG_HIP_CHECK(hipMemcpyAsync(d_lut, h_lut, lut_bytes + (size_t)n * area, hipMemcpyHostToDevice, s));
        // one launch per run of files with equal depth, row order and kind of table
        for (int i = 0; i < n;) {
            const BmpFile& b = file[(size_t)(f0 + i)];
            uint8_t* frame = d_out + (size_t)(f0 + i) * (size_t)frame_pitch;
            if (h_status[f0 + i] != 0) { ++i; continue; }  // (zeroed behind the launches)
            if (b.route == 2) {
                MRG_HIP_CHECK(hipMemcpy2DAsync(frame, (size_t)stride, d_pay + (size_t)i * area, (size_t)width, (size_t)width, (size_t)height,
                                               hipMemcpyDeviceToDevice, s));
                ++i;
                continue;
            }
            int e = i + 1;
            while (e < n && h_status[f0 + e] == 0 && b.same_launch(file[(size_t)(f0 + e)])) ++e;
            const int lrc = launch_bmp_unpack(ctx, d_pay + (size_t)i * area, (int64_t)area, d_lut + 256 * (size_t)i, e - i, width, height, b.bits,
                                              b.top_down, b.lut_identity, frame, frame_pitch, stride, s);
            if (lrc) return lrc;
            i = e;
        }
        return 0;
    };
    // the chunk slots are shared with the other loaders (ctx.h: loader_slot)
    const size_t slot_bytes = lut_bytes + (size_t)chunk * area;
    return loader_ring(ctx, nfiles, chunk, slot_bytes, slot_bytes, stage, zero_failed_frames(ctx, d_out, frame_pitch, stride, width, height, h_status),
                       nullptr);
}

}  // extern "C"
