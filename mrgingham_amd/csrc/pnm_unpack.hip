// Binary Netpbm on the device: the raster of a PBM, PGM or PAM file as it lies on disk -- packed bits, bytes or
// big-endian pairs, 1 .. 4 samples per pixel, rows without padding -- to uint8 / native uint16 grey frames with a row
// stride, and the batch loader that reads the rasters straight into page-locked staging.  The pixels themselves are
// pnm_pixels.h, the text the host decoder runs.  See include/mrgingham_amd.h for the contract of the entry points and
// DESIGN.md section 4.19 for the byte model and the numbers.
#include <stdio.h>
#include <string.h>

#include "ctx.h"
#include "image_io.h"
#include "loader.h"
#include "pnm_pixels.h"

using namespace mrg;

namespace {

constexpr int kLanes = 256;
constexpr int kWorkgroupsPerCu = 8;  // eight workgroups of 256 lanes fill a CU

// A grid-stride loop over the rows of all frames; a row is taken by 2^lpr_shift lanes of a workgroup (256 >> lpr_shift
// rows side by side), lane l by the words l, l + lanes, ... of the DESTINATION row: consecutive lanes store consecutive
// 16-byte words.  Word k of a row whose destination begins `ph` bytes behind a 16-byte boundary holds the samples of the
// pixels [(16k - ph) / ES, (16k - ph) / ES + 16 / ES) that lie inside the row (ES: bytes of a destination sample); a whole
// word is one 16-byte store (its address is a multiple of 16 by construction), the head and the tail of a row go out
// sample by sample.  The source row begins at byte y * rowb of the frame's payload, at any phase.
template <int BITS, int CH, bool BW>
__global__ __launch_bounds__(kLanes) void pnm_unpack_kernel(const uint8_t* __restrict__ payload, long long payload_pitch, int rowb, int width,
                                                            int height, long long nrows, uint8_t* __restrict__ out,
                                                            long long frame_pitch_b, long long stride_b, int lpr_shift) {
    constexpr int ES = BITS == 16 ? 2 : 1, NP = 16 / ES;
    const int lanes = 1 << lpr_shift, l = (int)threadIdx.x & (lanes - 1), sub = (int)threadIdx.x >> lpr_shift;
    const long long rows_per_step = (long long)gridDim.x * (kLanes >> lpr_shift);
    for (long long row = (long long)blockIdx.x * (kLanes >> lpr_shift) + sub; row < nrows; row += rows_per_step) {
        const long long f = row / height;
        const int y = (int)(row - f * height);
        const uint8_t* base = payload + f * payload_pitch;
        const long long row_off = (long long)y * rowb;
        uint8_t* dst = out + f * frame_pitch_b + (long long)y * stride_b;
        const int ph = (int)((uintptr_t)dst & 15);  // (even at 16 bits)
        const int K = (ph + width * ES + 15) >> 4;
        for (int k = l; k < K; k += lanes) {
            int x0 = (16 * k - ph) / ES, hi = x0 + NP;  // (16k - ph < 0 only with k == 0: x0 becomes 0 either way)
            if (x0 < 0) x0 = 0;
            if (hi > width) hi = width;
            const int n = hi - x0;
            uint32_t d[4];
            pnm_pixels<BITS, CH, BW>(base, payload_pitch, row_off, x0, n, d);
            uint8_t* o = dst + (long long)x0 * ES;
            if (n == NP) {
                *(uint4*)o = make_uint4(d[0], d[1], d[2], d[3]);
            } else if (ES == 2) {
#pragma unroll
                for (int p = 0; p < 7; ++p)
                    if (p < n) ((uint16_t*)o)[p] = (uint16_t)(d[p >> 1] >> (16 * (p & 1)));
            } else {
#pragma unroll
                for (int p = 0; p < 15; ++p)
                    if (p < n) o[p] = (uint8_t)(d[p >> 2] >> (8 * (p & 3)));
            }
        }
    }
}

int64_t pnm_row_bytes(int width, int bits, int channels) {
    return bits == 1 ? ((int64_t)width + 7) / 8 : (int64_t)width * channels * (bits / 8);
}

// checked arguments -> the launch (frame_pitch and stride in samples)
int launch_pnm_unpack(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, int nframes, int width, int height, int bits,
                      int channels, int bw, void* d_out, int64_t frame_pitch, int stride, hipStream_t s) {
    const int es = bits == 16 ? 2 : 1, rowb = (int)pnm_row_bytes(width, bits, channels);
    const long long nrows = (long long)nframes * height;
    // the lanes of a row: the power of two that covers its words (one more where a row can begin inside a word)
    const bool aligned = !((uintptr_t)d_out & 15) && !(((long long)frame_pitch * es) & 15) && !(((long long)stride * es) & 15);
    const int kmax = (width * es + 15) / 16 + (aligned ? 0 : 1);
    int lpr_shift = 0;
    while ((1 << lpr_shift) < kmax && (1 << lpr_shift) < kLanes) ++lpr_shift;
    const int rows_per_block = kLanes >> lpr_shift;
    int cus = 0;
    MRG_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    long long blocks = (nrows + rows_per_block - 1) / rows_per_block;  // sized to the device
    if (blocks > (long long)cus * kWorkgroupsPerCu) blocks = (long long)cus * kWorkgroupsPerCu;
#define MRG_PNM_LAUNCH(B, C, W)                                                                                                          \
    hipLaunchKernelGGL((pnm_unpack_kernel<B, C, W>), dim3((unsigned)blocks), dim3(kLanes), 0, s, d_payload, (long long)payload_pitch, rowb, \
                       width, height, nrows, (uint8_t*)d_out, (long long)frame_pitch * es, (long long)stride * es, lpr_shift)
    if (bits == 1) MRG_PNM_LAUNCH(1, 1, false);
    else if (bw) {
        if (channels == 1) MRG_PNM_LAUNCH(8, 1, true);
        else MRG_PNM_LAUNCH(8, 2, true);
    } else if (bits == 8) {
        switch (channels) {
            case 1: MRG_PNM_LAUNCH(8, 1, false); break;
            case 2: MRG_PNM_LAUNCH(8, 2, false); break;
            case 3: MRG_PNM_LAUNCH(8, 3, false); break;
            default: MRG_PNM_LAUNCH(8, 4, false); break;
        }
    } else {
        switch (channels) {
            case 1: MRG_PNM_LAUNCH(16, 1, false); break;
            case 2: MRG_PNM_LAUNCH(16, 2, false); break;
            case 3: MRG_PNM_LAUNCH(16, 3, false); break;
            default: MRG_PNM_LAUNCH(16, 4, false); break;
        }
    }
#undef MRG_PNM_LAUNCH
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

bool pnm_layout_ok(int bits, int channels, int bw) {
    if (bits == 1) return channels == 1 && !bw;
    if (bits != 8 && bits != 16) return false;
    if (channels < 1 || channels > 4) return false;
    return !bw || (bits == 8 && channels <= 2);
}

constexpr size_t kHeadBytes = 4096;  // (what probe_image reads first)

// the header out of the file's first bytes (a header with longer comments: out of twice as many, ...): pnm_header's value;
// *size receives the file's size
int read_pnm_header(FILE* f, std::vector<uint8_t>& head, mrgingham_amd_pnm_info* pi, size_t* size) {
    long sz = -1;
    if (fseek(f, 0, SEEK_END) == 0) sz = ftell(f);
    if (sz < 0 || fseek(f, 0, SEEK_SET) != 0) return -1;
    *size = (size_t)sz;
    int rc = kPgmHeaderCut;
    size_t got = 0;
    for (size_t want = kHeadBytes; rc == kPgmHeaderCut; want *= 2) {
        if (want > (size_t)sz) want = (size_t)sz;
        head.resize(want);
        got += fread(head.data() + got, 1, want - got, f);
        if (got != want) return -1;
        rc = pnm_header(head.data(), got, (size_t)sz, pi);
        if (want == (size_t)sz) break;  // the whole file
    }
    return rc;
}

// how a file of the list reaches its frame
struct PnmFile {
    int8_t route = 0;  // 0 failed (h_status says how), 1 its raster through the kernel, 2 decoded by a host thread
    int8_t bits = 0, channels = 0, bw = 0;
    int32_t row_bytes = 0;
    int64_t payload_offset = 0;
    bool same_launch(const PnmFile& o) const { return route == 1 && o.route == 1 && bits == o.bits && channels == o.channels && bw == o.bw; }
};

}  // namespace

extern "C" {

void mrgingham_amd_pnm_unpack_geometry(int* lanes_per_workgroup, int* max_workgroups_per_cu) {
    if (lanes_per_workgroup) *lanes_per_workgroup = kLanes;
    if (max_workgroups_per_cu) *max_workgroups_per_cu = kWorkgroupsPerCu;
}

int mrgingham_amd_pnm_unpack_batch(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, int nframes, int width, int height,
                                   int bits, int channels, int black_and_white, void* d_out, int64_t frame_pitch, int stride, void* stream) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (nframes < 0 || width < 0 || height < 0 || stride < width || frame_pitch < 0 || payload_pitch < 0 || (nframes > 0 && (!d_payload || !d_out)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad Netpbm payload batch descriptor");
    if (width > 32767 || height > 32767)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "frames larger than 32767 pixels per side are not supported");
    if (!pnm_layout_ok(bits, channels, black_and_white))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "Netpbm payloads: bits 1 (one channel), 8 or 16 with 1 .. 4 channels; black and white with 8 bits and 1 or 2 channels");
    if ((payload_pitch & 15) || payload_pitch < pnm_row_bytes(width, bits, channels) * height || ((uintptr_t)d_payload & 15) ||
        (bits == 16 && ((uintptr_t)d_out & 1)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "Netpbm payloads: 16-byte aligned, payload_pitch a multiple of 16 and at least row_bytes*height; 16-bit frames 2-byte aligned");
    if (nframes == 0 || width == 0 || height == 0) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    return launch_pnm_unpack(ctx, d_payload, payload_pitch, nframes, width, height, bits, channels, black_and_white ? 1 : 0, d_out, frame_pitch,
                             stride, (hipStream_t)stream);  // (the stream used as given: NULL is HIP's default stream)
}

int mrgingham_amd_read_pnms_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height, int bits, void* d_out,
                                  int64_t frame_pitch, int stride, int nthreads, int32_t* h_status) {
    const size_t es = bits == 8 ? 1 : bits == 16 ? 2 : 0;
    int rc = check_file_batch(ctx, "Netpbm", filenames, nfiles, width, height, es, d_out, frame_pitch, stride, h_status);
    if (rc) return rc;
    if (nfiles == 0) return 0;
    fb_drain(ctx);
    const CallerDevice caller_device_;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    nthreads = host_threads(nthreads);
    hipStream_t s = ctx->pix;
    const bool unpack = ctx->pnm_unpack != 0;
    const size_t npx = (size_t)width * height * es;  // bytes of a frame's samples

    // the headers first: what every file is, and with that the one size of the staging areas
    std::vector<PnmFile> file((size_t)nfiles);
    try {
        for_files<std::vector<uint8_t>>(ctx->pool, nthreads, nfiles, [&](int i, std::vector<uint8_t>& head) {
            int32_t st = -1;
            try {
                if (FILE* f = fopen(filenames[i], "rb")) {
                    mrgingham_amd_pnm_info pi;
                    size_t size = 0;
                    if (read_pnm_header(f, head, &pi, &size) == 0) {
                        // (P5: pnm_header leaves the payload to its caller)
                        if ((uint64_t)pi.row_bytes * (uint64_t)pi.height > size - (size_t)pi.payload_offset) st = -1;
                        else if (pi.width != width || pi.height != height || (pi.bits == 16 ? 16 : 8) != bits) st = -2;
                        else {
                            st = 0;
                            PnmFile& p = file[(size_t)i];
                            p.route = unpack ? 1 : 2;
                            p.bits = (int8_t)pi.bits; p.channels = (int8_t)pi.channels; p.bw = (int8_t)pi.black_and_white;
                            p.row_bytes = pi.row_bytes;
                            p.payload_offset = pi.payload_offset;
                        }
                    }
                    fclose(f);
                }
            } catch (...) {  // std::bad_alloc
                st = -1;
            }
            h_status[i] = st;
        });
    } catch (...) {
        return fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "out of host memory");
    }
    // every file of a chunk gets one area of the staging, a multiple of 16 bytes: its raster lies there as in the file (a
    // host-decoded file: its grey samples, dense)
    size_t area = 16;
    for (const PnmFile& p : file) {
        const size_t need = p.route == 1 ? (size_t)p.row_bytes * height : p.route == 2 ? npx : 0;
        if (((need + 15) & ~(size_t)15) > area) area = (need + 15) & ~(size_t)15;
    }
    const int chunk = loader_chunk_frames(ctx->jpeg_coef_budget, area, nfiles, nthreads, ctx->pnm_chunk_frames);
    auto stage = [&](int k, int f0, int n) -> int {
        uint8_t* h_pay = (uint8_t*)ctx->loader_slot[k].pin.p;
        for_files<Image>(ctx->pool, nthreads, n, [&](int i, Image& im) {
            const PnmFile& p = file[(size_t)(f0 + i)];
            if (p.route == 0) return;
            bool ok = false;
            uint8_t* dst = h_pay + (size_t)i * area;
            try {
                if (p.route == 2) {
                    ok = read_image(filenames[f0 + i], im) && im.depth == bits && im.w == width && im.h == height;
                    if (ok) memcpy(dst, bits == 8 ? (const void*)im.px8.data() : (const void*)im.px16.data(), npx);
                } else if (FILE* f = fopen(filenames[f0 + i], "rb")) {
                    // the raster straight from the file (a file that shrank since the first pass: unreadable)
                    const size_t need = (size_t)p.row_bytes * height;
                    ok = fseek(f, (long)p.payload_offset, SEEK_SET) == 0 && fread(dst, 1, need, f) == need;
                    fclose(f);
                }
            } catch (...) {  // std::bad_alloc
                ok = false;
            }
            if (!ok) h_status[f0 + i] = -1;
        });
        uint8_t* d_pay = (uint8_t*)ctx->loader_slot[k].dev.p;
        MRG_HIP_CHECK(hipMemcpyAsync(d_pay, h_pay, (size_t)n * area, hipMemcpyHostToDevice, s));
        // one launch per run of files with the same layout
        for (int i = 0; i < n;) {
            const PnmFile& p = file[(size_t)(f0 + i)];
            uint8_t* frame = (uint8_t*)d_out + (size_t)(f0 + i) * (size_t)frame_pitch * es;
            if (h_status[f0 + i] != 0) { ++i; continue; }  // (zeroed behind the launches)
            if (p.route == 2) {
                MRG_HIP_CHECK(hipMemcpy2DAsync(frame, (size_t)stride * es, d_pay + (size_t)i * area, (size_t)width * es, (size_t)width * es,
                                               (size_t)height, hipMemcpyDeviceToDevice, s));
                ++i;
                continue;
            }
            int e = i + 1;
            while (e < n && h_status[f0 + e] == 0 && p.same_launch(file[(size_t)(f0 + e)])) ++e;
            const int lrc = launch_pnm_unpack(ctx, d_pay + (size_t)i * area, (int64_t)area, e - i, width, height, p.bits, p.channels, p.bw, frame,
                                              frame_pitch, stride, s);
            if (lrc) return lrc;
            i = e;
        }
        return 0;
    };
    // a failed file's area holds whatever the slot held before: its frame is zeroed behind the launches
    auto after = [&](int, int f0, int n) -> int {
        for (int i = f0; i < f0 + n; ++i)
            if (h_status[i] != 0) MRG_HIP_CHECK(zero_frame(d_out, i, frame_pitch, stride, width, height, es, s));
        return 0;
    };
    // the chunk slots are shared with the other loaders (ctx.h: loader_slot)
    return loader_ring(ctx, nfiles, chunk, (size_t)chunk * area, (size_t)chunk * area, stage, after, nullptr);
}

}  // extern "C"
