// Binary Netpbm on the device: the raster of a PBM, PGM or PAM file as it lies on disk -- packed bits, bytes or
// big-endian pairs, 1 .. 4 samples per pixel, rows without padding -- to uint8 / native uint16 grey frames with a row
// stride, and the batch loader that reads the rasters straight into page-locked staging.  The pixels themselves are
// pnm_pixels.h, the text the host decoder runs.  See include/mrgingham_amd.h for the contract of the entry points and
// DESIGN.md section 4.19 for the byte model and the numbers.
#include <stdio.h>
#include <string.h>

#include "ctx.h"
#include "image_io.h"
#include "pnm_pixels.h"
#include "unpack_rows.h"

using namespace mrg;

namespace {

// a row of the raster: it begins at byte y * rowb of the frame's payload, at any phase
template <int BITS, int CH, bool BW>
struct PnmRows {
    const uint8_t* __restrict__ payload;
    long long payload_pitch;
    int rowb;
    struct Row {
        const uint8_t* __restrict__ base;
        long long limit, row_off;
        __device__ __forceinline__ void pixels(int x0, int n, uint32_t d[4]) const { pnm_pixels<BITS, CH, BW>(base, limit, row_off, x0, n, d); }
    };
    __device__ __forceinline__ Row row(long long f, int y) const { return Row{payload + f * payload_pitch, payload_pitch, (long long)y * rowb}; }
};

// unpack_rows.h has the schedule
template <int BITS, int CH, bool BW>
__global__ __launch_bounds__(kUnpackLanes) void pnm_unpack_kernel(const uint8_t* __restrict__ payload, long long payload_pitch, int rowb,
                                                                  int width, int height, long long nrows, uint8_t* __restrict__ out,
                                                                  long long frame_pitch_b, long long stride_b, int lpr_shift) {
    unpack_rows<BITS == 16 ? 2 : 1>(PnmRows<BITS, CH, BW>{payload, payload_pitch, rowb}, width, height, nrows, out, frame_pitch_b, stride_b,
                                    lpr_shift);
}

int64_t pnm_row_bytes(int width, int bits, int channels) {
    return bits == 1 ? ((int64_t)width + 7) / 8 : (int64_t)width * channels * (bits / 8);
}

// checked arguments -> the launch (frame_pitch and stride in samples)
int launch_pnm_unpack(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, int nframes, int width, int height, int bits,
                      int channels, int bw, void* d_out, int64_t frame_pitch, int stride, hipStream_t s) {
    const int es = bits == 16 ? 2 : 1, rowb = (int)pnm_row_bytes(width, bits, channels);
    const long long nrows = (long long)nframes * height;
    UnpackShape sh;
    if (int rc = unpack_launch_shape(ctx, d_out, (long long)frame_pitch * es, (long long)stride * es, (long long)width * es, nrows, &sh)) return rc;
#define MRG_PNM_LAUNCH(B, C, W)                                                                                                          \
    hipLaunchKernelGGL((pnm_unpack_kernel<B, C, W>), dim3((unsigned)sh.blocks), dim3(kUnpackLanes), 0, s, d_payload, (long long)payload_pitch, \
                       rowb, width, height, nrows, (uint8_t*)d_out, (long long)frame_pitch * es, (long long)stride * es, sh.lpr_shift)
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

// what the launch of a file that goes through the kernel depends on, and where its raster lies
struct PnmFile {
    int8_t bits = 0, channels = 0, bw = 0;
    int32_t row_bytes = 0;
    int64_t payload_offset = 0;
    bool same_launch(const PnmFile& o) const { return bits == o.bits && channels == o.channels && bw == o.bw; }
};

}  // namespace

extern "C" {

void mrgingham_amd_pnm_unpack_geometry(int* lanes_per_workgroup, int* max_workgroups_per_cu) {
    if (lanes_per_workgroup) *lanes_per_workgroup = kUnpackLanes;
    if (max_workgroups_per_cu) *max_workgroups_per_cu = kUnpackWorkgroupsPerCu;
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
    const bool unpack = ctx->pnm_unpack != 0;
    std::vector<PnmFile> file((size_t)nfiles);
    StagedFormat fmt;
    fmt.front = 0;
    fmt.chunk_cap = ctx->pnm_chunk_frames;
    fmt.header = [&](int i, StagedThread& t, int* route, size_t* raster_bytes) -> int32_t {
        FILE* f = fopen(filenames[i], "rb");
        if (!f) return -1;
        mrgingham_amd_pnm_info pi;
        size_t size = 0;
        int hrc = -1;
        try {
            hrc = read_pnm_header(f, t.head, &pi, &size);
        } catch (...) {  // std::bad_alloc
        }
        fclose(f);
        // (P5: pnm_header leaves the payload to its caller)
        if (hrc != 0 || (uint64_t)pi.row_bytes * (uint64_t)pi.height > size - (size_t)pi.payload_offset) return -1;
        if (pi.width != width || pi.height != height || (pi.bits == 16 ? 16 : 8) != bits) return -2;
        *route = unpack ? 1 : 2;
        *raster_bytes = (size_t)pi.row_bytes * height;
        file[(size_t)i] = PnmFile{(int8_t)pi.bits, (int8_t)pi.channels, (int8_t)pi.black_and_white, pi.row_bytes, pi.payload_offset};
        return 0;
    };
    fmt.stage_raster = [&](int i, StagedThread&, uint8_t* dst, uint8_t*) -> bool {
        FILE* f = fopen(filenames[i], "rb");
        if (!f) return false;
        // the raster straight from the file (a file that shrank since the first pass: unreadable)
        const PnmFile& p = file[(size_t)i];
        const size_t need = (size_t)p.row_bytes * height;
        const bool ok = fseek(f, (long)p.payload_offset, SEEK_SET) == 0 && fread(dst, 1, need, f) == need;
        fclose(f);
        return ok;
    };
    fmt.same_launch = [&](int i, int j) { return file[(size_t)i].same_launch(file[(size_t)j]); };
    fmt.launch = [&](int i, int n, const uint8_t* d_pay, int64_t pitch, const uint8_t*, uint8_t* frame) {
        const PnmFile& p = file[(size_t)i];
        return launch_pnm_unpack(ctx, d_pay, pitch, n, width, height, p.bits, p.channels, p.bw, frame, frame_pitch, stride, ctx->pix);
    };
    return read_staged_batch(ctx, filenames, nfiles, width, height, bits, d_out, frame_pitch, stride, nthreads, h_status, fmt);
}

}  // extern "C"
