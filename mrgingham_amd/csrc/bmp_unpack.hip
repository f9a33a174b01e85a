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
#include "unpack_rows.h"

using namespace mrg;

namespace {

// a row of the pixel array, bottom-up unless top_down, with the frame's grey table
template <int BITS, bool LUT>
struct BmpRows {
    const uint8_t* __restrict__ payload;
    long long payload_pitch;
    const uint8_t* __restrict__ lut;
    int rowb, height, top_down;
    struct Row {
        const uint8_t* __restrict__ src;
        const uint8_t* __restrict__ table;
        int rowb;
        __device__ __forceinline__ void pixels(int x0, int n, uint32_t d[4]) const { bmp_pixels<BITS, LUT>(src, rowb, table, x0, n, d); }
    };
    __device__ __forceinline__ Row row(long long f, int y) const {
        return Row{payload + f * payload_pitch + (long long)(top_down ? y : height - 1 - y) * rowb, LUT ? lut + 256 * f : nullptr, rowb};
    }
};

// unpack_rows.h has the schedule
template <int BITS, bool LUT>
__global__ __launch_bounds__(kUnpackLanes) void bmp_unpack_kernel(const uint8_t* __restrict__ payload, long long payload_pitch,
                                                                  const uint8_t* __restrict__ lut, int rowb, int width, int height,
                                                                  long long nrows, int top_down, uint8_t* __restrict__ out,
                                                                  long long frame_pitch, long long stride, int lpr_shift) {
    unpack_rows<1>(BmpRows<BITS, LUT>{payload, payload_pitch, lut, rowb, height, top_down}, width, height, nrows, out, frame_pitch, stride,
                   lpr_shift);
}

// checked arguments -> the launch
int launch_bmp_unpack(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, const uint8_t* d_lut, int nframes, int width,
                      int height, int bits, int top_down, int lut_identity, uint8_t* d_out, int64_t frame_pitch, int stride, hipStream_t s) {
    const int rowb = (int)((((long long)width * bits + 31) / 32) * 4);
    const long long nrows = (long long)nframes * height;
    UnpackShape sh;
    if (int rc = unpack_launch_shape(ctx, d_out, frame_pitch, stride, width, nrows, &sh)) return rc;
#define MRG_BMP_LAUNCH(B, L)                                                                                                                  \
    hipLaunchKernelGGL((bmp_unpack_kernel<B, L>), dim3((unsigned)sh.blocks), dim3(kUnpackLanes), 0, s, d_payload, (long long)payload_pitch,    \
                       d_lut, rowb, width, height, nrows, top_down ? 1 : 0, d_out, (long long)frame_pitch, (long long)stride, sh.lpr_shift)
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

// what the launch of a file that goes through the kernel depends on
struct BmpFile {
    int8_t bits = 0, top_down = 0, lut_identity = 0;
    bool same_launch(const BmpFile& o) const { return bits == o.bits && top_down == o.top_down && lut_identity == o.lut_identity; }
};

}  // namespace

extern "C" {

void mrgingham_amd_bmp_unpack_geometry(int* lanes_per_workgroup, int* max_workgroups_per_cu) {
    if (lanes_per_workgroup) *lanes_per_workgroup = kUnpackLanes;
    if (max_workgroups_per_cu) *max_workgroups_per_cu = kUnpackWorkgroupsPerCu;
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
    const bool unpack = ctx->bmp_unpack != 0;
    std::vector<BmpFile> file((size_t)nfiles);
    StagedFormat fmt;
    fmt.front = 256;  // the grey table
    fmt.chunk_cap = ctx->bmp_chunk_frames;
    fmt.header = [&](int i, StagedThread& t, int* route, size_t* raster_bytes) -> int32_t {
        mrgingham_amd_bmp_info bi;
        int head = -1;
        FILE* f = open_bmp(filenames[i], t.head, &bi, &head);
        if (!f) return -1;
        fclose(f);
        if (head != 0 && head != kBmpNotTaken) return -1;
        if (bi.width != width || bi.height != height) return -2;
        *route = unpack && head == 0 ? 1 : 2;
        *raster_bytes = (size_t)bi.row_bytes * height;
        file[(size_t)i] = BmpFile{(int8_t)bi.bits, (int8_t)bi.top_down, (int8_t)bi.lut_identity};
        return 0;
    };
    fmt.stage_raster = [&](int i, StagedThread& t, uint8_t* dst, uint8_t* lut) -> bool {
        const BmpFile& b = file[(size_t)i];
        mrgingham_amd_bmp_info bi;
        int head = -1;
        FILE* f = open_bmp(filenames[i], t.head, &bi, &head);
        if (!f) return false;
        bool ok = false;
        // (the file the first pass saw)
        if (head == 0 && bi.width == width && bi.height == height && bi.bits == b.bits && bi.top_down == b.top_down &&
            bi.lut_identity == b.lut_identity) {
            memcpy(lut, bi.lut, 256);
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
        return ok;
    };
    // one launch per run of files with equal depth, row order and kind of table
    fmt.same_launch = [&](int i, int j) { return file[(size_t)i].same_launch(file[(size_t)j]); };
    fmt.launch = [&](int i, int n, const uint8_t* d_pay, int64_t pitch, const uint8_t* d_lut, uint8_t* frame) {
        const BmpFile& b = file[(size_t)i];
        return launch_bmp_unpack(ctx, d_pay, pitch, d_lut, n, width, height, b.bits, b.top_down, b.lut_identity, frame, frame_pitch, stride, ctx->pix);
    };
    return read_staged_batch(ctx, filenames, nfiles, width, height, 8, d_out, frame_pitch, stride, nthreads, h_status, fmt);
}

}  // extern "C"
