// Binary PGM on the device: the payload of a file as it lies on disk -- bytes, or big-endian pairs -- to uint8 / native
// uint16 frames with a row stride, and the batch loader that reads the payloads straight into page-locked staging.  See
// include/mrgingham_amd.h for the contract of the entry points and DESIGN.md section 4.13 for the byte model and the numbers.
#include <stdio.h>
#include <string.h>

#include "ctx.h"
#include "image_io.h"
#include "loader.h"
#include "unpack_rows.h"

using namespace mrg;

namespace {

// What a lane holds of one 16-byte word of a destination row: bytes [lo, lo + n) of the row, n <= 16, in d from byte 0 on.
struct PgmGroup {
    uint32_t d[4];
    int lo, n;
};

// Word k of a row whose destination begins `ph` bytes behind a 16-byte boundary: the row bytes that fall into it, from the
// two aligned 16-byte words of the payload that cover them (the second only where a needed byte lies in it: nothing
// beyond the frame's pitch is read), shifted down by whole dwords with selects and by bytes with a funnel shift.
template <int BITS>
__device__ __forceinline__ PgmGroup pgm_load(const uint8_t* src, int rowb, int ph, int k) {
    PgmGroup g;
    g.lo = 16 * k - ph;
    int hi = g.lo + 16;
    if (g.lo < 0) g.lo = 0;
    if (hi > rowb) hi = rowb;
    g.n = hi - g.lo;
    const uint8_t* s = src + g.lo;
    const int sh = (int)((uintptr_t)s & 15);
    const uint4* a = (const uint4*)(s - sh);
    const uint4 A = a[0];
    uint4 B = make_uint4(0, 0, 0, 0);
    if (sh + g.n > 16) B = a[1];
    uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    if (sh & 8) {
#pragma unroll
        for (int i = 0; i < 6; ++i) w[i] = w[i + 2];
    }
    if (sh & 4) {
#pragma unroll
        for (int i = 0; i < 5; ++i) w[i] = w[i + 1];
    }
    const int r = 8 * (sh & 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t v = (uint32_t)(((((unsigned long long)w[i + 1]) << 32) | w[i]) >> r);
        // 16 bit: the two bytes of either half change places (one v_perm_b32: selector byte i names the source byte of byte i)
        g.d[i] = BITS == 16 ? __builtin_amdgcn_perm(v, v, 0x02030001u) : v;
    }
    return g;
}

// a whole word is one 16-byte store (its address is a multiple of 16 by construction); the head and the tail of a row go
// out sample by sample
template <int BITS>
__device__ __forceinline__ void pgm_store(uint8_t* dst, const PgmGroup& g) {
    uint8_t* o = dst + g.lo;
    if (g.n == 16) {
        *(uint4*)o = make_uint4(g.d[0], g.d[1], g.d[2], g.d[3]);
    } else if (BITS == 16) {
#pragma unroll
        for (int p = 0; p < 7; ++p)
            if (2 * p < g.n) ((uint16_t*)o)[p] = (uint16_t)(g.d[p >> 1] >> (16 * (p & 1)));
    } else {
#pragma unroll
        for (int p = 0; p < 15; ++p)
            if (p < g.n) o[p] = (uint8_t)(g.d[p >> 2] >> (8 * (p & 3)));
    }
}

// A grid-stride loop over the rows of all frames; a row is taken by 2^lpr_shift lanes of a workgroup (256 >> lpr_shift
// rows side by side), lane l by lane l's words l, l + lanes, ...: consecutive lanes store consecutive 16-byte words.  Two
// words per lane are in flight: both are loaded before either is stored.  No __restrict__: `out` may be the payload
// itself where the two layouts coincide; the words of source and destination are then the same, a lane stores exactly
// the samples it loaded, and the samples of a word that two rows share are stored by the lane that uses them.
template <int BITS>
__global__ __launch_bounds__(kUnpackLanes) void pgm_unpack_kernel(const uint8_t* payload, long long payload_pitch, int rowb, int height,
                                                            long long nrows, uint8_t* out, long long frame_pitch_b,
                                                            long long stride_b, int lpr_shift) {
    const int lanes = 1 << lpr_shift, l = (int)threadIdx.x & (lanes - 1), sub = (int)threadIdx.x >> lpr_shift;
    const long long rows_per_step = (long long)gridDim.x * (kUnpackLanes >> lpr_shift);
    for (long long row = (long long)blockIdx.x * (kUnpackLanes >> lpr_shift) + sub; row < nrows; row += rows_per_step) {
        const long long f = row / height;
        const int y = (int)(row - f * height);
        const uint8_t* src = payload + f * payload_pitch + (long long)y * rowb;
        uint8_t* dst = out + f * frame_pitch_b + (long long)y * stride_b;
        const int ph = (int)((uintptr_t)dst & 15);
        const int K = (ph + rowb + 15) >> 4;
        for (int k = l; k < K; k += 2 * lanes) {
            const bool two = k + lanes < K;
            const PgmGroup g0 = pgm_load<BITS>(src, rowb, ph, k);
            PgmGroup g1 = g0;
            if (two) g1 = pgm_load<BITS>(src, rowb, ph, k + lanes);
            pgm_store<BITS>(dst, g0);
            if (two) pgm_store<BITS>(dst, g1);
        }
    }
}

// checked arguments -> the launch
int launch_pgm_unpack(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, int nframes, int width, int height, int bits,
                      void* d_out, int64_t frame_pitch, int stride, hipStream_t s) {
    const int es = bits / 8, rowb = width * es;
    const long long nrows = (long long)nframes * height;
    UnpackShape sh;
    if (int rc = unpack_launch_shape(ctx, d_out, (long long)frame_pitch * es, (long long)stride * es, rowb, nrows, &sh)) return rc;
    if (bits == 8)
        hipLaunchKernelGGL(pgm_unpack_kernel<8>, dim3((unsigned)sh.blocks), dim3(kUnpackLanes), 0, s, d_payload, (long long)payload_pitch, rowb, height,
                           nrows, (uint8_t*)d_out, (long long)frame_pitch * es, (long long)stride * es, sh.lpr_shift);
    else
        hipLaunchKernelGGL(pgm_unpack_kernel<16>, dim3((unsigned)sh.blocks), dim3(kUnpackLanes), 0, s, d_payload, (long long)payload_pitch, rowb, height,
                           nrows, (uint8_t*)d_out, (long long)frame_pitch * es, (long long)stride * es, sh.lpr_shift);
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int mrgingham_amd_pgm_unpack_batch(mrgingham_amd_ctx* ctx, const uint8_t* d_payload, int64_t payload_pitch, int nframes, int width,
                                   int height, int bits, void* d_out, int64_t frame_pitch, int stride, void* stream) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (nframes < 0 || width < 0 || height < 0 || stride < width || frame_pitch < 0 || payload_pitch < 0 || (nframes > 0 && (!d_payload || !d_out)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad PGM payload batch descriptor");
    if (width > 32767 || height > 32767)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "frames larger than 32767 pixels per side are not supported");
    if (bits != 8 && bits != 16) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "PGM payloads: 8 or 16 bits");
    if ((payload_pitch & 15) || payload_pitch < (int64_t)width * height * (bits / 8) || ((uintptr_t)d_payload & 15) ||
        (bits == 16 && ((uintptr_t)d_out & 1)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "PGM payloads: 16-byte aligned, payload_pitch a multiple of 16 and at least width*height*bits/8; 16-bit frames 2-byte aligned");
    if (nframes == 0 || width == 0 || height == 0) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    return launch_pgm_unpack(ctx, d_payload, payload_pitch, nframes, width, height, bits, d_out, frame_pitch, stride,
                             (hipStream_t)stream);  // (the stream used as given: NULL is HIP's default stream)
}

int mrgingham_amd_read_pgms_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height, int bits,
                                  void* d_out, int64_t frame_pitch, int stride, int nthreads, int32_t* h_status) {
    const size_t es = bits == 8 ? 1 : bits == 16 ? 2 : 0;
    int rc = check_file_batch(ctx, "PGM", filenames, nfiles, width, height, es, d_out, frame_pitch, stride, h_status);
    if (rc) return rc;
    if (nfiles == 0) return 0;
    fb_drain(ctx);
    const CallerDevice caller_device_;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    nthreads = host_threads(nthreads);

    // every file of a chunk gets one area of the staging, a multiple of 16 bytes: its payload lies there as in the file
    const size_t need = (size_t)width * height * es, area = (need + 15) & ~(size_t)15;
    const int chunk = loader_chunk_frames(ctx->jpeg_coef_budget, area, nfiles, nthreads, ctx->pgm_chunk_frames);
    hipStream_t s = ctx->pix;
    constexpr size_t kHeadBytes = 4096;  // (what probe_image reads first)
    auto stage = [&](int k, int f0, int n) -> int {
        uint8_t* h_pay = (uint8_t*)ctx->loader_slot[k].pin.p;
        for_files<std::vector<uint8_t>>(ctx->pool, nthreads, n, [&](int i, std::vector<uint8_t>& head) {
            int32_t st = -1;
            FILE* f = fopen(filenames[f0 + i], "rb");
            if (f) {
                try {
                    // the header out of the file's first bytes (a header with longer comments: out of twice as many, ...)
                    int w = 0, h = 0, b = 0, hrc = kPgmHeaderCut;
                    size_t off = 0, got = 0;
                    for (size_t want = kHeadBytes; hrc == kPgmHeaderCut; want *= 2) {
                        head.resize(want);
                        got += fread(head.data() + got, 1, want - got, f);
                        hrc = pgm_header(head.data(), got, &w, &h, &b, &off);
                        if (got < want) break;  // the whole file
                    }
                    if (hrc == 0 && (w != width || h != height || b != bits)) st = -2;
                    else if (hrc == 0) {
                        // the samples behind the header, then the rest of the payload straight from the file
                        uint8_t* dst = h_pay + (size_t)i * area;
                        const size_t have = got - off < need ? got - off : need;
                        memcpy(dst, head.data() + off, have);
                        if (fread(dst + have, 1, need - have, f) == need - have) st = 0;
                    }
                } catch (...) {  // std::bad_alloc
                    st = -1;
                }
                fclose(f);
            }
            h_status[f0 + i] = st;
        });
        uint8_t* dev = (uint8_t*)ctx->loader_slot[k].dev.p;
        MRG_HIP_CHECK(hipMemcpyAsync(dev, h_pay, (size_t)n * area, hipMemcpyHostToDevice, s));
        return launch_pgm_unpack(ctx, dev, (int64_t)area, n, width, height, bits, (char*)d_out + (size_t)f0 * frame_pitch * es, frame_pitch,
                                 stride, s);
    };
    // a failed file's area holds whatever the slot held before: its frame is zeroed behind the launch; the chunk slots are
    // shared with the other loaders (ctx.h: loader_slot)
    return loader_ring(ctx, nfiles, chunk, (size_t)chunk * area, (size_t)chunk * area, stage,
                       zero_failed_frames(ctx, d_out, frame_pitch, stride, width, height, es, h_status), nullptr);
}

}  // extern "C"
