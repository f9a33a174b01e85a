// Baseline JPEG on the device, the entropy half: the restart intervals of a file are independent streams (byte aligned,
// DC predictors reset), so one lane Huffman-decodes one interval -- jpeg_huff_lane.h, the text the host runs under the
// sanitizers -- and the coefficients are born in HBM, where jpeg_idct_kernel expects them.  The host only finds the
// markers (jpeg_scan) and uploads the compressed bytes.  Files without restart intervals keep the host decoder, or,
// under option "jpeg_sync", go through the self-synchronising decoder of jpeg_huff_sync.hip.  See
// include/mrgingham_amd.h for the contract of mrgingham_amd_jpeg_entropy_batch and of option "jpeg_entropy",
// jpeg_stage.h for the staging images of both decoders (which files they take, the layout, the bytes), and DESIGN.md
// section 4.10 for the measured figures.  What is left here needs the context or the device: the kernel, the chunk driver
// both callers run, the loader route and the batch entry point.
#include <string.h>

#include <algorithm>

#include "ctx.h"
#include "image_io.h"
#include "jpeg_huff_lane.h"
#include "jpeg_stage.h"

using namespace mrg;

namespace {

constexpr int kLanes = 256;
constexpr int kTableDwords = (int)(sizeof(JpegHuffTable) / 4);

__constant__ uint8_t kNaturalDev[64] = {MRG_JPEG_NATURAL_ORDER};

// Grid = (groups of 256 intervals, frames); lane = one restart interval of its frame.  The tables the frame's scan names
// (at most six) are copied to LDS once per workgroup; a lane runs the shared decoder over its interval and stores ONE
// status byte (1 decoded, 2 failed) with a plain store -- the host reduces them per file.  Nothing here trusts the
// stream: see jpeg_huff_lane.h for what is checked.  The records (`frames`, `intervals`) are written by the host from a
// scan it has validated.
template <bool kWholeBlocks>
__global__ __launch_bounds__(kLanes) void jpeg_huff_kernel(const uint8_t* __restrict__ image, const HuffFrame* __restrict__ frames,
                                                           const uint2* __restrict__ intervals, int frame0, int16_t* __restrict__ coef,
                                                           long long coef_pitch, uint8_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint32_t stab[kJpegLaneTables * kTableDwords];
    __shared__ uint8_t snat[64];
    const int t = threadIdx.x, f = frame0 + blockIdx.y;
    const HuffFrame fr = frames[f];
    if ((int)(blockIdx.x * kLanes) >= fr.nintervals) return;  // (the whole workgroup: the grid is sized by the largest file)
    const int ntab = fr.ntables < kJpegLaneTables ? fr.ntables : kJpegLaneTables;
    const uint32_t* src = (const uint32_t*)(image + fr.table_off);
    for (int i = t; i < ntab * kTableDwords; i += kLanes) stab[i] = src[i];
    if (t < 64) snat[t] = kNaturalDev[t];
    __syncthreads();
    const int i = (int)(blockIdx.x * kLanes) + t;
    if (i >= fr.nintervals) return;
    const uint2 iv = intervals[fr.interval_first + (uint32_t)i];
    const uint32_t first = (uint32_t)i * (uint32_t)fr.restart_interval;
    const uint32_t left = (uint32_t)fr.nmcu - first;
    const bool ok = jpeg_huff_lane<kWholeBlocks>(image + fr.stream_off, iv.x, iv.y, (const JpegHuffTable*)stab, snat, fr.geom, first,
                                                 left < (uint32_t)fr.restart_interval ? left : (uint32_t)fr.restart_interval,
                                                 i == fr.nintervals - 1, coef + (long long)f * coef_pitch);
    status[fr.interval_first + (uint32_t)i] = ok ? 1 : 2;
}

// One chunk of files through both device decoders, in slot k of the context's staging buffers: plan() scans the files on
// the pool, lays out both images (jpeg_stage.h) and grows the slot's buffers; fill(i) writes file i into its image (any
// thread, one per file); queue() puts the uploads, the zeroing, the kernels and the read-backs on the stream -- the
// interval decoder first, then the sync decoder; once the stream has passed them, outcome(i) tells what became of file i.
struct EntropyChunk {
    mrgingham_amd_ctx* ctx;
    int k;
    std::vector<JpegStageFile> files;
    int n = 0, blocks_w = 0, blocks_h = 0;
    JpegImageLayout huff;
    JpegSyncLayout sync;

    char* huff_image() const { return (char*)ctx->jpeg_huff_pin[k].p; }
    uint16_t* quant(int i) const { return (uint16_t*)(huff_image() + huff.quant) + (size_t)i * 64; }  // of file i, in the image
    const uint16_t* d_quant() const { return (const uint16_t*)((char*)ctx->jpeg_huff_dev[k].p + huff.quant); }

    // load(i, file) gives file i its data and nbytes (data stays NULL: unreadable); it runs on the pool and may throw
    template <class F>
    int plan(int nthreads, int count, int width, int height, int bw, int bh, F&& load) {
        n = count;
        blocks_w = bw;
        blocks_h = bh;
        if (files.size() < (size_t)n) files.resize((size_t)n);
        for_files(ctx->pool, nthreads, n, [&](int i) {
            JpegStageFile& j = files[(size_t)i];
            j.data = nullptr;
            try {
                load(i, j);
                jpeg_stage_plan(j, width, height, bw, bh, ctx->jpeg_entropy_max_interval, ctx->jpeg_sync != 0);
            } catch (...) {  // std::bad_alloc on a file too large to hold
                j.status = -1;
                j.route = JpegRoute::kNone;
            }
        });
        huff = jpeg_huff_lay_out(files.data(), n);
        sync = jpeg_sync_lay_out(files.data(), n, (uint32_t)ctx->jpeg_sync_subsequence);
        int rc;
        if (huff.total > ctx->jpeg_huff_dev[k].bytes && (rc = ensure(ctx, ctx->jpeg_huff_dev[k], huff.total + huff.total / 4))) return rc;
        if ((rc = ensure_pinned(ctx, ctx->jpeg_huff_pin[k], huff.total, 4, false))) return rc;
        return jpeg_sync_grow(ctx, k, sync);
    }

    void fill(int i) {
        const JpegStageFile& j = files[(size_t)i];
        jpeg_huff_fill(huff_image(), huff.total, huff, j, i, blocks_h, blocks_w);
        if (j.route == JpegRoute::kSync) jpeg_sync_fill((char*)ctx->jpeg_sync_pin[k].p, sync.total, sync, j, j.index, blocks_h, blocks_w);
    }

    // d_coef: frame i of the chunk at d_coef + i * coef_pitch.  zero_others: the files the interval decoder does not take
    // get their coefficient area zeroed (otherwise the caller fills them).
    int queue(int16_t* d_coef, int64_t coef_pitch, size_t area_elems, bool zero_others, hipStream_t s) {
        char* pin = huff_image();
        char* dev = (char*)ctx->jpeg_huff_dev[k].p;
        MRG_HIP_CHECK(hipMemcpyAsync(dev, pin, huff.back, hipMemcpyHostToDevice, s));
        const bool front = ctx->jpeg_entropy_memset != 0;
        if (front && huff.nfiles == n && (size_t)coef_pitch == area_elems) {  // (dense frames: one piece)
            MRG_HIP_CHECK(hipMemsetAsync(d_coef, 0, (size_t)n * area_elems * sizeof(int16_t), s));
        } else {
            for (int i = 0; i < n; ++i)
                if (files[(size_t)i].route == JpegRoute::kIntervals ? front : zero_others)
                    MRG_HIP_CHECK(hipMemsetAsync(d_coef + (size_t)i * (size_t)coef_pitch, 0, area_elems * sizeof(int16_t), s));
        }
        if (huff.nfiles) {
            const unsigned groups = (unsigned)((huff.most_items + kLanes - 1) / kLanes);
            TimingBracket mark;
            MRG_HIP_CHECK(mark.begin(ctx, 0, 1));
            MRG_HIP_CHECK(mark.tick(ctx, 0, s));
            const auto kernel = front ? jpeg_huff_kernel<false> : jpeg_huff_kernel<true>;
            for_frame_slabs(n, [&](int f0, unsigned nf) {
                hipLaunchKernelGGL(kernel, dim3(groups, nf), dim3(kLanes), 0, s, (const uint8_t*)dev, (const HuffFrame*)dev,
                                   (const uint2*)(dev + huff.items), f0, d_coef, (long long)coef_pitch, (uint8_t*)(dev + huff.back));
            });
            MRG_HIP_CHECK(hipGetLastError());
            MRG_HIP_CHECK(mark.tick(ctx, 1, s));
            MRG_HIP_CHECK(hipMemcpyAsync(pin + huff.back, dev + huff.back, huff.total - huff.back, hipMemcpyDeviceToHost, s));
        }
        return jpeg_sync_launch(ctx, k, sync, files.data(), n, d_coef, coef_pitch, area_elems, s);
    }

    // 0 decoded; -1 unreadable; -3 the host has to decode it (no decoder took it, or it did not converge within the cap);
    // -2 another size
    int32_t outcome(int i) const {
        const JpegStageFile& j = files[(size_t)i];
        if (j.route == JpegRoute::kSync) return jpeg_sync_status(ctx, k, sync, j.index);
        if (j.route == JpegRoute::kNone) return j.status;
        const uint8_t* st = (const uint8_t*)huff_image() + huff.back + j.item_first;
        for (uint32_t q = 0; q < j.nitems; ++q)
            if (st[q] != 1) return -1;  // (an interval failed)
        return 0;
    }
};

}  // namespace

namespace mrg {

hipError_t TimingBracket::begin(mrgingham_amd_ctx* ctx, int open_at, int close_at) {
    open = open_at;
    close = close_at;
    if (!ctx->timing) return hipSuccess;
    for (hipEvent_t& e : mark)
        if (!(e = timing_event(ctx))) {
            const hipError_t err = hipGetLastError();  // (what kept it from being created)
            if (err != hipSuccess) return err;
        }
    return hipSuccess;
}

hipError_t TimingBracket::tick(mrgingham_amd_ctx* ctx, int boundary, hipStream_t s) {
    if (!mark[0]) return hipSuccess;
    if (boundary == open) return hipEventRecord(mark[0], s);
    if (boundary != close) return hipSuccess;
    const hipError_t err = hipEventRecord(mark[1], s);
    if (err == hipSuccess) ctx->timing_events.pairs.emplace_back(mark[0], mark[1]);
    return err;
}

int read_jpegs_device_entropy(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height,
                              uint8_t* d_out, int64_t frame_pitch, int stride, int nthreads, int32_t* h_status, int bw, int bh,
                              int chunk) {
    const size_t per_frame = (size_t)bw * bh * 64;  // elements
    const size_t slot_bytes = (size_t)chunk * (per_frame * sizeof(int16_t) + 64 * sizeof(uint16_t));
    hipStream_t s = ctx->pix;
    EntropyChunk chunks[2] = {{ctx, 0}, {ctx, 1}};
    std::vector<std::vector<uint8_t>> bytes[2];
    int first[2] = {0, 0};
    // (the coefficient staging of a slot is grown where there is a file for the host threads to decode)
    auto host_coef = [&](int k) { return ensure_pinned(ctx, ctx->loader_slot[k].pin, slot_bytes, 0, true); };
    // the host decode of file i of the chunk in slot k into the slot's coefficient staging: 0 or -1
    auto host_decode = [&](int k, int i) -> int32_t {
        const JpegStageFile& j = chunks[k].files[(size_t)i];
        JpegInfo info;
        return jpeg_coefficients(j.data, j.nbytes, (int16_t*)ctx->loader_slot[k].pin.p + (size_t)i * per_frame, per_frame, bw, &info) == 0 ? 0 : -1;
    };
    // the chunk in slot k has passed the stream: its status bytes and sync words are on the host.  A file a decoder took
    // and found unreadable has its frame zeroed behind the transform that has run over it.  One that did not converge
    // within the cap is known only now: the pool threads decode those, their coefficient slices are uploaded and the
    // transform runs over their frames again (the table is in the image already).
    auto finish = [&](int k) -> int {
        const EntropyChunk& ch = chunks[k];
        std::vector<int> late;
        for (int i = 0; i < ch.n; ++i) {
            if (ch.files[(size_t)i].route == JpegRoute::kNone) continue;  // (settled in stage)
            const int32_t st = ch.outcome(i);
            if (st == -3) late.push_back(i);
            if (st == -1) {
                h_status[first[k] + i] = -1;
                MRG_HIP_CHECK(zero_frame(d_out, first[k] + i, frame_pitch, stride, width, height, 1, s));
            }
        }
        if (late.empty()) return 0;
        int rc;
        if ((rc = host_coef(k))) return rc;
        for_files(ctx->pool, nthreads, (int)late.size(), [&](int q) { h_status[first[k] + late[(size_t)q]] = host_decode(k, late[(size_t)q]); });
        int16_t* h_coef = (int16_t*)ctx->loader_slot[k].pin.p;
        char* dev = (char*)ctx->loader_slot[k].dev.p;
        for (int i : late) {
            if (h_status[first[k] + i] != 0) {
                MRG_HIP_CHECK(zero_frame(d_out, first[k] + i, frame_pitch, stride, width, height, 1, s));
                continue;
            }
            int16_t* d_slice = (int16_t*)dev + (size_t)i * per_frame;
            MRG_HIP_CHECK(hipMemcpyAsync(d_slice, h_coef + (size_t)i * per_frame, per_frame * sizeof(int16_t), hipMemcpyHostToDevice, s));
            launch_jpeg_idct(d_slice, (int64_t)per_frame, ch.d_quant() + (size_t)i * 64, 1, width, height, bw,
                             d_out + (size_t)(first[k] + i) * frame_pitch, frame_pitch, stride, s);
        }
        MRG_HIP_CHECK(hipGetLastError());
        MRG_HIP_CHECK(hipStreamSynchronize(s));  // (the slot's staging is filled again next)
        return 0;
    };
    auto stage = [&](int k, int f0, int n) -> int {
        int rc;
        EntropyChunk& ch = chunks[k];
        bytes[k].resize((size_t)chunk);
        first[k] = f0;
        // 1. host threads read and scan
        if ((rc = ch.plan(nthreads, n, width, height, bw, bh, [&](int i, JpegStageFile& j) {
                if (!read_file(filenames[f0 + i], bytes[k][(size_t)i])) return;
                j.data = bytes[k][(size_t)i].data();
                j.nbytes = bytes[k][(size_t)i].size();
            })))
            return rc;
        auto for_host = [&](int i) { return ch.files[(size_t)i].status == -3 && ch.files[(size_t)i].route == JpegRoute::kNone; };
        int nhost = 0;
        for (int i = 0; i < n; ++i) nhost += for_host(i);
        if (nhost && (rc = host_coef(k))) return rc;
        // 2. the files a decoder takes go into its image (decoded unless finish() finds otherwise); 3. the others are
        // decoded by the same threads as without the option, into the coefficient staging, and their table joins the image
        for_files(ctx->pool, nthreads, n, [&](int i) {
            const JpegStageFile& j = ch.files[(size_t)i];
            const int32_t st = for_host(i) ? host_decode(k, i) : j.route == JpegRoute::kNone ? j.status : 0;
            ch.fill(i);
            if (j.status == -3 && st == 0) memcpy(ch.quant(i), j.scan.info.quant, 64 * sizeof(uint16_t));
            h_status[f0 + i] = st;
        });
        int16_t* h_coef = (int16_t*)ctx->loader_slot[k].pin.p;
        char* dev = (char*)ctx->loader_slot[k].dev.p;
        for (int i = 0; i < n; ++i)  // only the slices the host has decoded are uploaded as coefficients
            if (for_host(i) && h_status[f0 + i] == 0)
                MRG_HIP_CHECK(hipMemcpyAsync(dev + (size_t)i * per_frame * sizeof(int16_t), h_coef + (size_t)i * per_frame,
                                             per_frame * sizeof(int16_t), hipMemcpyHostToDevice, s));
        if ((rc = ch.queue((int16_t*)dev, (int64_t)per_frame, per_frame, false, s))) return rc;
        launch_jpeg_idct((const int16_t*)dev, (int64_t)per_frame, ch.d_quant(), n, width, height, bw, d_out + (size_t)f0 * frame_pitch,
                         frame_pitch, stride, s);
        MRG_HIP_CHECK(hipGetLastError());
        return 0;
    };
    return loader_ring(ctx, nfiles, chunk, slot_bytes, 0, stage, zero_failed_frames(ctx, d_out, frame_pitch, stride, width, height, 1, h_status),
                       finish);
}

}  // namespace mrg

extern "C" {

int mrgingham_amd_jpeg_restart_intervals(const uint8_t* data, size_t nbytes, int* restart_interval, int64_t* offsets,
                                         size_t capacity, size_t* nintervals) {
    if (!data) return -1;
    JpegScan sc;
    try {
        if (jpeg_scan(data, nbytes, &sc)) return -1;
    } catch (...) {
        return -1;
    }
    const size_t n = sc.intervals.size() / 2;
    if (restart_interval) *restart_interval = (int)sc.restart_interval;
    if (nintervals) *nintervals = n;
    if (!offsets) return 0;
    if (capacity < n) return -2;
    for (size_t i = 0; i < 2 * n; ++i) offsets[i] = (int64_t)sc.intervals[i];
    return 0;
}

int mrgingham_amd_jpeg_entropy_batch(mrgingham_amd_ctx* ctx, const uint8_t* const* data, const size_t* nbytes, int nfiles, int width,
                                     int height, int16_t* d_coef, int64_t coef_pitch, int blocks_w, int blocks_h, uint16_t* d_quant,
                                     int32_t* h_status) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (nfiles < 0 || width <= 0 || height <= 0 || blocks_w < 0 || blocks_h < 0 || coef_pitch < 0 ||
        (nfiles > 0 && (!data || !nbytes || !d_coef || !d_quant || !h_status)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad JPEG entropy batch descriptor");
    int rc = check_coef_area(ctx, d_coef, coef_pitch, width, height, blocks_w, blocks_h);
    if (rc) return rc;
    for (int i = 0; i < nfiles; ++i)
        if (!data[i]) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "file %d of the JPEG entropy batch is NULL", i);
    if (nfiles == 0) return 0;
    fb_drain(ctx);
    const CallerDevice caller_device_;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->pix;
    const size_t area = (size_t)blocks_w * blocks_h * 64;
    const int nthreads = host_threads(0);
    // chunks of files whose compressed bytes stay near 256 MB (one staging image, reused: the call is synchronous)
    EntropyChunk ch{ctx, 0};
    for (int f0 = 0; f0 < nfiles;) {
        int n = 0;
        for (size_t bytes = 0; f0 + n < nfiles && n < 4096 && (n == 0 || bytes + nbytes[f0 + n] <= ((size_t)256 << 20)); ++n) bytes += nbytes[f0 + n];
        if ((rc = ch.plan(nthreads, n, width, height, blocks_w, blocks_h, [&](int i, JpegStageFile& j) {
                j.data = data[f0 + i];
                j.nbytes = nbytes[f0 + i];
            })))
            return rc;
        for_files(ctx->pool, nthreads, n, [&](int i) {
            ch.fill(i);  // (the table of a sync file goes up with the others; taken back below if it fails)
            if (ch.files[(size_t)i].route == JpegRoute::kSync) memcpy(ch.quant(i), ch.files[(size_t)i].scan.info.quant, 64 * sizeof(uint16_t));
        });
        int16_t* coef = d_coef + (size_t)f0 * (size_t)coef_pitch;
        if ((rc = ch.queue(coef, coef_pitch, area, true, s))) return rc;
        MRG_HIP_CHECK(hipMemcpyAsync(d_quant + (size_t)f0 * 64, ch.quant(0), (size_t)n * 64 * sizeof(uint16_t), hipMemcpyHostToDevice, s));
        MRG_HIP_CHECK(hipStreamSynchronize(s));
        bool again = false;
        for (int i = 0; i < n; ++i) {
            const int32_t st = h_status[f0 + i] = ch.outcome(i);
            if (st == 0 || ch.files[(size_t)i].route == JpegRoute::kNone) continue;
            // unreadable after all, or not converged within the cap: no half-decoded coefficients, no table
            MRG_HIP_CHECK(hipMemsetAsync(coef + (size_t)i * (size_t)coef_pitch, 0, area * sizeof(int16_t), s));
            MRG_HIP_CHECK(hipMemsetAsync(d_quant + (size_t)(f0 + i) * 64, 0, 64 * sizeof(uint16_t), s));
            again = true;
        }
        if (again) MRG_HIP_CHECK(hipStreamSynchronize(s));
        f0 += n;
    }
    return MRGINGHAM_AMD_OK;
}

}  // extern "C"
