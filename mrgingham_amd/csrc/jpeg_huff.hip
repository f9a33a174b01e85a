// Baseline JPEG on the device, the entropy half: the restart intervals of a file are independent streams (byte aligned,
// DC predictors reset), so one lane Huffman-decodes one interval -- jpeg_huff_lane.h, the text the host runs under the
// sanitizers -- and the coefficients are born in HBM, where jpeg_idct_kernel expects them.  The host only finds the
// markers (jpeg_scan) and uploads the compressed bytes.  Files without restart intervals keep the host decoder, or,
// under option "jpeg_sync", go through the self-synchronising decoder of jpeg_huff_sync.hip.  See
// include/mrgingham_amd.h for the contract of mrgingham_amd_jpeg_entropy_batch and of option "jpeg_entropy", and
// DESIGN.md section 4.10 for the layout and the measured figures.
#include <string.h>

#include <algorithm>

#include "ctx.h"
#include "image_io.h"
#include "jpeg.h"
#include "jpeg_huff_lane.h"

using namespace mrg;

namespace {

constexpr int kLanes = 256;
constexpr int kTableDwords = (int)(sizeof(JpegHuffTable) / 4);

// One file of a chunk, as the kernel sees it (64 bytes).  Offsets are bytes into the chunk's staging image.
struct HuffFrame {
    uint64_t stream_off;      // its entropy-coded bytes (a multiple of 4; padded so that whole dwords can be read)
    uint32_t table_off;       // its ntables tables, JpegHuffTable each
    uint32_t interval_first;  // index of its first interval record and status byte
    int32_t nintervals;       // 0: the device does not take this file
    int32_t restart_interval, nmcu, ntables;
    JpegLaneGeom geom;
};
static_assert(sizeof(HuffFrame) == 64, "HuffFrame is laid out by hand in the staging image");

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

// One file of a chunk on the host.
struct FileJob {
    const uint8_t* data = nullptr;
    size_t nbytes = 0;
    JpegScan scan;
    int32_t status = -1;  // 0: the device takes it
    int ntables = 0;
    const JpegHuffTable* tables[kJpegLaneTables] = {};
    uint32_t slots = 0;
    size_t stream_bytes = 0;  // padded
    // where it lies in the staging image
    size_t stream_off = 0, table_off = 0, interval_first = 0;
    // status -3 and no restart intervals, option "jpeg_sync" on: jpeg_huff_sync.hip takes it, as file `sync` of the chunk's
    // JpegSyncChunk (-1: not)
    int sync = -1;
    uint32_t sync_len = 0;
};

// 0 the device takes it, -1 unreadable, -2 another size, -3 readable but the host has to decode it
void plan_file(const mrgingham_amd_ctx* ctx, FileJob& j, int width, int height, int blocks_w, int blocks_h) {
    const int max_interval = ctx->jpeg_entropy_max_interval;
    j.status = -1;
    j.ntables = 0;
    j.sync = -1;
    if (!j.data || jpeg_scan(j.data, j.nbytes, &j.scan)) return;
    const JpegScan& sc = j.scan;
    if (sc.info.width != width || sc.info.height != height || sc.info.blocks_w > blocks_w || sc.info.blocks_h > blocks_h) { j.status = -2; return; }
    j.status = -3;
    if (jpeg_sync_plan(ctx, j.data, j.nbytes, sc, &j.sync_len)) j.sync = 0;  // (numbered by sync_files)
    if (!sc.restart_interval || sc.restart_interval > (unsigned)max_interval || j.nbytes >= 0xFFFFFFF0u) return;
    j.slots = 0;
    for (int c = 0; c < sc.ncomp; ++c)
        for (int ac = 0; ac < 2; ++ac) {
            const JpegHuffTable* t = ac ? &sc.ac[sc.ta[c]] : &sc.dc[sc.td[c]];
            int s = 0;
            while (s < j.ntables && j.tables[s] != t) ++s;
            if (s == j.ntables) j.tables[j.ntables++] = t;  // (at most 2 * 3)
            j.slots |= (uint32_t)s << (4 * (ac ? 4 + c : c));
        }
    const size_t len = (size_t)(sc.intervals.back() - sc.entropy_begin);
    j.stream_bytes = ((len + 3) & ~(size_t)3) + 4;
    j.status = 0;
}

// The staging image of a chunk of n files: frame records | quantisation tables (n x 64 uint16, zeros for a file that is
// not decoded) | Huffman tables | interval records (two uint32: [begin, end) relative to the file's stream) |
// streams || status bytes.  Everything in front of the status bytes is uploaded, the status bytes come back.
struct Layout {
    size_t quant = 0, tables = 0, intervals = 0, streams = 0, status = 0, total = 0;
    size_t nintervals = 0;
    int most_intervals = 0, ndevice = 0;
};

Layout lay_out(FileJob* jobs, int n) {
    Layout l;
    l.quant = (size_t)n * sizeof(HuffFrame);
    l.tables = l.quant + (size_t)n * 64 * sizeof(uint16_t);
    size_t ntab = 0, nstream = 0;
    for (int i = 0; i < n; ++i) {
        FileJob& j = jobs[i];
        if (j.status != 0) continue;
        ++l.ndevice;
        j.table_off = l.tables + ntab * sizeof(JpegHuffTable);
        j.interval_first = l.nintervals;
        j.stream_off = nstream;  // (from l.streams, added below)
        ntab += (size_t)j.ntables;
        const size_t ni = j.scan.intervals.size() / 2;
        l.nintervals += ni;
        l.most_intervals = std::max(l.most_intervals, (int)ni);
        nstream += j.stream_bytes;
    }
    l.intervals = l.tables + ntab * sizeof(JpegHuffTable);
    l.streams = l.intervals + l.nintervals * 2 * sizeof(uint32_t);
    for (int i = 0; i < n; ++i) jobs[i].stream_off += l.streams;
    l.status = l.streams + nstream;
    l.total = l.status + ((l.nintervals + 3) & ~(size_t)3);
    return l;
}

// writes file i of the chunk into the image (every byte the kernel may read of it)
void fill_image(char* image, const Layout& l, const FileJob& j, int i, int blocks_h, int pitch_blocks) {
    HuffFrame fr;
    memset(&fr, 0, sizeof(fr));
    uint16_t* quant = (uint16_t*)(image + l.quant) + (size_t)i * 64;
    if (j.status != 0) {
        memset(quant, 0, 64 * sizeof(uint16_t));
        memcpy(image + (size_t)i * sizeof(HuffFrame), &fr, sizeof(fr));
        return;
    }
    const JpegScan& sc = j.scan;
    memcpy(quant, sc.info.quant, 64 * sizeof(uint16_t));
    fr.stream_off = j.stream_off;
    fr.table_off = (uint32_t)j.table_off;
    fr.interval_first = (uint32_t)j.interval_first;
    fr.nintervals = (int32_t)(sc.intervals.size() / 2);
    fr.restart_interval = (int32_t)sc.restart_interval;
    fr.nmcu = sc.mcus_x * sc.mcus_y;
    fr.ntables = j.ntables;
    fr.geom.ncomp = sc.ncomp;
    fr.geom.H0 = sc.comp_h[0];
    fr.geom.V0 = sc.comp_v[0];
    fr.geom.mcus_x = sc.mcus_x;
    for (int c = 0; c < sc.ncomp; ++c) fr.geom.nblk |= (uint32_t)(sc.comp_h[c] * sc.comp_v[c]) << (8 * c);
    fr.geom.slots = j.slots;
    fr.geom.blocks_h = blocks_h;
    fr.geom.pitch_blocks = pitch_blocks;
    memcpy(image + (size_t)i * sizeof(HuffFrame), &fr, sizeof(fr));
    for (int s = 0; s < j.ntables; ++s) memcpy(image + j.table_off + (size_t)s * sizeof(JpegHuffTable), j.tables[s], sizeof(JpegHuffTable));
    uint32_t* iv = (uint32_t*)(image + l.intervals) + 2 * j.interval_first;
    for (size_t q = 0; q < sc.intervals.size(); ++q) iv[q] = (uint32_t)(sc.intervals[q] - sc.entropy_begin);
    const size_t len = (size_t)(sc.intervals.back() - sc.entropy_begin);
    memcpy(image + j.stream_off, j.data + sc.entropy_begin, len);
    memset(image + j.stream_off + len, 0, j.stream_bytes - len);
    memset(image + l.status + j.interval_first, 0, (size_t)fr.nintervals);
}

// the files of a chunk that the sync path takes, numbered in order, and where they lie in slot k's buffers of that path
int sync_files(mrgingham_amd_ctx* ctx, int k, FileJob* jobs, int n, JpegSyncChunk* ch) {
    ch->files.clear();
    for (int i = 0; i < n; ++i) {
        FileJob& j = jobs[i];
        if (j.sync < 0) continue;
        j.sync = (int)ch->files.size();
        JpegSyncFile f;
        f.data = j.data;
        f.scan = &j.scan;
        f.len = j.sync_len;
        f.frame = i;
        ch->files.push_back(f);
    }
    return ch->files.empty() ? 0 : jpeg_sync_lay_out(ctx, k, ch);
}

int ensure_image(mrgingham_amd_ctx* ctx, int slot, size_t bytes) {
    int rc;
    if (bytes > ctx->jpeg_huff_dev[slot].bytes && (rc = ensure(ctx, ctx->jpeg_huff_dev[slot], bytes + bytes / 4))) return rc;
    return ensure_pinned(ctx, ctx->jpeg_huff_pin[slot], bytes, 4, false);
}

// Queues a filled image of slot k: the upload, the zeroing the chosen variant needs, the kernel, the status bytes back.
// d_coef: frame i of the chunk at d_coef + i * coef_pitch.  zero_others: files the device does not take get their
// coefficient area zeroed (the caller does not fill them itself).
int queue_huff(mrgingham_amd_ctx* ctx, int k, const Layout& l, const FileJob* jobs, int n, int16_t* d_coef, int64_t coef_pitch,
               size_t area_elems, bool zero_others, hipStream_t s) {
    char* pin = (char*)ctx->jpeg_huff_pin[k].p;
    char* dev = (char*)ctx->jpeg_huff_dev[k].p;
    MRG_HIP_CHECK(hipMemcpyAsync(dev, pin, l.status, hipMemcpyHostToDevice, s));
    const bool front = ctx->jpeg_entropy_memset != 0;
    if (front && l.ndevice == n && (size_t)coef_pitch == area_elems) {  // (dense frames: one piece)
        MRG_HIP_CHECK(hipMemsetAsync(d_coef, 0, (size_t)n * area_elems * sizeof(int16_t), s));
    } else {
        for (int i = 0; i < n; ++i)
            if (jobs[i].status == 0 ? front : zero_others)
                MRG_HIP_CHECK(hipMemsetAsync(d_coef + (size_t)i * (size_t)coef_pitch, 0, area_elems * sizeof(int16_t), s));
    }
    if (l.ndevice) {
        const unsigned groups = (unsigned)((l.most_intervals + kLanes - 1) / kLanes);
        // kernel timing on: a pair of events around the launches, read by mrgingham_amd_chess_kernel_ms like the response's
        hipEvent_t mark[2] = {nullptr, nullptr};
        if (ctx->timing) {
            for (hipEvent_t& e : mark)
                if (!(e = timing_event(ctx))) MRG_HIP_CHECK(hipGetLastError());  // (what kept it from being created)
            MRG_HIP_CHECK(hipEventRecord(mark[0], s));
        }
        for (int f0 = 0; f0 < n; f0 += 65535) {
            const dim3 grid(groups, (unsigned)std::min(n - f0, 65535));
            if (front)
                hipLaunchKernelGGL(jpeg_huff_kernel<false>, grid, dim3(kLanes), 0, s, (const uint8_t*)dev, (const HuffFrame*)dev,
                                   (const uint2*)(dev + l.intervals), f0, d_coef, (long long)coef_pitch, (uint8_t*)(dev + l.status));
            else
                hipLaunchKernelGGL(jpeg_huff_kernel<true>, grid, dim3(kLanes), 0, s, (const uint8_t*)dev, (const HuffFrame*)dev,
                                   (const uint2*)(dev + l.intervals), f0, d_coef, (long long)coef_pitch, (uint8_t*)(dev + l.status));
        }
        MRG_HIP_CHECK(hipGetLastError());
        if (mark[0]) {
            MRG_HIP_CHECK(hipEventRecord(mark[1], s));
            ctx->timing_events.pairs.emplace_back(mark[0], mark[1]);
        }
        MRG_HIP_CHECK(hipMemcpyAsync(pin + l.status, dev + l.status, l.total - l.status, hipMemcpyDeviceToHost, s));
    }
    return 0;
}

// after the stream has passed the status download: every interval of the file decoded?
bool all_decoded(const char* pin, const Layout& l, const FileJob& j) {
    const uint8_t* st = (const uint8_t*)pin + l.status + j.interval_first;
    const size_t ni = j.scan.intervals.size() / 2;
    for (size_t i = 0; i < ni; ++i)
        if (st[i] != 1) return false;
    return true;
}

}  // namespace

namespace mrg {

int read_jpegs_device_entropy(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height,
                              uint8_t* d_out, int64_t frame_pitch, int stride, int nthreads, int32_t* h_status, int bw, int bh,
                              int chunk) {
    const size_t per_frame = (size_t)bw * bh * 64;  // elements
    const size_t slot_bytes = (size_t)chunk * (per_frame * sizeof(int16_t) + 64 * sizeof(uint16_t));
    hipStream_t s = ctx->pix;
    std::vector<FileJob> jobs[2];
    std::vector<std::vector<uint8_t>> files[2];
    Layout lay[2];
    JpegSyncChunk sync[2];
    int first[2] = {0, 0}, count[2] = {0, 0};
    // (the coefficient staging of a slot is grown where there is a file for the host threads to decode)
    auto host_coef = [&](int k) { return ensure_pinned(ctx, ctx->loader_slot[k].pin, slot_bytes, 0, true); };
    // the chunk in slot k has passed the stream: its status bytes are on the host.  A file with a failed interval is
    // unreadable, and its frame is zeroed behind the transform that has run over it.
    // A file of the sync path whose write pass failed is unreadable as well; one that did not converge within the cap is
    // known only now: the pool threads decode those, their coefficient slices are uploaded and the transform runs over
    // their frames again (the table is in the image already).
    auto finish = [&](int k) -> int {
        std::vector<int> late;
        for (int i = 0; i < count[k]; ++i) {
            const FileJob& j = jobs[k][i];
            int32_t st = 0;
            if (j.status == 0) st = all_decoded((const char*)ctx->jpeg_huff_pin[k].p, lay[k], j) ? 0 : -1;
            else if (j.sync >= 0) st = jpeg_sync_status(ctx, k, sync[k], j.sync, nullptr);
            if (st == -3) late.push_back(i);
            if (st == -1) {
                h_status[first[k] + i] = -1;
                MRG_HIP_CHECK(zero_frame(d_out, first[k] + i, frame_pitch, stride, width, height, 1, s));
            }
        }
        if (late.empty()) return 0;
        int rc;
        if ((rc = host_coef(k))) return rc;
        int16_t* h_coef = (int16_t*)ctx->loader_slot[k].pin.p;
        for_files(ctx->pool, nthreads, (int)late.size(), [&](int q) {
            const int i = late[(size_t)q];
            const FileJob& j = jobs[k][i];
            JpegInfo info;
            h_status[first[k] + i] = jpeg_coefficients(j.data, j.nbytes, h_coef + (size_t)i * per_frame, per_frame, bw, &info) == 0 ? 0 : -1;
        });
        char* dev = (char*)ctx->loader_slot[k].dev.p;
        const uint16_t* d_quant = (const uint16_t*)((char*)ctx->jpeg_huff_dev[k].p + lay[k].quant);
        for (int i : late) {
            if (h_status[first[k] + i] != 0) {
                MRG_HIP_CHECK(zero_frame(d_out, first[k] + i, frame_pitch, stride, width, height, 1, s));
                continue;
            }
            int16_t* d_slice = (int16_t*)dev + (size_t)i * per_frame;
            MRG_HIP_CHECK(hipMemcpyAsync(d_slice, h_coef + (size_t)i * per_frame, per_frame * sizeof(int16_t), hipMemcpyHostToDevice, s));
            launch_jpeg_idct(d_slice, (int64_t)per_frame, d_quant + (size_t)i * 64, 1, width, height, bw,
                             d_out + (size_t)(first[k] + i) * frame_pitch, frame_pitch, stride, s);
        }
        MRG_HIP_CHECK(hipGetLastError());
        MRG_HIP_CHECK(hipStreamSynchronize(s));  // (the slot's staging is filled again next)
        return 0;
    };
    auto stage = [&](int k, int f0, int n) -> int {
        int rc;
        jobs[k].resize((size_t)chunk);
        files[k].resize((size_t)chunk);
        first[k] = f0;
        count[k] = n;
        // 1. host threads read and scan
        for_files(ctx->pool, nthreads, n, [&](int i) {
            FileJob& j = jobs[k][i];
            j.data = nullptr;
            try {
                if (read_file(filenames[f0 + i], files[k][i])) {
                    j.data = files[k][i].data();
                    j.nbytes = files[k][i].size();
                }
                plan_file(ctx, j, width, height, bw, bh);
            } catch (...) {  // std::bad_alloc on a file too large to hold
                j.status = -1;
            }
        });
        lay[k] = lay_out(jobs[k].data(), n);
        if ((rc = ensure_image(ctx, k, lay[k].total))) return rc;
        if ((rc = sync_files(ctx, k, jobs[k].data(), n, &sync[k]))) return rc;
        int nhost = 0;
        for (int i = 0; i < n; ++i) nhost += jobs[k][i].status == -3 && jobs[k][i].sync < 0;
        if (nhost && (rc = host_coef(k))) return rc;
        int16_t* h_coef = (int16_t*)ctx->loader_slot[k].pin.p;
        // 2. the files the device takes go into the image; 3. the others are decoded by the same threads as without the
        // option, into the coefficient staging
        char* image = (char*)ctx->jpeg_huff_pin[k].p;
        for_files(ctx->pool, nthreads, n, [&](int i) {
            FileJob& j = jobs[k][i];
            int32_t st = j.status;
            if (j.sync >= 0) {  // (decoded unless finish() finds otherwise)
                jpeg_sync_fill(ctx, k, sync[k], j.sync, bh, bw);
                st = 0;
            } else if (st == -3) {
                JpegInfo info;
                st = jpeg_coefficients(j.data, j.nbytes, h_coef + (size_t)i * per_frame, per_frame, bw, &info) == 0 ? 0 : -1;
            }
            fill_image(image, lay[k], j, i, bh, bw);
            if (j.status == -3 && st == 0) memcpy((uint16_t*)(image + lay[k].quant) + (size_t)i * 64, j.scan.info.quant, 64 * sizeof(uint16_t));
            h_status[f0 + i] = st;
        });
        char* dev = (char*)ctx->loader_slot[k].dev.p;
        for (int i = 0; i < n; ++i)  // only the slices the host has decoded are uploaded as coefficients
            if (jobs[k][i].status == -3 && jobs[k][i].sync < 0 && h_status[f0 + i] == 0)
                MRG_HIP_CHECK(hipMemcpyAsync(dev + (size_t)i * per_frame * sizeof(int16_t), h_coef + (size_t)i * per_frame,
                                             per_frame * sizeof(int16_t), hipMemcpyHostToDevice, s));
        if ((rc = queue_huff(ctx, k, lay[k], jobs[k].data(), n, (int16_t*)dev, (int64_t)per_frame, per_frame, false, s))) return rc;
        if ((rc = jpeg_sync_launch(ctx, k, sync[k], (int16_t*)dev, (int64_t)per_frame, per_frame, s))) return rc;
        launch_jpeg_idct((const int16_t*)dev, (int64_t)per_frame, (const uint16_t*)((char*)ctx->jpeg_huff_dev[k].p + lay[k].quant), n, width,
                         height, bw, d_out + (size_t)f0 * frame_pitch, frame_pitch, stride, s);
        MRG_HIP_CHECK(hipGetLastError());
        return 0;
    };
    auto zero_failed = [&](int, int f0, int n) -> int {
        for (int i = f0; i < f0 + n; ++i)
            if (h_status[i] != 0) MRG_HIP_CHECK(zero_frame(d_out, i, frame_pitch, stride, width, height, 1, s));
        return 0;
    };
    return loader_ring(ctx, nfiles, chunk, slot_bytes, 0, stage, zero_failed, finish);
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
    if (width > 32767 || height > 32767)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "frames larger than 32767 pixels per side are not supported");
    if (blocks_w > 4100 || blocks_h > 4100 || (long long)blocks_w * 8 < width || (long long)blocks_h * 8 < height)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "blocks_w x blocks_h does not cover width x height");
    if (coef_pitch < (int64_t)blocks_w * blocks_h * 64 || (coef_pitch & 7) || ((uintptr_t)d_coef & 15))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "coefficients: 16-byte aligned, coef_pitch a multiple of 8 and at least blocks_w*blocks_h*64");
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
    std::vector<FileJob> jobs;
    for (int f0 = 0; f0 < nfiles;) {
        int n = 0;
        for (size_t bytes = 0; f0 + n < nfiles && n < 4096 && (n == 0 || bytes + nbytes[f0 + n] <= ((size_t)256 << 20)); ++n) bytes += nbytes[f0 + n];
        jobs.resize((size_t)n);
        for_files(ctx->pool, nthreads, n, [&](int i) {
            jobs[i].data = data[f0 + i];
            jobs[i].nbytes = nbytes[f0 + i];
            try {
                plan_file(ctx, jobs[i], width, height, blocks_w, blocks_h);
            } catch (...) {
                jobs[i].status = -1;
            }
        });
        const Layout l = lay_out(jobs.data(), n);
        int rc;
        if ((rc = ensure_image(ctx, 0, l.total))) return rc;
        JpegSyncChunk sync;
        if ((rc = sync_files(ctx, 0, jobs.data(), n, &sync))) return rc;
        char* image = (char*)ctx->jpeg_huff_pin[0].p;
        for_files(ctx->pool, nthreads, n, [&](int i) {
            fill_image(image, l, jobs[i], i, blocks_h, blocks_w);
            if (jobs[i].sync < 0) return;  // (its table goes up with the others; taken back below if it fails)
            jpeg_sync_fill(ctx, 0, sync, jobs[i].sync, blocks_h, blocks_w);
            memcpy((uint16_t*)(image + l.quant) + (size_t)i * 64, jobs[i].scan.info.quant, 64 * sizeof(uint16_t));
        });
        int16_t* coef = d_coef + (size_t)f0 * (size_t)coef_pitch;
        if ((rc = queue_huff(ctx, 0, l, jobs.data(), n, coef, coef_pitch, area, true, s))) return rc;
        if ((rc = jpeg_sync_launch(ctx, 0, sync, coef, coef_pitch, area, s))) return rc;
        MRG_HIP_CHECK(hipMemcpyAsync(d_quant + (size_t)f0 * 64, image + l.quant, (size_t)n * 64 * sizeof(uint16_t), hipMemcpyHostToDevice, s));
        MRG_HIP_CHECK(hipStreamSynchronize(s));
        bool again = false;
        for (int i = 0; i < n; ++i) {
            int32_t st = jobs[i].status;
            const int32_t synced = jobs[i].sync >= 0 ? jpeg_sync_status(ctx, 0, sync, jobs[i].sync, nullptr) : 0;
            if (jobs[i].sync >= 0 && synced == 0) st = 0;
            if ((st == 0 && jobs[i].sync < 0 && !all_decoded(image, l, jobs[i])) || synced != 0) {
                // unreadable after all (or not converged within the cap: -3 stays): no half-decoded coefficients, no table
                st = synced ? synced : -1;
                MRG_HIP_CHECK(hipMemsetAsync(coef + (size_t)i * (size_t)coef_pitch, 0, area * sizeof(int16_t), s));
                MRG_HIP_CHECK(hipMemsetAsync(d_quant + (size_t)(f0 + i) * 64, 0, 64 * sizeof(uint16_t), s));
                again = true;
            }
            h_status[f0 + i] = st;
        }
        if (again) MRG_HIP_CHECK(hipStreamSynchronize(s));
        f0 += n;
    }
    return MRGINGHAM_AMD_OK;
}

}  // extern "C"
