// Baseline JPEG on the device, the entropy half for files WITHOUT restart markers: the entropy-coded segment is cut into
// subsequences of S raw bytes, one lane each, that decode from a guessed state and are then re-entered from their left
// neighbour's exit until nothing changes -- jpeg_huff_sync.h, the text the host runs under the sanitizers, has the
// decoder, DESIGN.md section 4.10 the method and the measured figures, include/mrgingham_amd.h the options "jpeg_sync",
// "jpeg_sync_subsequence" and "jpeg_sync_max_rounds".  Four kernels, all plain launches that the stream orders: round 0,
// R + 1 update rounds (a file that has converged costs its workgroups one load), the scan, the write pass.  No kernel
// waits for another workgroup.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "jpeg.h"
#include "jpeg_huff_sync.h"

using namespace mrg;

namespace {

constexpr int kLanes = 256;
constexpr int kTableDwords = (int)(sizeof(JpegHuffTable) / 4);

// One file of a chunk, as the kernels see it (80 bytes).  Offsets are bytes into the chunk's staging image.
struct SyncFrame {
    uint64_t stream_off;  // its entropy-coded bytes (a multiple of 4; padded so that whole dwords can be read)
    uint32_t table_off;   // its ntables tables, JpegHuffTable each
    uint32_t rec_first;   // index of its first record
    uint32_t nsub, len, total, ntables;
    uint32_t frame;       // which coefficient area of the chunk is its own
    uint32_t unused[3];
    JpegLaneGeom geom;
};
static_assert(sizeof(SyncFrame) == 80, "SyncFrame is laid out by hand in the staging image");

// What the kernels keep per file (zeroed in front of round 0, read back behind the write pass).
struct SyncWords {
    uint32_t last_changed;  // the last update round (1 ..) that changed one of its records
    uint32_t flags;         // kReached / kError from the write pass, kScanReached / kNotConverged from the scan
};
constexpr uint32_t kReached = 1, kError = 2, kScanReached = 4, kNotConverged = 8;

__constant__ uint8_t kNaturalSync[64] = {MRG_JPEG_NATURAL_ORDER};

__device__ inline void load_tables(uint32_t* stab, uint8_t* snat, const uint8_t* image, const SyncFrame& fr) {
    const int t = threadIdx.x;
    const int ntab = fr.ntables < (uint32_t)kJpegLaneTables ? (int)fr.ntables : kJpegLaneTables;
    const uint32_t* src = (const uint32_t*)(image + fr.table_off);
    for (int i = t; i < ntab * kTableDwords; i += kLanes) stab[i] = src[i];
    if (t < 64) snat[t] = kNaturalSync[t];
    __syncthreads();
}

__device__ inline uint32_t sub_end(const SyncFrame& fr, uint32_t i, uint32_t S) {
    const uint32_t begin = i * S;
    return begin + S < fr.len ? begin + S : fr.len;
}

// Round 0.  Grid = (groups of 256 subsequences, files); lane = one subsequence, decoded from the file's true start (the
// first) or from its own first byte with (m, k) = (0, 0).  The record goes to `spec`, where it stays, and to `cur`.
__global__ __launch_bounds__(kLanes) void jpeg_sync_spec_kernel(const uint8_t* __restrict__ image, const SyncFrame* __restrict__ frames,
                                                                int frame0, uint32_t S, JpegSyncRecord* __restrict__ spec,
                                                                JpegSyncRecord* __restrict__ cur) {
    __shared__ __attribute__((aligned(16))) uint32_t stab[kJpegLaneTables * kTableDwords];
    __shared__ uint8_t snat[64];
    const SyncFrame fr = frames[frame0 + blockIdx.y];
    if (blockIdx.x * kLanes >= fr.nsub) return;  // (the whole workgroup: the grid is sized by the largest file)
    load_tables(stab, snat, image, fr);
    const uint32_t i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= fr.nsub) return;
    const uint8_t* stream = image + fr.stream_off;
    const uint64_t entry = i ? jpeg_sync_spec_entry(stream, fr.len, i * S) : jpeg_sync_pack(0, 0, 0);
    JpegSyncRecord r;
    jpeg_sync_speculate(stream, fr.len, sub_end(fr, i, S), entry, (const JpegHuffTable*)stab, snat, fr.geom, &r);
    spec[fr.rec_first + i] = r;
    cur[fr.rec_first + i] = r;
}

// Update round `round` (1 ..): every lane re-enters its subsequence from the exit its left neighbour had after the round
// before (`before`, read only) and writes `after`; jpeg_sync_update carries the record forward where the entry is the
// one it was computed from.  A changed record raises the file's last_changed to `round`; a file whose round - 1 changed
// nothing has converged, and its workgroups return at once (both buffers hold its records).
__global__ __launch_bounds__(kLanes) void jpeg_sync_round_kernel(const uint8_t* __restrict__ image, const SyncFrame* __restrict__ frames,
                                                                 int frame0, uint32_t S, uint32_t round, SyncWords* __restrict__ words,
                                                                 const JpegSyncRecord* __restrict__ spec,
                                                                 const JpegSyncRecord* __restrict__ before,
                                                                 JpegSyncRecord* __restrict__ after) {
    __shared__ __attribute__((aligned(16))) uint32_t stab[kJpegLaneTables * kTableDwords];
    __shared__ uint8_t snat[64];
    __shared__ uint32_t s_last;
    const int f = frame0 + blockIdx.y;
    const SyncFrame fr = frames[f];
    if (blockIdx.x * kLanes >= fr.nsub) return;
    if (threadIdx.x == 0) s_last = words[f].last_changed;  // (one load, so that the whole workgroup decides alike)
    __syncthreads();
    if (s_last + 1 < round) return;
    load_tables(stab, snat, image, fr);
    const uint32_t i = blockIdx.x * kLanes + threadIdx.x;
    bool changed = false;
    if (i < fr.nsub) {
        const uint32_t at = fr.rec_first + i;
        JpegSyncRecord r;
        if (i == 0) {
            r = before[at];
        } else {
            changed = jpeg_sync_update(image + fr.stream_off, fr.len, sub_end(fr, i, S), before[at - 1], before[at], spec[at],
                                       (const JpegHuffTable*)stab, snat, fr.geom, &r);
        }
        after[at] = r;
    }
    if (__any(changed) && (threadIdx.x & 63) == 0) atomicMax(&words[f].last_changed, round);
}

// The scan, one workgroup per file: the exclusive prefix of (blocks, DC sums) over the converged records gives every
// subsequence the index of its first block and its predictors, in 64-bit sums.  Thread j owns a run of consecutive
// records: it sums the run, thread 0 walks the 256 sums, every thread walks its run again.  Nothing behind the first
// record whose decode from the true entry failed is looked at (its blocks up to the failure count; the subsequences
// behind it get nothing to write).  kScanReached: the frame's block total is reached.  A file that has not converged
// within max_rounds gets kNotConverged and nothing else.
__global__ __launch_bounds__(kLanes) void jpeg_sync_scan_kernel(const SyncFrame* __restrict__ frames, int frame0, uint32_t max_rounds,
                                                                SyncWords* __restrict__ words, const JpegSyncRecord* __restrict__ buf0,
                                                                const JpegSyncRecord* __restrict__ buf1, JpegSyncStart* __restrict__ start) {
    __shared__ unsigned long long s_blocks[kLanes];
    __shared__ long long s_sum[3][kLanes];
    __shared__ uint32_t s_dead[kLanes];
    const int f = frame0 + blockIdx.x, t = threadIdx.x;
    const SyncFrame fr = frames[f];
    if (fr.nsub == 0) return;
    const uint32_t last = words[f].last_changed;  // (nothing writes it any more)
    if (last > max_rounds) {
        if (t == 0) words[f].flags = kNotConverged;
        return;
    }
    const JpegSyncRecord* rec = (((last + 1) & 1) ? buf1 : buf0) + fr.rec_first;  // what round last + 1 wrote
    const uint32_t per = (fr.nsub + kLanes - 1) / kLanes;
    const uint32_t lo = (uint32_t)t * per < fr.nsub ? (uint32_t)t * per : fr.nsub, hi = lo + per < fr.nsub ? lo + per : fr.nsub;
    unsigned long long cnt = 0;
    long long dc0 = 0, dc1 = 0, dc2 = 0;
    uint32_t dead = 0;
    for (uint32_t i = lo; i < hi && !dead; ++i) {
        const uint32_t b = rec[i].blocks;
        dead = b >> 31;
        cnt += dead ? (b >> 16) & 0x7FFFu : b & 0xFFFFu;
        dc0 += rec[i].dc[0];
        dc1 += rec[i].dc[1];
        dc2 += rec[i].dc[2];
    }
    s_blocks[t] = cnt;
    s_sum[0][t] = dc0;
    s_sum[1][t] = dc1;
    s_sum[2][t] = dc2;
    s_dead[t] = dead;
    __syncthreads();
    if (t == 0) {  // exclusive, in place; s_dead[j] becomes: a record in front of run j has failed
        unsigned long long c = 0;
        long long d0 = 0, d1 = 0, d2 = 0;
        uint32_t any = 0;
        for (int j = 0; j < kLanes; ++j) {
            const unsigned long long cj = s_blocks[j];
            const long long e0 = s_sum[0][j], e1 = s_sum[1][j], e2 = s_sum[2][j];
            const uint32_t dj = s_dead[j];
            s_blocks[j] = c;
            s_sum[0][j] = d0;
            s_sum[1][j] = d1;
            s_sum[2][j] = d2;
            s_dead[j] = any;
            c += cj;
            d0 += e0;
            d1 += e1;
            d2 += e2;
            any |= dj;
        }
    }
    __syncthreads();
    cnt = s_blocks[t];
    dc0 = s_sum[0][t];
    dc1 = s_sum[1][t];
    dc2 = s_sum[2][t];
    dead = s_dead[t];
    const long long lim = 1 << 30;  // (a predictor this far out has failed a lane in front already)
    for (uint32_t i = lo; i < hi; ++i) {
        JpegSyncStart st;
        st.first_block = dead || cnt > fr.total ? fr.total : (uint32_t)cnt;
        st.pred[0] = (int32_t)(dc0 < -lim ? -lim : dc0 > lim ? lim : dc0);
        st.pred[1] = (int32_t)(dc1 < -lim ? -lim : dc1 > lim ? lim : dc1);
        st.pred[2] = (int32_t)(dc2 < -lim ? -lim : dc2 > lim ? lim : dc2);
        start[fr.rec_first + i] = st;
        if (dead) continue;
        const uint32_t b = rec[i].blocks;
        dead = b >> 31;
        const uint32_t count = dead ? (b >> 16) & 0x7FFFu : b & 0xFFFFu;
        if (cnt < fr.total && cnt + count >= fr.total) atomicOr(&words[f].flags, kScanReached);
        cnt += count;
        dc0 += rec[i].dc[0];
        dc1 += rec[i].dc[1];
        dc2 += rec[i].dc[2];
    }
}

// The write pass.  Grid as round 0; a lane decodes its subsequence once more from its true entry and stores the non-zero
// luma coefficients into the file's zeroed area; DC values are stored absolute.  The lane that completes the frame's last
// block raises kReached, a lane that fails in front of it kError: the file is decoded iff kReached alone is up.
__global__ __launch_bounds__(kLanes) void jpeg_sync_write_kernel(const uint8_t* __restrict__ image, const SyncFrame* __restrict__ frames,
                                                                 int frame0, uint32_t S, SyncWords* __restrict__ words,
                                                                 const JpegSyncRecord* __restrict__ buf0,
                                                                 const JpegSyncRecord* __restrict__ buf1,
                                                                 const JpegSyncStart* __restrict__ start, int16_t* __restrict__ coef,
                                                                 long long coef_pitch) {
    __shared__ __attribute__((aligned(16))) uint32_t stab[kJpegLaneTables * kTableDwords];
    __shared__ uint8_t snat[64];
    __shared__ uint32_t s_flags;
    const int f = frame0 + blockIdx.y;
    const SyncFrame fr = frames[f];
    if (blockIdx.x * kLanes >= fr.nsub) return;
    if (threadIdx.x == 0) s_flags = words[f].flags;
    __syncthreads();
    if (!(s_flags & kScanReached)) return;  // not converged, or unreadable: the block total is never reached
    load_tables(stab, snat, image, fr);
    const uint32_t i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= fr.nsub) return;
    const JpegSyncStart st = start[fr.rec_first + i];
    if (st.first_block >= fr.total) return;
    const JpegSyncRecord* rec = (((words[f].last_changed + 1) & 1) ? buf1 : buf0) + fr.rec_first;
    const uint64_t entry = i ? rec[i - 1].exit : jpeg_sync_pack(0, 0, 0);
    int rc = 2;
    if (!(entry & kJpegSyncFailed)) {
        JpegSyncRecord unused;
        rc = jpeg_sync_lane<true>(image + fr.stream_off, fr.len, sub_end(fr, i, S), entry, (const JpegHuffTable*)stab, snat, fr.geom, st,
                                  fr.total, coef + (long long)fr.frame * coef_pitch, &unused);
    }
    if (rc) atomicOr(&words[f].flags, (uint32_t)rc);
}

}  // namespace

namespace mrg {

bool jpeg_sync_plan(const mrgingham_amd_ctx* ctx, const uint8_t* data, size_t nbytes, const JpegScan& sc, uint32_t* len) {
    if (!ctx->jpeg_sync || sc.restart_interval) return false;
    const size_t end = jpeg_segment_end(data, nbytes, sc.entropy_begin);
    if (end - sc.entropy_begin >= kJpegSyncMaxStream) return false;  // (an empty segment is taken: unreadable, as on the host)
    *len = (uint32_t)(end - sc.entropy_begin);
    return true;
}

int jpeg_sync_max_rounds(const mrgingham_amd_ctx* ctx) {
    return ctx->jpeg_sync_max_rounds > 0 ? ctx->jpeg_sync_max_rounds : 8192 / ctx->jpeg_sync_subsequence;
}

int jpeg_sync_lay_out(mrgingham_amd_ctx* ctx, int k, JpegSyncChunk* ch) {
    const uint32_t S = (uint32_t)ctx->jpeg_sync_subsequence;
    const size_t n = ch->files.size();
    ch->tables = n * sizeof(SyncFrame);
    size_t ntab = 0, nstream = 0;
    ch->nrecords = 0;
    ch->most = 0;
    for (JpegSyncFile& j : ch->files) {
        const JpegHuffTable* named[kJpegLaneTables] = {};
        JpegLaneGeom g;
        jpeg_lane_setup(*j.scan, named, &j.ntables, &g, 1, 1);
        j.table_off = ch->tables + ntab * sizeof(JpegHuffTable);
        j.nsub = (j.len + S - 1) / S;
        j.rec_first = ch->nrecords;
        j.stream_off = nstream;  // (from ch->streams, added below)
        ntab += (size_t)j.ntables;
        ch->nrecords += j.nsub;
        ch->most = std::max(ch->most, j.nsub);
        nstream += (((size_t)j.len + 3) & ~(size_t)3) + 4;
    }
    ch->streams = ch->tables + ntab * sizeof(JpegHuffTable);
    for (JpegSyncFile& j : ch->files) j.stream_off += ch->streams;
    ch->words = ch->streams + nstream;  // (on the host: where the words come back to)
    ch->total = ch->words + n * sizeof(SyncWords);
    if (ch->nrecords >= ((size_t)1 << 31)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "too many JPEG subsequences in one chunk");
    int rc;
    if ((rc = ensure_pinned(ctx, ctx->jpeg_sync_pin[k], ch->total, 4, false))) return rc;
    if ((rc = ensure(ctx, ctx->jpeg_sync_dev[k], ch->words))) return rc;
    // device only: words | spec | two record buffers | starts
    const size_t recs = ch->nrecords * sizeof(JpegSyncRecord);
    ch->d_spec = (n * sizeof(SyncWords) + 31) & ~(size_t)31;
    return ensure(ctx, ctx->jpeg_sync_rec[k], ch->d_spec + 3 * recs + ch->nrecords * sizeof(JpegSyncStart));
}

void jpeg_sync_fill(mrgingham_amd_ctx* ctx, int k, const JpegSyncChunk& ch, int i, int blocks_h, int pitch_blocks) {
    char* image = (char*)ctx->jpeg_sync_pin[k].p;
    const JpegSyncFile& j = ch.files[(size_t)i];
    const JpegScan& sc = *j.scan;
    SyncFrame fr;
    memset(&fr, 0, sizeof(fr));
    const JpegHuffTable* named[kJpegLaneTables] = {};
    int ntables = 0;
    jpeg_lane_setup(sc, named, &ntables, &fr.geom, blocks_h, pitch_blocks);
    fr.stream_off = j.stream_off;
    fr.table_off = (uint32_t)j.table_off;
    fr.rec_first = (uint32_t)j.rec_first;
    fr.nsub = j.nsub;
    fr.len = j.len;
    fr.total = (uint32_t)(sc.mcus_x * sc.mcus_y * sc.blocks_per_mcu);
    fr.ntables = (uint32_t)ntables;
    fr.frame = (uint32_t)j.frame;
    memcpy(image + (size_t)i * sizeof(SyncFrame), &fr, sizeof(fr));
    for (int s = 0; s < ntables; ++s) memcpy(image + j.table_off + (size_t)s * sizeof(JpegHuffTable), named[s], sizeof(JpegHuffTable));
    memcpy(image + j.stream_off, j.data + sc.entropy_begin, j.len);
    memset(image + j.stream_off + j.len, 0, ((((size_t)j.len + 3) & ~(size_t)3) + 4) - j.len);
}

int jpeg_sync_launch(mrgingham_amd_ctx* ctx, int k, const JpegSyncChunk& ch, int16_t* d_coef, int64_t coef_pitch, size_t area_elems,
                     hipStream_t s) {
    const int n = (int)ch.files.size();
    if (n == 0) return 0;
    char* pin = (char*)ctx->jpeg_sync_pin[k].p;
    char* dev = (char*)ctx->jpeg_sync_dev[k].p;
    char* scratch = (char*)ctx->jpeg_sync_rec[k].p;
    const uint32_t S = (uint32_t)ctx->jpeg_sync_subsequence, R = (uint32_t)jpeg_sync_max_rounds(ctx);
    SyncWords* words = (SyncWords*)scratch;
    JpegSyncRecord* spec = (JpegSyncRecord*)(scratch + ch.d_spec);
    JpegSyncRecord* buf[2] = {spec + ch.nrecords, spec + 2 * ch.nrecords};
    JpegSyncStart* start = (JpegSyncStart*)(spec + 3 * ch.nrecords);
    MRG_HIP_CHECK(hipMemcpyAsync(dev, pin, ch.words, hipMemcpyHostToDevice, s));
    MRG_HIP_CHECK(hipMemsetAsync(words, 0, (size_t)n * sizeof(SyncWords), s));
    for (const JpegSyncFile& j : ch.files)  // the lanes store non-zero coefficients only
        MRG_HIP_CHECK(hipMemsetAsync(d_coef + (size_t)j.frame * (size_t)coef_pitch, 0, area_elems * sizeof(int16_t), s));
    // kernel timing on: a pair of events around the launches (option "jpeg_sync_time_phase": around round 0, the update
    // rounds, the scan or the write pass alone), read by mrgingham_amd_chess_kernel_ms like the response's
    hipEvent_t mark[2] = {nullptr, nullptr};
    if (ctx->timing)
        for (hipEvent_t& e : mark)
            if (!(e = timing_event(ctx))) MRG_HIP_CHECK(hipGetLastError());  // (what kept it from being created)
    const int phase = ctx->jpeg_sync_time_phase;
    auto tick = [&](int boundary) -> hipError_t {  // boundary q lies between phase q and phase q + 1 (1 .. 4)
        if (!mark[0]) return hipSuccess;
        if (boundary == (phase ? phase - 1 : 0)) return hipEventRecord(mark[0], s);
        if (boundary == (phase ? phase : 4)) return hipEventRecord(mark[1], s);
        return hipSuccess;
    };
    MRG_HIP_CHECK(tick(0));
    const unsigned groups = std::max(1u, (unsigned)((ch.most + kLanes - 1) / kLanes));  // (a file may have no subsequence at all)
    const uint8_t* image = (const uint8_t*)dev;
    const SyncFrame* frames = (const SyncFrame*)dev;
    for (int f0 = 0; f0 < n; f0 += 65535)
        hipLaunchKernelGGL(jpeg_sync_spec_kernel, dim3(groups, (unsigned)std::min(n - f0, 65535)), dim3(kLanes), 0, s, image, frames, f0, S,
                           spec, buf[0]);
    MRG_HIP_CHECK(tick(1));
    for (uint32_t t = 1; t <= R + 1; ++t)
        for (int f0 = 0; f0 < n; f0 += 65535)
            hipLaunchKernelGGL(jpeg_sync_round_kernel, dim3(groups, (unsigned)std::min(n - f0, 65535)), dim3(kLanes), 0, s, image, frames, f0,
                               S, t, words, (const JpegSyncRecord*)spec, (const JpegSyncRecord*)buf[(t - 1) & 1], buf[t & 1]);
    MRG_HIP_CHECK(tick(2));
    for (int f0 = 0; f0 < n; f0 += 65535)
        hipLaunchKernelGGL(jpeg_sync_scan_kernel, dim3((unsigned)std::min(n - f0, 65535)), dim3(kLanes), 0, s, frames, f0, R, words,
                           (const JpegSyncRecord*)buf[0], (const JpegSyncRecord*)buf[1], start);
    MRG_HIP_CHECK(tick(3));
    for (int f0 = 0; f0 < n; f0 += 65535)
        hipLaunchKernelGGL(jpeg_sync_write_kernel, dim3(groups, (unsigned)std::min(n - f0, 65535)), dim3(kLanes), 0, s, image, frames, f0, S,
                           words, (const JpegSyncRecord*)buf[0], (const JpegSyncRecord*)buf[1], (const JpegSyncStart*)start, d_coef,
                           (long long)coef_pitch);
    MRG_HIP_CHECK(hipGetLastError());
    MRG_HIP_CHECK(tick(4));
    if (mark[0]) ctx->timing_events.pairs.emplace_back(mark[0], mark[1]);
    MRG_HIP_CHECK(hipMemcpyAsync(pin + ch.words, words, (size_t)n * sizeof(SyncWords), hipMemcpyDeviceToHost, s));
    return 0;
}

int32_t jpeg_sync_status(const mrgingham_amd_ctx* ctx, int k, const JpegSyncChunk& ch, int i, int* rounds) {
    const SyncWords w = ((const SyncWords*)((const char*)ctx->jpeg_sync_pin[k].p + ch.words))[i];
    if (rounds) *rounds = (int)w.last_changed;
    if (w.flags & kNotConverged) return -3;
    return (w.flags & kScanReached) && (w.flags & kReached) && !(w.flags & kError) ? 0 : -1;
}

}  // namespace mrg

extern "C" {

int mrgingham_amd_jpeg_sync_rounds(const uint8_t* data, size_t nbytes, int subsequence_bytes, int* rounds, size_t* nsubsequences) {
    if (rounds) *rounds = 0;
    if (nsubsequences) *nsubsequences = 0;
    if (!data) return -1;
    try {
        JpegInfo info;
        if (jpeg_coefficients(data, nbytes, nullptr, 0, 0, &info)) return -1;
        std::vector<int16_t> coef((size_t)info.blocks_w * info.blocks_h * 64);
        JpegSyncState st;
        int rc = jpeg_sync_begin(data, nbytes, subsequence_bytes, &st);
        if (rc == -3 || rc == -4) return jpeg_coefficients(data, nbytes, coef.data(), coef.size(), 0, &info) == 0 ? rc : -1;
        if (rc) return -1;
        int t = 0;
        while (jpeg_sync_round(&st)) ++t;  // (at most one round per subsequence: see jpeg.h)
        if (jpeg_sync_finish(st, coef.data(), coef.size(), 0)) return -1;
        if (rounds) *rounds = t;
        if (nsubsequences) *nsubsequences = st.nsub;
        return 0;
    } catch (...) {
        return -1;
    }
}

}  // extern "C"
