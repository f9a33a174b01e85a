// Baseline JPEG on the device, the entropy half for files WITHOUT restart markers: the entropy-coded segment is cut into
// subsequences of S raw bytes, one lane each, that decode from a guessed state and are then re-entered from their left
// neighbour's exit until nothing changes -- jpeg_huff_sync.h, the text the host runs under the sanitizers, has the
// decoder, DESIGN.md section 4.10 the method and the measured figures, include/mrgingham_amd.h the options "jpeg_sync",
// "jpeg_sync_subsequence" and "jpeg_sync_max_rounds".  Four kernels, all plain launches that the stream orders: round 0,
// R + 1 update rounds (a file that has converged costs its workgroups one load), the scan, the write pass.  No kernel
// waits for another workgroup.  The staging image the kernels read is built by jpeg_stage.h; here are the kernels and what
// grows the buffers, queues a filled image and reads the per-file words.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "jpeg_huff_sync.h"
#include "jpeg_stage.h"

using namespace mrg;

namespace {

constexpr int kLanes = 256;
constexpr int kTableDwords = (int)(sizeof(JpegHuffTable) / 4);

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

int jpeg_sync_grow(mrgingham_amd_ctx* ctx, int k, const JpegSyncLayout& l) {
    if (l.nfiles == 0) return 0;
    if (l.nitems >= ((size_t)1 << 31)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "too many JPEG subsequences in one chunk");
    int rc;
    if ((rc = ensure_pinned(ctx, ctx->jpeg_sync_pin[k], l.total, 4, false))) return rc;
    if ((rc = ensure(ctx, ctx->jpeg_sync_dev[k], l.back))) return rc;
    return ensure(ctx, ctx->jpeg_sync_rec[k], l.d_bytes);
}

int jpeg_sync_launch(mrgingham_amd_ctx* ctx, int k, const JpegSyncLayout& l, const JpegStageFile* files, int nfiles, int16_t* d_coef,
                     int64_t coef_pitch, size_t area_elems, hipStream_t s) {
    const int n = l.nfiles;
    if (n == 0) return 0;
    char* pin = (char*)ctx->jpeg_sync_pin[k].p;
    char* dev = (char*)ctx->jpeg_sync_dev[k].p;
    char* scratch = (char*)ctx->jpeg_sync_rec[k].p;
    const uint32_t S = (uint32_t)ctx->jpeg_sync_subsequence;
    const uint32_t R = (uint32_t)(ctx->jpeg_sync_max_rounds > 0 ? ctx->jpeg_sync_max_rounds : 8192 / ctx->jpeg_sync_subsequence);
    SyncWords* words = (SyncWords*)scratch;
    JpegSyncRecord* spec = (JpegSyncRecord*)(scratch + l.d_spec);
    JpegSyncRecord* buf[2] = {spec + l.nitems, spec + 2 * l.nitems};
    JpegSyncStart* start = (JpegSyncStart*)(spec + 3 * l.nitems);
    MRG_HIP_CHECK(hipMemcpyAsync(dev, pin, l.back, hipMemcpyHostToDevice, s));
    MRG_HIP_CHECK(hipMemsetAsync(words, 0, (size_t)n * sizeof(SyncWords), s));
    for (int i = 0; i < nfiles; ++i)  // the lanes store non-zero coefficients only
        if (files[i].route == JpegRoute::kSync)
            MRG_HIP_CHECK(hipMemsetAsync(d_coef + (size_t)i * (size_t)coef_pitch, 0, area_elems * sizeof(int16_t), s));
    // kernel timing: boundary q lies between phase q and phase q + 1 of round 0, the update rounds, the scan, the write
    // pass; option "jpeg_sync_time_phase" brackets one of them alone
    const int phase = ctx->jpeg_sync_time_phase;
    TimingBracket mark;
    MRG_HIP_CHECK(mark.begin(ctx, phase ? phase - 1 : 0, phase ? phase : 4));
    MRG_HIP_CHECK(mark.tick(ctx, 0, s));
    const unsigned groups = std::max(1u, (unsigned)((l.most_items + kLanes - 1) / kLanes));  // (a file may have no subsequence at all)
    const uint8_t* image = (const uint8_t*)dev;
    const SyncFrame* frames = (const SyncFrame*)dev;
    for_frame_slabs(n, [&](int f0, unsigned nf) {
        hipLaunchKernelGGL(jpeg_sync_spec_kernel, dim3(groups, nf), dim3(kLanes), 0, s, image, frames, f0, S, spec, buf[0]);
    });
    MRG_HIP_CHECK(mark.tick(ctx, 1, s));
    for (uint32_t t = 1; t <= R + 1; ++t)
        for_frame_slabs(n, [&](int f0, unsigned nf) {
            hipLaunchKernelGGL(jpeg_sync_round_kernel, dim3(groups, nf), dim3(kLanes), 0, s, image, frames, f0, S, t, words,
                               (const JpegSyncRecord*)spec, (const JpegSyncRecord*)buf[(t - 1) & 1], buf[t & 1]);
        });
    MRG_HIP_CHECK(mark.tick(ctx, 2, s));
    for_frame_slabs(n, [&](int f0, unsigned nf) {
        hipLaunchKernelGGL(jpeg_sync_scan_kernel, dim3(nf), dim3(kLanes), 0, s, frames, f0, R, words, (const JpegSyncRecord*)buf[0],
                           (const JpegSyncRecord*)buf[1], start);
    });
    MRG_HIP_CHECK(mark.tick(ctx, 3, s));
    for_frame_slabs(n, [&](int f0, unsigned nf) {
        hipLaunchKernelGGL(jpeg_sync_write_kernel, dim3(groups, nf), dim3(kLanes), 0, s, image, frames, f0, S, words,
                           (const JpegSyncRecord*)buf[0], (const JpegSyncRecord*)buf[1], (const JpegSyncStart*)start, d_coef,
                           (long long)coef_pitch);
    });
    MRG_HIP_CHECK(hipGetLastError());
    MRG_HIP_CHECK(mark.tick(ctx, 4, s));
    MRG_HIP_CHECK(hipMemcpyAsync(pin + l.back, words, (size_t)n * sizeof(SyncWords), hipMemcpyDeviceToHost, s));
    return 0;
}

int32_t jpeg_sync_status(const mrgingham_amd_ctx* ctx, int k, const JpegSyncLayout& l, int i) {
    const SyncWords w = ((const SyncWords*)((const char*)ctx->jpeg_sync_pin[k].p + l.back))[i];
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
