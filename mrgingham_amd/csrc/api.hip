// Host side of libmrgingham_amd.so, the context itself: its lifetime and options, the kernel-timing read-out, the scratch
// sets and status words, sync and the stream hand-offs, and the pixel-only _batch entry points (response, level images,
// blur, preprocessing).  chain.hip (what the detector puts on the streams), multi.hip, reference.hip, boards.hip and
// blobs_api.hip hold the rest of the host side (ctx.h).
// See include/mrgingham_amd.h for the contract of every entry point.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ctx.h"

namespace mrg {

int fail(mrgingham_amd_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    fprintf(stderr, "mrgingham_amd: %s\n", buf);
    return code;
}

int fail_hip(mrgingham_amd_ctx* ctx, hipError_t e, const char* what, const char* file, int line) {
    return fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "%s:%d: %s failed: %s", file, line, what, hipGetErrorString(e));
}

int scratch_fill_from_env() {
    const char* e = getenv("MRGINGHAM_AMD_SCRATCH_FILL");
    if (!e || !*e) return -1;
    char* end = nullptr;
    const long v = strtol(e, &end, 0);
    return (end == e || *end || v < 0 || v > 255) ? -1 : (int)v;
}

int ensure(mrgingham_amd_ctx* ctx, DevBuf& b, size_t bytes) {
    if (bytes <= b.bytes) return 0;
    if (b.p) {
        MRG_HIP_CHECK(hipDeviceSynchronize());
        MRG_HIP_CHECK(hipFree(b.p));
        ctx->scratch_total -= (long long)b.bytes;
        b.p = nullptr;
        b.bytes = 0;
    }
    // growth headroom for the small buffers only: the per-level tables of a large batch are gigabytes, and 1/8 on top
    // of them was 1 GiB of the 64-frame bench's scratch
    const size_t want = bytes + (bytes < (64u << 20) ? bytes / 8 : 0) + 256;
    MRG_HIP_CHECK(hipMalloc(&b.p, want));
    b.bytes = want;
    ctx->scratch_total += (long long)want;
    // (what set_option "scratch_fill_now" walks: a buffer is noted once, its address is a member's)
    bool noted = false;
    for (const DevBuf* q : ctx->scratch_bufs) noted = noted || q == &b;
    if (!noted) ctx->scratch_bufs.push_back(&b);
    if (ctx->scratch_fill >= 0) {  // (complete before whatever the caller queues on the context's streams, which do not wait for the null stream)
        MRG_HIP_CHECK(hipMemset(b.p, ctx->scratch_fill, want));
        MRG_HIP_CHECK(hipDeviceSynchronize());
    }
    return 0;
}

void release(mrgingham_amd_ctx* ctx, DevBuf& b) {
    if (!b.p) return;
    (void)hipFree(b.p);
    ctx->scratch_total -= (long long)b.bytes;
    b.p = nullptr;
    b.bytes = 0;
}

// (the step of ensure_pinned, for the one caller that goes on without the memory: ensure_level_set)
static hipError_t grow_pinned(mrgingham_amd_ctx* ctx, PinBuf& b, size_t bytes, int slack_divisor, bool zero_on_growth) {
    if (bytes <= b.bytes) return hipSuccess;
    if (b.p) {
        const hipError_t e = hipHostFree(b.p);
        if (e != hipSuccess) return e;
        b.p = nullptr;
        b.bytes = 0;
    }
    const size_t want = bytes + (slack_divisor ? bytes / slack_divisor : 0);
    const hipError_t e = hipHostMalloc(&b.p, want, hipHostMallocDefault);
    if (e != hipSuccess) {
        b.p = nullptr;
        return e;
    }
    b.bytes = want;
    bool noted = false;
    for (const PinBuf* q : ctx->pinned_bufs) noted = noted || q == &b;
    if (!noted) ctx->pinned_bufs.push_back(&b);
    if (ctx->scratch_fill >= 0) memset(b.p, ctx->scratch_fill, want);
    else if (zero_on_growth) memset(b.p, 0, want);
    return hipSuccess;
}

int ensure_pinned(mrgingham_amd_ctx* ctx, PinBuf& b, size_t bytes, int slack_divisor, bool zero_on_growth) {
    MRG_HIP_CHECK(grow_pinned(ctx, b, bytes, slack_divisor, zero_on_growth));
    return 0;
}

// Rows between host and device (or device and device): ONE plain copy whenever both sides are dense (every caller's usual case).  The 2-D copy
// of the runtime is a slow path into pageable memory and serialises the threads of a process.
hipError_t copy_rows_async(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes, size_t rows,
                           hipMemcpyKind kind, hipStream_t s) {
    if (dpitch == width_bytes && spitch == width_bytes) return hipMemcpyAsync(dst, src, width_bytes * rows, kind, s);
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, width_bytes, rows, kind, s);
}

int level_dims(int W, int H, int level, int* w, int* h) {
    if (level < 0 || level > kMaxLevel) return -1;  // find_chessboard_corners.cc:433-441
    auto rnd = [level](int v) {                     // cvRound(v / 2^level): ties to even
        const int s = 1 << level;
        int q = v >> level;
        const int rem = v & (s - 1), half = s >> 1;
        if (level > 0 && (rem > half || (rem == half && (q & 1)))) ++q;
        return q;
    };
    *w = rnd(W);
    *h = rnd(H);
    return 0;
}

int validate_frames(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* f) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (!f || (!f->frames && f->nframes > 0) || f->nframes < 0 || f->width < 0 || f->height < 0 ||
        f->stride < f->width)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad frame batch descriptor");
    if (f->width > 32767 || f->height > 32767)  // int16 coordinates, find_chessboard_corners.cc:91
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "frames larger than 32767 pixels per side are not supported");
    return 0;
}

// Scratch of level `level` for a batch of nframes W x H frames and up to `pitch` points per frame.
int ensure_level_set(mrgingham_amd_ctx* ctx, int set, int level, int nframes, int W, int H, int pitch) {
    LevelScratch& L = ctx->lvs[set][level];
    int w, h;
    level_dims(W, H, level, &w, &h);
    const int shift = ctx->cap_shift < ctx->grown_shift[level] ? ctx->cap_shift : ctx->grown_shift[level];
    if (nframes <= L.nframes && w == L.w && h == L.h && pitch <= L.pitch && L.shift == shift) return 0;
    if (w == L.w && h == L.h) {
        nframes = nframes > L.nframes ? nframes : L.nframes;
        pitch = pitch > L.pitch ? pitch : L.pitch;
    }
    const long long px = (long long)w * h;
    long long cap = px >> shift;
    if (cap < 4096) cap = 4096;
    if (cap > px) cap = px > 0 ? px : 1;
    if (cap > 0x3fffffff) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "frame too large");
    // Components that pass the size / peak / margin tests: at most cap / 2 (two pixels each).  Tables of
    // that size are only allocated at shift 0 (the "one entry per pixel" retry of the reference-symbol
    // wrappers); otherwise a fraction, with overflow reported like a hot-list overflow.
    long long cand_cap = shift == 0 ? cap / 2 + 1 : cap / 16 + 1024;
    if (cand_cap < pitch) cand_cap = pitch;
    long long sort_cap = 1;
    while (sort_cap < cand_cap) sort_cap <<= 1;
    // LIFO arena: a super-component of n hot pixels gets 4n + 1 words (every pixel is pushed at most
    // once per neighbour), so 5 * cap bounds a frame.  Same policy as the candidate table.
    const long long arena_cap = (shift == 0 ? 5 * cap : cap + cap / 4) + 16LL * (pitch > 1024 ? pitch : 1024);
    const size_t nf = (size_t)nframes;
    int rc = 0;
    if (level > 0 && (rc = ensure(ctx, L.img, nf * (size_t)px + 16))) return rc;
    if ((rc = ensure(ctx, L.resp, nf * (size_t)px * 2 + 16))) return rc;
    if ((rc = ensure(ctx, L.gidx, nf * (size_t)((w + 7) / 8) * h * 8 + 16))) return rc;
    if (nframes > ctx->counters_nf) {
        MRG_HIP_CHECK(hipDeviceSynchronize());
        const int cnf = nframes + nframes / 8 + 8;
        for (int k = 0; k < kMaxSets; ++k) {
            if ((rc = ensure(ctx, ctx->counters2[k], (size_t)(kMaxLevel + 1) * 3 * cnf * 4))) return rc;
            MRG_HIP_CHECK(hipMemset(ctx->counters2[k].p, 0, ctx->counters2[k].bytes));
            ctx->status_copied[k] = false;  // (the layout of the words changes with counters_nf)
        }
        // the page-locked mirrors of the status words (end_op copies into them) change size with it: here, where the
        // device is idle and nothing is queued.  A mirror that cannot be had stays away until the next growth (the sync
        // then makes a blocking copy: harvest_set)
        for (int k = 0; k < kMaxSets; ++k)
            if (grow_pinned(ctx, ctx->status_pin[k], (size_t)(kMaxLevel + 1) * cnf * sizeof(int32_t), 0, false) != hipSuccess) (void)hipGetLastError();
        ctx->counters_nf = cnf;
    }
    if ((rc = ensure(ctx, L.hot_xy, nf * (size_t)cap * 4))) return rc;
    if ((rc = ensure(ctx, L.parent, nf * (size_t)cap * 4))) return rc;
    if ((rc = ensure(ctx, L.comp_cnt, nf * (size_t)cap * 4))) return rc;
    if ((rc = ensure(ctx, L.roots, nf * (size_t)cap * 4))) return rc;
    if ((rc = ensure(ctx, L.comp_first, nf * (size_t)cap * 4))) return rc;
    if ((rc = ensure(ctx, L.comp_box, nf * (size_t)cap * 16))) return rc;
    if ((rc = ensure(ctx, L.arena, nf * (size_t)arena_cap * 4))) return rc;
    if ((rc = ensure(ctx, L.cand, nf * (size_t)cand_cap * sizeof(Cand)))) return rc;
    if ((rc = ensure(ctx, L.sortkeys, nf * (size_t)sort_cap * 8))) return rc;
    L.w = w; L.h = h; L.nframes = nframes; L.pitch = pitch;
    L.cap = (int)cap; L.cand_cap = (int)cand_cap; L.sort_cap = (int)sort_cap; L.arena_cap = arena_cap;
    L.shift = shift;
    return 0;
}

// How many scratch sets (= calls whose component searches may be in flight) this batch shape gets, unless the
// option "scratch_sets" fixed it: three while three sets of the whole chain's scratch stay below 8 GB (small
// frames, whose search chain is much longer than their pixel kernels: 64 x 640x480 chains 280 k -> 399 k
// frames/s), two otherwise (64 x 4096x3072: no gain from a third, 9.9 GiB each).  A change of the rotation waits
// for everything in flight first.
int choose_sets(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr) {
    if (ctx->nsets_fixed) return 0;
    const double per_set = 5.0 * (double)fr->nframes * fr->width * fr->height;  // bytes; measured 4.9 per frame pixel at the default table size
    if (per_set > ctx->max_set_bytes) ctx->max_set_bytes = per_set;  // the largest batch so far decides (scratch only grows)
    // (a context that has run sparse chains keeps three sets up to 16 GB: their component chain is what limits a step,
    // (pixel kernels + chain) / sets -- 64 x 4096x3072: 0.47 -> 0.39 ms per step for 11 instead of 7.3 GiB.  Sticky, so
    // that a dense repeat of one call does not free and reallocate a set.)
    const int want = 3.0 * ctx->max_set_bytes <= (ctx->sparse_seen ? 16e9 : 8e9) ? 3 : 2;
    if (want == ctx->nsets) return 0;
    const int rc = mrgingham_amd_sync(ctx);
    if (want < ctx->nsets)  // the sets that leave the rotation give their scratch back (a larger batch has arrived)
        for (int set = want; set < ctx->nsets; ++set)
            for (LevelScratch& L : ctx->lvs[set]) {  // (the small per-point scratch stays: it is sized for all sets)
                L.for_each_buffer([ctx](DevBuf& b) { release(ctx, b); });
                L.nframes = 0; L.w = L.h = 0; L.pitch = 0;
            }
    ctx->nsets = want;
    ctx->cur = 0;
    return rc;
}

int ensure_level(mrgingham_amd_ctx* ctx, int level, int nframes, int W, int H, int pitch) {
    int rc = 0;
    for (int set = 0; !rc && set < ctx->nsets; ++set) rc = ensure_level_set(ctx, set, level, nframes, W, H, pitch);
    return rc;
}

// Per-call point scratch shared by the levels (the component kernels of the levels of one call
// run one after the other on that call's component stream); one copy per scratch set.
int ensure_points(mrgingham_amd_ctx* ctx, int nframes, int pitch) {
    if (nframes <= ctx->pts_nframes && pitch <= ctx->pts_pitch) return 0;
    nframes = nframes > ctx->pts_nframes ? nframes : ctx->pts_nframes;
    pitch = pitch > ctx->pts_pitch ? pitch : ctx->pts_pitch;
    const size_t np = (size_t)nframes * (size_t)(pitch > 0 ? pitch : 1);
    int rc = 0;
    for (auto& ps : ctx->pts) {
        if ((rc = ensure(ctx, ps.leader, np * 4))) return rc;
        if ((rc = ensure(ctx, ps.need, np * 4))) return rc;
        if ((rc = ensure(ctx, ps.nseeds, np * 4))) return rc;
        if ((rc = ensure(ctx, ps.seeds, np * 9 * 4))) return rc;
        if ((rc = ensure(ctx, ps.sroot, np * 9 * 4))) return rc;
        if ((rc = ensure(ctx, ps.cand_xy, np * 8))) return rc;
        if ((rc = ensure(ctx, ps.cand_counts, (size_t)nframes * 4))) return rc;
        // sparse refinement: at most 4 cells per seed position of a point and 9 of those, of which at most 9 distinct
        if ((rc = ensure(ctx, ps.cell_list, 2 * np * kCellsPerPoint * 4))) return rc;  // two buffers: consecutive levels alternate
        if ((rc = ensure(ctx, ps.cell_cnt, (size_t)nframes * 4 * kCellHdr * (kMaxLevel + 1)))) return rc;  // per level and frame: the list's header
        if ((rc = ensure(ctx, ps.flag_list, ((size_t)nframes + 1) * 4))) return rc;  // the frames a sparse chain reported
    }
    ctx->pts_nframes = nframes;
    ctx->pts_pitch = pitch;
    return 0;
}

// The status words of one (scratch set, level) as the host has them (`host`: nact words), inspected; `words` = where they
// live on the device: cleared when any is set.  A table overflow grows the tables of the level to what the fullest frame
// asked for.  *rc keeps the first error.  Nothing of that set may be running at that level.
static int inspect_status(mrgingham_amd_ctx* ctx, int set, int level, const int32_t* host, int nact, int32_t* words, int* rc,
                          bool quiet) {
    // every pending status block is inspected and cleared; only the first error is reported
    bool dirty = false;
    int flags = 0, first = -1;
    long long need = 0;  // hot pixels the fullest frame asked for (status words carry it in units of 64)
    for (int f = 0; f < nact; ++f) {
        const int st = host[f];
        if (!st) continue;
        dirty = true;
        if (first < 0) first = f;
        flags |= st & 0xff;
        const long long n = (long long)((uint32_t)st >> 8) * 64;
        if (n > need) need = n;
    }
    if (!dirty) return 0;
    if ((flags & kStatusSparse) && !(flags & (kStatusHotOverflow | kStatusCandOverflow))) {
        // cannot happen: the dense repeat behind every sparse refinement clears the flag (queue_sparse_levels)
        if (*rc == MRGINGHAM_AMD_OK)
            *rc = fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "internal: frame %d, level %d left a sparse-refinement flag behind", first, level);
    } else {
        // grow the tables of this level to what was asked for (+25 %); candidate / LIFO overflow: four times
        const LevelScratch& LS = ctx->lvs[set][level];
        const long long px = (long long)LS.w * LS.h;
        int sh = LS.shift;
        if (flags & kStatusHotOverflow)
            while (sh > 0 && (px >> sh) < need + need / 4) --sh;
        if (flags & kStatusCandOverflow) sh = sh >= 2 ? (sh - 2 < LS.shift - 2 ? sh - 2 : LS.shift - 2) : 0;
        if (sh < 0) sh = 0;
        if (sh < ctx->grown_shift[level]) ctx->grown_shift[level] = sh;
        if (quiet) *rc = MRGINGHAM_AMD_ERR_CAPACITY;  // (the caller has dealt with the frames; the tables grow for the next batch)
        else if (*rc == MRGINGHAM_AMD_OK)
            *rc = fail(ctx, MRGINGHAM_AMD_ERR_CAPACITY,
                       "frame %d, level %d: component tables overflowed (status %d, %lld hot pixels asked for); "
                       "the tables of this level grow from 1/%d to 1/%d of its pixels: make the call again",
                       first, level, flags, need, 1 << LS.shift, 1 << sh);
    }
    MRG_HIP_CHECK(hipMemset(words, 0, sizeof(int32_t) * nact));
    return 0;
}

static int32_t* status_words(mrgingham_amd_ctx* ctx, int set, int level) {
    const int saved = ctx->cur;
    ctx->cur = set;
    int32_t* const words = status_of(ctx, level);
    ctx->cur = saved;
    return words;
}

// one (scratch set, level): its words copied, inspected, cleared
int harvest_status(mrgingham_amd_ctx* ctx, int set, int level, int* rc, bool quiet) {
    const int nact = ctx->pending_frames[set][level];
    ctx->pending_frames[set][level] = 0;
    if (nact <= 0 || !ctx->counters2[set].p) return 0;
    int32_t* const words = status_words(ctx, set, level);
    ctx->host_status.resize(nact);
    MRG_HIP_CHECK(hipMemcpy(ctx->host_status.data(), words, sizeof(int32_t) * nact, hipMemcpyDeviceToHost));
    return inspect_status(ctx, set, level, ctx->host_status.data(), nact, words, rc, quiet);
}

// every level of a scratch set: the levels' status words are one block of the set's counter buffer, so ONE copy brings all
// of them (a blocking 256-byte copy costs 15-30 us: a chain call's sync made four of them, a sync behind pipelined chain
// calls up to eight)
static int harvest_set(mrgingham_amd_ctx* ctx, int set, int* rc) {
    int lo = -1, hi = -1;
    for (int level = 0; level <= kMaxLevel; ++level)
        if (ctx->pending_frames[set][level] > 0) {
            if (lo < 0) lo = level;
            hi = level;
        }
    if (lo < 0 || !ctx->counters2[set].p) {
        for (int level = 0; level <= kMaxLevel; ++level) ctx->pending_frames[set][level] = 0;
        return 0;
    }
    const size_t cnf = (size_t)ctx->counters_nf, nwords = (size_t)(hi - lo + 1) * cnf;
    const int32_t* host;
    const bool pinned = ctx->status_copied[set];  // (end_op's copy: the whole block, sized by counters_nf like the words)
    if (pinned) {  // (the set's stream has been waited for: the copy end_op queued has landed)
        host = (const int32_t*)ctx->status_pin[set].p + (size_t)lo * cnf;
    } else {
        ctx->host_status.resize(nwords);
        MRG_HIP_CHECK(hipMemcpy(ctx->host_status.data(), status_words(ctx, set, lo), sizeof(int32_t) * nwords, hipMemcpyDeviceToHost));
        host = ctx->host_status.data();
    }
    for (int level = lo; level <= hi; ++level) {
        const int nact = ctx->pending_frames[set][level];
        ctx->pending_frames[set][level] = 0;
        if (nact <= 0) continue;
        const int32_t* hw = host + (size_t)(level - lo) * cnf;
        bool any = false;
        for (int f = 0; f < nact && !any; ++f) any = hw[f] != 0;
        const int r = inspect_status(ctx, set, level, hw, nact, status_words(ctx, set, level), rc, false);
        if (r) return r;
        if (any && pinned) memset((int32_t*)ctx->status_pin[set].p + (size_t)level * cnf, 0, (size_t)nact * sizeof(int32_t));  // (cleared on the device: here too)
    }
    return 0;
}

// One level image (level >= 1) of the batch into `out` (dense, frames back to back): levels 1..3 through the
// one-pass pyramid kernel restricted to that level (16 x 8 source blocks per thread, 16-byte loads; the
// per-pixel kernel took 425 us for level 1 of 64 frames of 4096x3072, this one reads the frames at HBM speed),
// which falls back to the per-pixel kernels itself for ragged shapes.
void launch_one_level_image(const mrgingham_amd_frames* fr, int level, uint8_t* out, int w, int h, hipStream_t s) {
    const FrameBatch fb{fr->frames, fr->frame_pitch, fr->width, fr->height, fr->stride};
    if (level <= 3) {
        PyramidOut po{};
        po.out[level - 1] = out;
        po.w[level - 1] = w;
        po.h[level - 1] = h;
        launch_pyramid(fb, po, level, fr->nframes, s);
    } else {
        launch_decimate(fb, level, out, (long long)w * h, w, h, 0, fr->nframes, s);
    }
}

}  // namespace mrg

using namespace mrg;

extern "C" {

int mrgingham_amd_abi_version(void) { return MRGINGHAM_AMD_ABI_VERSION; }

#ifndef MRG_KERNEL_ID
#define MRG_KERNEL_ID "unknown"
#endif
const char* mrgingham_amd_kernel_id(void) { return MRG_KERNEL_ID; }

int mrgingham_amd_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int mrgingham_amd_level_dims(int width, int height, int level, int* w, int* h) {
    if (!w || !h || width < 0 || height < 0) return MRGINGHAM_AMD_ERR_ARG;
    return level_dims(width, height, level, w, h) == 0 ? MRGINGHAM_AMD_OK : MRGINGHAM_AMD_ERR_ARG;
}

mrgingham_amd_ctx* mrgingham_amd_create(int device_ordinal) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        fprintf(stderr, "mrgingham_amd: no usable HIP device (%s); this library has no CPU path\n",
                e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        return nullptr;
    }
    if (device_ordinal < 0 || device_ordinal >= ndev) {
        fprintf(stderr, "mrgingham_amd: device ordinal %d out of range (0..%d)\n", device_ordinal, ndev - 1);
        return nullptr;
    }
    if (hipSetDevice(device_ordinal) != hipSuccess) return nullptr;
    mrgingham_amd_ctx* ctx = new mrgingham_amd_ctx();
    ctx->device = device_ordinal;
    for (int& g : ctx->grown_shift) g = 31;
    ctx->scratch_fill = scratch_fill_from_env();  // (test hook, ctx.h: off unless the variable holds a byte)
#ifdef MRG_EXPERIMENT
    const char* v0 = getenv("MRGINGHAM_AMD_CHESS_V0");
    ctx->use_v0 = v0 && atoi(v0) != 0;
#endif
    int prio_lo = 0, prio_hi = 0;  // the component stream gets the highest dispatch priority
    hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    // Experiment hooks (tools/interference_ab.py): MRGINGHAM_AMD_CC_CUS = k confines the component
    // streams to k CUs per XCD (CU-mask bit i is XCD i % 8, CU i / 8: probed with
    // tools/ubench/cu_mask.hip); MRGINGHAM_AMD_PIX_COMPLEMENT = 1 keeps the pixel stream off them.
    // (only in -DMRG_EXPERIMENT builds: the shipped library reads no environment variable but MRGINGHAM_AMD_DEVICE and the
    // test hook MRGINGHAM_AMD_SCRATCH_FILL)
#ifdef MRG_EXPERIMENT
    const char* ecc = getenv("MRGINGHAM_AMD_CC_CUS");
    const int cc_cus = ecc ? atoi(ecc) : 0;
    const char* epx = getenv("MRGINGHAM_AMD_PIX_COMPLEMENT");
    const bool pix_compl = epx && atoi(epx) != 0;
#else
    const int cc_cus = 0;
    const bool pix_compl = false;
#endif
    bool ok = true;
    if (cc_cus > 0 && cc_cus < 32) {
        uint32_t mask[8] = {}, inv[8];
        for (int b = 0; b < 8 * cc_cus; ++b) mask[b >> 5] |= 1u << (b & 31);
        for (int i = 0; i < 8; ++i) inv[i] = ~mask[i];
        for (int k = 0; ok && k < kMaxSets; ++k) ok = hipExtStreamCreateWithCUMask(&ctx->ccs[k].h, 8, mask) == hipSuccess;
        ok = ok &&
             (pix_compl ? hipExtStreamCreateWithCUMask(&ctx->pix.h, 8, inv)
                        : hipStreamCreateWithPriority(&ctx->pix.h, hipStreamNonBlocking, prio_lo)) == hipSuccess;
    } else {
        ok = hipStreamCreateWithPriority(&ctx->pix.h, hipStreamNonBlocking, prio_lo) == hipSuccess;
        for (int k = 0; ok && k < kMaxSets; ++k)
            ok = hipStreamCreateWithPriority(&ctx->ccs[k].h, hipStreamNonBlocking, prio_hi) == hipSuccess;
    }
    for (int k = 0; ok && k < kMaxSets; ++k) ok = ctx->ev_cc_done[k].create(hipEventDisableTiming) == hipSuccess;
    for (int i = 0; ok && i <= kMaxLevel; ++i) ok = ctx->ev_pix[i].create(hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        fprintf(stderr, "mrgingham_amd: could not create HIP streams/events\n");
        mrgingham_amd_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

void mrgingham_amd_destroy(mrgingham_amd_ctx* ctx) {
    if (!ctx) return;
#ifdef MRG_EXPERIMENT
    if (ctx->fb_prof_n > 0 && getenv("MRG_DBG_FB")) {
        static const char* names[10] = {"submit: checks + scratch", "submit: host part begins (big frames, threads start)", "submit: device passes queued",
                                        "host part: grid finder joined", "host part: refinement queued", "collect: wait for the refinement",
                                        "collect: boards copied", "", "", ""};
        for (int i = 0; i < 7; ++i) fprintf(stderr, "  [fb] %-56s %8.3f ms per batch\n", names[i], ctx->fb_prof[i] / ctx->fb_prof_n);
    }
#endif
    for (auto& j : ctx->jobs)  // batches still in flight are abandoned: only their host threads have to be out
        if (j.grid_running) {
            ctx->pool.wait();
            j.grid_running = false;
        }
    if (ctx->one) mrgingham_amd_destroy(ctx->one);
    hipSetDevice(ctx->device);
    hipDeviceSynchronize();
    delete ctx;  // (every buffer, event and stream of the context is a member that frees itself: ctx.h, OWNERS)
}

int mrgingham_amd_debug_paths(mrgingham_amd_ctx* ctx, int level, int nframes, int32_t* h_paths) {
    if (!ctx || !h_paths || level < 0 || level > kMaxLevel || nframes < 0 || nframes > ctx->counters_nf)
        return MRGINGHAM_AMD_ERR_ARG;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    MRG_HIP_CHECK(hipDeviceSynchronize());
    MRG_HIP_CHECK(hipMemcpy(h_paths, path_of(ctx, level), sizeof(int32_t) * (size_t)nframes, hipMemcpyDeviceToHost));
    return MRGINGHAM_AMD_OK;
}

int mrgingham_amd_debug_refine_clock(mrgingham_amd_ctx* ctx, long long* h_ticks12) {
    if (!ctx || !h_ticks12) return MRGINGHAM_AMD_ERR_ARG;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    MRG_HIP_CHECK(hipDeviceSynchronize());
    const DevBuf& b = ctx->pts[ctx->cur].sroot;
    if (!b.p || b.bytes < 12 * sizeof(long long)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "no refinement has run yet");
    MRG_HIP_CHECK(hipMemcpy(h_ticks12, b.p, 12 * sizeof(long long), hipMemcpyDeviceToHost));
    return MRGINGHAM_AMD_OK;
}

int mrgingham_amd_chain_info(const mrgingham_amd_ctx* ctx, int* fused_pyramid, int* merged_levels) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (fused_pyramid) *fused_pyramid = ctx->last_fused;
    if (merged_levels) *merged_levels = ctx->last_merged;
    return 0;
}

long long mrgingham_amd_scratch_bytes(const mrgingham_amd_ctx* ctx) {
    if (!ctx) return 0;
    long long total = ctx->scratch_total;
    if (ctx->one) total += mrgingham_amd_scratch_bytes(ctx->one);
    return total;
}

const char* mrgingham_amd_last_error(const mrgingham_amd_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }

int mrgingham_amd_sparse_fallbacks(mrgingham_amd_ctx* ctx) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (!ctx->sparse_stat.p) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    MRG_HIP_CHECK(hipDeviceSynchronize());
    int32_t n = 0;
    MRG_HIP_CHECK(hipMemcpy(&n, ctx->sparse_stat.p, sizeof(n), hipMemcpyDeviceToHost));
    MRG_HIP_CHECK(hipMemset(ctx->sparse_stat.p, 0, sizeof(n)));
    return n;
}

void mrgingham_amd_set_kernel_timing(mrgingham_amd_ctx* ctx, int enable) {
    if (!ctx) return;
    ctx->timing = (enable & 1) != 0;   // bit 0: hipEvents around the level-0 response launches
    ctx->clk_on = enable != 0;         // any non-zero value: the engine-clock probe (2 = the probe alone, no events)
    if (ctx->clk_on && !ctx->clk.p) {  // the engine-clock probe's two counters (without them the probe stays off)
        const CallerDevice keep;
        hipSetDevice(ctx->device);
        if (ensure(ctx, ctx->clk, 2 * sizeof(unsigned long long)) == 0) hipMemset(ctx->clk.p, 0, 2 * sizeof(unsigned long long));
    }
}

double mrgingham_amd_sclk_mhz(mrgingham_amd_ctx* ctx) {
    if (!ctx || !ctx->clk.p) return 0.;
    const CallerDevice keep;
    hipSetDevice(ctx->device);
    if (hipDeviceSynchronize() != hipSuccess) return 0.;
    unsigned long long c[2] = {0, 0};
    if (hipMemcpy(c, ctx->clk.p, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess) return 0.;
    hipMemset(ctx->clk.p, 0, sizeof(c));
    int khz = 0;  // rate of s_memrealtime
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) != hipSuccess || khz <= 0) khz = 100000;
    return c[1] ? (double)c[0] / (double)c[1] * khz * 1e-3 : 0.;
}

// set_option "scratch_fill_now" (test hook, ctx.h): with nothing of the context in flight, every scratch buffer it owns
// gets `byte` over its whole size -- but for the state ctx.h lists
static int fill_scratch_now(mrgingham_amd_ctx* ctx, int byte) {
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    const int rc = mrgingham_amd_sync(ctx);
    MRG_HIP_CHECK(hipDeviceSynchronize());
    ctx->pixel_stage.valid = false;  // (mrgingham_amd_debug_pixel_products reads scratch)
    for (DevBuf* b : ctx->scratch_bufs) {
        if (!b->p || b == &ctx->sparse_stat || b == &ctx->clk || b == &ctx->grid_stat) continue;
        size_t skip = 0;  // counters2: the hot-count and status words stay, the path words behind them go
        for (const DevBuf& c : ctx->counters2)
            if (b == &c) skip = (size_t)(kMaxLevel + 1) * 2 * (size_t)ctx->counters_nf * sizeof(int32_t);
        if (skip < b->bytes) MRG_HIP_CHECK(hipMemset((char*)b->p + skip, byte, b->bytes - skip));
    }
    for (PinBuf* b : ctx->pinned_bufs)
        if (b->p) memset(b->p, byte, b->bytes);
    MRG_HIP_CHECK(hipDeviceSynchronize());
    if (ctx->one) {
        const int r1 = fill_scratch_now(ctx->one, byte);
        if (r1) return r1;
    }
    return rc;
}

/* tunables (not part of the reference surface) */
int mrgingham_amd_set_option(mrgingham_amd_ctx* ctx, const char* name, int value) {
    if (!ctx || !name) return MRGINGHAM_AMD_ERR_ARG;
    fb_drain(ctx);
    if (!strcmp(name, "scratch_fill")) {  // test hook (ctx.h): what new allocations of this context are filled with, -1 = nothing
        if (value < -1 || value > 255) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "scratch_fill: -1 (off) or a byte");
        ctx->scratch_fill = value;
        if (ctx->one) ctx->one->scratch_fill = value;
        return 0;
    }
    if (!strcmp(name, "scratch_fill_now")) {
        if (value < 0 || value > 255) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "scratch_fill_now: a byte");
        return fill_scratch_now(ctx, value);
    }
    if (!strcmp(name, "hot_capacity_shift")) {
        if (value < 0 || value > 10) return MRGINGHAM_AMD_ERR_ARG;
        ctx->cap_shift = value;
        for (int& g : ctx->grown_shift) g = 31;  // an explicit choice starts over
        return 0;
    }
    if (!strcmp(name, "hot_capacity_shift_temporary")) {
        // the retry of a caller (one table entry per pixel for one call, then back): the capacity changes, what the tables
        // have GROWN to is kept -- a context that has met an adversarial frame does not forget it (the C wrappers do the
        // same around their last attempt)
        if (value < 0 || value > 10) return MRGINGHAM_AMD_ERR_ARG;
        ctx->cap_shift = value;
        return 0;
    }
#ifdef MRG_EXPERIMENT
    if (!strcmp(name, "chess_v0")) { ctx->use_v0 = value != 0; return 0; }
#endif
    if (!strcmp(name, "chess_variant")) {
        if (value != 0 && value != 1 && value != 16) return MRGINGHAM_AMD_ERR_ARG;
        ctx->chess_variant = value;
        return 0;
    }
#ifdef MRG_EXPERIMENT
    if (!strcmp(name, "chess16_pair")) { mrg::chess16_pair = value != 0; return 0; }
    if (!strcmp(name, "chess_variant_hot")) {
        if (value & ~48) return MRGINGHAM_AMD_ERR_ARG;  // 16: levels below 0 on chess_v16, 32: level 0 with the level images on chess_v16
        ctx->chess_variant_hot = value;
        return 0;
    }
#endif
    if (!strcmp(name, "sparse_subsets")) {
        if (value < 1 || value > 4) return MRGINGHAM_AMD_ERR_ARG;
        ctx->sparse_subsets = value;
        return 0;
    }
#ifdef MRG_EXPERIMENT
    if (!strcmp(name, "clahe_hist_copies")) { mrg::clahe_hist_copies = value; return 0; }
#endif
    if (!strcmp(name, "preprocess_fused")) { ctx->pre_fused = value != 0; return 0; }
    if (!strcmp(name, "chess16_seg") || !strcmp(name, "chess_seg")) {
        // rows per workgroup of chess_v16_kernel / the chess_v1 kernels of THIS context (0 = automatic): the frame is cut into
        // ceil(height / value) balanced segments (common.h, segment_rows)
        if (value < 0 || value > 65536) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "%s: 0 (automatic) or a row count", name);
        (name[5] == '1' ? ctx->chess16_seg : ctx->chess_seg) = value;
        return 0;
    }
    if (!strcmp(name, "multi_level_launch")) { ctx->multi_level = value < 0 ? 0 : value > 2 ? 2 : value; return 0; }
#ifdef MRG_EXPERIMENT
    if (!strcmp(name, "cc_schedule")) { ctx->cc_schedule = value; return 0; }
    if (!strcmp(name, "chess_multi_min_blocks")) { mrg::chess_multi_min_blocks = value; return 0; }
    if (!strcmp(name, "chess_stage")) { mrg::chess_stage_override = value; return 0; }
    if (!strcmp(name, "pyramid_lds_pad")) { mrg::pyramid_lds_pad = value; return 0; }
#endif
    if (!strcmp(name, "scratch_sets")) {
        if (value != 0 && (value < 2 || value > kMaxSets))
            return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "scratch_sets must be 0 (automatic), 2 or %d", kMaxSets);
        const int rc = mrgingham_amd_sync(ctx);  // nothing may be in flight when the rotation changes
        ctx->nsets_fixed = value != 0;
        if (value) ctx->nsets = value;
        ctx->cur = 0;
        return rc;
    }
    if (!strcmp(name, "fuse_pyramid")) { ctx->fuse_pyramid = value != 0; return 0; }
    if (!strcmp(name, "find_boards_pipeline")) { ctx->fb_pipeline = value != 0; return 0; }
    if (!strcmp(name, "find_boards_grid")) {
        if (value != 0 && value != 1) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "find_boards_grid: 0 (the host grid finder) or 1 (the device's)");
        ctx->fb_grid_device = value;
        return 0;
    }
    if (!strcmp(name, "find_grids_guard_bits")) {
        if (value < 8 || value > 45) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "find_grids_guard_bits: 8 .. 45");
        ctx->find_grids_guard_bits = value;
        return 0;
    }
    if (!strcmp(name, "blob_chunk_frames")) {
        if (value < 0) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "blob_chunk_frames: 0 (by the scratch budget) or a frame count");
        ctx->blob_chunk_frames = value;
        return 0;
    }
    if (!strcmp(name, "jpeg_chunk_frames")) {
        if (value < 0) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "jpeg_chunk_frames: 0 (by the scratch budget) or a frame count");
        ctx->jpeg_chunk_frames = value;
        return 0;
    }
    if (!strcmp(name, "png_chunk_frames")) {
        if (value < 0) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "png_chunk_frames: 0 (by the scratch budget) or a file count");
        ctx->png_chunk_frames = value;
        return 0;
    }
    if (!strcmp(name, "pgm_chunk_frames")) {
        if (value < 0) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "pgm_chunk_frames: 0 (by the scratch budget) or a file count");
        ctx->pgm_chunk_frames = value;
        return 0;
    }
    if (!strcmp(name, "tiff_chunk_frames")) {
        if (value < 0) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "tiff_chunk_frames: 0 (by the scratch budget) or a file count");
        ctx->tiff_chunk_frames = value;
        return 0;
    }
    if (!strcmp(name, "bmp_chunk_frames")) {
        if (value < 0) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bmp_chunk_frames: 0 (by the scratch budget) or a file count");
        ctx->bmp_chunk_frames = value;
        return 0;
    }
    if (!strcmp(name, "bmp_unpack")) {
        if (value != 0 && value != 1) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bmp_unpack: 0 (host threads decode) or 1 (the device unpacks)");
        ctx->bmp_unpack = value;
        return 0;
    }
    if (!strcmp(name, "pnm_chunk_frames")) {
        if (value < 0) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "pnm_chunk_frames: 0 (by the scratch budget) or a file count");
        ctx->pnm_chunk_frames = value;
        return 0;
    }
    if (!strcmp(name, "pnm_unpack")) {
        if (value != 0 && value != 1) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "pnm_unpack: 0 (host threads decode) or 1 (the device unpacks)");
        ctx->pnm_unpack = value;
        return 0;
    }
    if (!strcmp(name, "tiff_lzw_max_strip")) {
        if (value < 1 || value > (1 << 20)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "tiff_lzw_max_strip: decoded bytes per strip, 1 .. 1048576");
        ctx->tiff_lzw_max_strip = value;
        return 0;
    }
    if (!strcmp(name, "tiff_lzw_lanes")) {
        if (value < 0 || value > 16384 || (value & 63)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "tiff_lzw_lanes: 0 (16384) or a multiple of 64 up to 16384");
        ctx->tiff_lzw_lanes = value;
        return 0;
    }
    if (!strcmp(name, "tiff_deflate")) {
        if (value != 0 && value != 1) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "tiff_deflate: 0 (host threads) or 1 (the device, for strips up to tiff_deflate_max_strip)");
        ctx->tiff_deflate = value;
        return 0;
    }
    if (!strcmp(name, "tiff_deflate_max_strip")) {
        if (value < 0 || value > (1 << 20)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "tiff_deflate_max_strip: decoded bytes per strip, 0 (no file) .. 1048576");
        ctx->tiff_deflate_max_strip = value;
        return 0;
    }
    if (!strcmp(name, "tiff_deflate_lanes")) {
        if (value < 0 || value > mrgingham_amd_tiff_inflate_lanes() || (value & 63))
            return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "tiff_deflate_lanes: 0 (the shipped count) or a multiple of 64 up to it");
        ctx->tiff_deflate_lanes = value;
        return 0;
    }
    if (!strcmp(name, "jpeg_entropy")) {
        if (value != 0 && value != 1) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "jpeg_entropy: 0 (host threads) or 1 (the device, for files with restart intervals)");
        ctx->jpeg_entropy = value;
        return 0;
    }
    if (!strcmp(name, "jpeg_entropy_max_interval")) {
        if (value < 1) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "jpeg_entropy_max_interval: at least 1 MCU");
        ctx->jpeg_entropy_max_interval = value;
        return 0;
    }
    if (!strcmp(name, "jpeg_sync")) {
        if (value != 0 && value != 1) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "jpeg_sync: 0 (files without restart intervals keep the host decoder) or 1 (the device decodes them)");
        ctx->jpeg_sync = value;
        return 0;
    }
    if (!strcmp(name, "jpeg_sync_subsequence")) {
        if (value < 8 || value > 1024 || (value & 3)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "jpeg_sync_subsequence: bytes, a multiple of 4 in 8..1024");
        ctx->jpeg_sync_subsequence = value;
        return 0;
    }
    if (!strcmp(name, "jpeg_sync_max_rounds")) {
        if (value < 0 || value > 4096) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "jpeg_sync_max_rounds: 0 (8192 / jpeg_sync_subsequence) or 1..4096");
        ctx->jpeg_sync_max_rounds = value;
        return 0;
    }
    if (!strcmp(name, "jpeg_sync_time_phase")) {
        if (value < 0 || value > 4) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "jpeg_sync_time_phase: 0 (all launches) or 1..4 (round 0, update rounds, scan, write pass)");
        ctx->jpeg_sync_time_phase = value;
        return 0;
    }
    if (!strcmp(name, "jpeg_entropy_memset")) { ctx->jpeg_entropy_memset = value != 0; return 0; }
    if (!strcmp(name, "sparse_refine")) {
        if (value < 0 || value > 2) return MRGINGHAM_AMD_ERR_ARG;
        ctx->sparse_refine = value;
        return 0;
    }
    if (!strcmp(name, "cc_lds")) {
        // 0 / 1 and the test hook 256 (no banding, no windows: every result is still exact); the timing ablations
        // (bits 2, 4, 8, 16, 128) and the phase clock (512) exist in -DMRG_EXPERIMENT builds only
#ifndef MRG_EXPERIMENT
        if (value & ~(1 | 256)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "cc_lds: only 0, 1 and 1 | 256 in this build");
#endif
        ctx->cc_lds = value;
        return 0;
    }
    return MRGINGHAM_AMD_ERR_ARG;
}

double mrgingham_amd_chess_kernel_ms(mrgingham_amd_ctx* ctx, int* nlaunches) {
    if (nlaunches) *nlaunches = 0;
    if (!ctx) return 0.;
    hipSetDevice(ctx->device);
    hipDeviceSynchronize();
    double total = 0.;
    int n = 0;
    TimingEvents& te = ctx->timing_events;
    for (auto& pr : te.pairs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { total += ms; ++n; }
    }
    te.pairs.clear();
    te.idle.clear();  // (nothing is recorded across a read-out: every event is idle again)
    for (const Event& e : te.all) te.idle.push_back(e);
    if (nlaunches) *nlaunches = n;
    return n ? total / n : 0.;
}


int mrgingham_amd_sync(mrgingham_amd_ctx* ctx) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    MRG_HIP_CHECK(hipStreamSynchronize(ctx->pix));
    for (int set = 0; set < kMaxSets; ++set) {
        MRG_HIP_CHECK(hipStreamSynchronize(ctx->ccs[set]));
        ctx->cc_pending[set] = false;
    }
    MRG_HIP_CHECK(hipGetLastError());
    int rc = MRGINGHAM_AMD_OK;
    for (int set = 0; set < kMaxSets; ++set) {
        const int r = harvest_set(ctx, set, &rc);
        if (r) return r;
    }
    return rc;
}

int mrgingham_amd_stream_wait(mrgingham_amd_ctx* ctx, void* stream) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    for (int set = 0; set < kMaxSets; ++set)  // consecutive calls finish on different component streams
        if (ctx->cc_pending[set]) MRG_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, ctx->ev_cc_done[set], 0));
    return MRGINGHAM_AMD_OK;
}

int mrgingham_amd_after_stream(mrgingham_amd_ctx* ctx, void* stream) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    MRG_HIP_CHECK(ctx->ev_ext.create(hipEventDisableTiming));
    MRG_HIP_CHECK(hipEventRecord(ctx->ev_ext, (hipStream_t)stream));
    // every kernel of a call is ordered behind the pixel stream's work of that call
    MRG_HIP_CHECK(hipStreamWaitEvent(ctx->pix, ctx->ev_ext, 0));
    return MRGINGHAM_AMD_OK;
}

int mrgingham_amd_chess_response_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int level,
                                       int clamp, int16_t* d_response, void* stream) {
    int rc = validate_frames(ctx, fr);
    if (rc) return rc;
    int w, h;
    if (level_dims(fr->width, fr->height, level, &w, &h) || !d_response)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad level %d or NULL response", level);
    if (fr->nframes == 0) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;  // used as given: NULL is HIP's default stream
    LevelBatch lb;
    lb.nframes = fr->nframes;
    lb.w = w;
    lb.h = h;
    if (level == 0) {
        lb.img = fr->frames;
        lb.img_pitch = fr->frame_pitch;
        lb.img_stride = fr->stride;
    } else {
        if ((rc = ensure(ctx, ctx->aux_img, (size_t)fr->nframes * w * h + 16))) return rc;
        launch_one_level_image(fr, level, (uint8_t*)ctx->aux_img.p, w, h, s);
        lb.img = (const uint8_t*)ctx->aux_img.p;
        lb.img_pitch = (long long)w * h;
        lb.img_stride = w;
    }
    lb.resp = d_response;
    lb.resp_pitch = (long long)w * h;
    if (level == 0 && ctx->clk_on) lb.clk = (unsigned long long*)ctx->clk.p;
    launch_chess_any(ctx, lb, CompTables{}, fr->nframes, clamp != 0, false, s, level == 0);
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

int mrgingham_amd_decimate_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int level, uint8_t* d_out,
                                 void* stream) {
    int rc = validate_frames(ctx, fr);
    if (rc) return rc;
    int w, h;
    if (level_dims(fr->width, fr->height, level, &w, &h) || !d_out)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad level %d or NULL output", level);
    if (fr->nframes == 0) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;  // used as given: NULL is HIP's default stream
    if (level == 0) {
        for (int f = 0; f < fr->nframes; ++f)
            MRG_HIP_CHECK(copy_rows_async(d_out + (size_t)f * w * h, w, fr->frames + (size_t)f * fr->frame_pitch,
                                          fr->stride, w, h, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    launch_one_level_image(fr, level, d_out, w, h, s);
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

int mrgingham_amd_box_blur_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int radius, uint8_t* d_out,
                                 void* stream) {
    int rc = validate_frames(ctx, fr);
    if (rc) return rc;
    if (radius < 0 || radius > 64 || !d_out) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad blur radius or output");
    if (fr->nframes == 0) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;  // used as given: NULL is HIP's default stream
    FrameBatch fb{fr->frames, fr->frame_pitch, fr->width, fr->height, fr->stride};
    launch_box_blur(fb, radius, d_out, 0, fr->nframes, s);
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

int mrgingham_amd_preprocess_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int do_clahe,
                                   int blur_radius, uint8_t* d_out, void* stream) {
    int rc = validate_frames(ctx, fr);
    if (rc) return rc;
    if (blur_radius < 0 || blur_radius > 64 || !d_out)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad blur radius or output");
    if (fr->nframes == 0) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;  // used as given: NULL is HIP's default stream
    FrameBatch fb{fr->frames, fr->frame_pitch, fr->width, fr->height, fr->stride};
    if (do_clahe) {
        if (fr->width < 8 || fr->height < 8)
            return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "CLAHE needs a frame of at least 8x8 pixels");
        const size_t frame_bytes = (size_t)fr->width * fr->height;
        if ((rc = ensure(ctx, ctx->pre_scratch, clahe_scratch_bytes(fr->nframes)))) return rc;
        // clip limit 8, default 8x8 tiles: mrgingham-from-image.cc:41-45
        if (blur_radius == 1 && ctx->pre_fused) {
            // the tool's default chain: blend + 3x3 blur in one pass over the frame where the geometry allows it
            uint8_t* tmp = nullptr;
            if (!clahe_blur3_fused(fb, d_out)) {
                if ((rc = ensure(ctx, ctx->pre_tmp, frame_bytes * fr->nframes))) return rc;
                tmp = (uint8_t*)ctx->pre_tmp.p;
            }
            launch_clahe(fb, fr->nframes, 8.0, true, d_out, ctx->pre_scratch.p, s, true, tmp, ctx->clk_on ? (unsigned long long*)ctx->clk.p : nullptr);
        } else {
            uint8_t* clahe_out = d_out;
            if (blur_radius > 0) {
                if ((rc = ensure(ctx, ctx->pre_tmp, frame_bytes * fr->nframes))) return rc;
                clahe_out = (uint8_t*)ctx->pre_tmp.p;
            }
            launch_clahe(fb, fr->nframes, 8.0, true, clahe_out, ctx->pre_scratch.p, s);
            if (blur_radius > 0) {
                const FrameBatch tb{clahe_out, (long long)frame_bytes, fr->width, fr->height, fr->width};
                launch_box_blur(tb, blur_radius, d_out, 0, fr->nframes, s);
            }
        }
    } else {
        launch_box_blur(fb, blur_radius, d_out, 0, fr->nframes, s);  // radius 0 = dense copy
    }
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

int mrgingham_amd_preprocess16_batch(mrgingham_amd_ctx* ctx, const uint16_t* d_frames, int64_t frame_pitch, int nframes,
                                     int width, int height, int stride, int do_clahe, int blur_radius, uint8_t* d_out,
                                     void* stream) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if ((!d_frames && nframes > 0) || nframes < 0 || width < 0 || height < 0 || stride < width || frame_pitch < 0)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad frame batch descriptor");
    if (width > 32767 || height > 32767)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "frames larger than 32767 pixels per side are not supported");
    if (blur_radius < 0 || blur_radius > 64 || !d_out) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad blur radius or output");
    if (do_clahe && (width < 8 || height < 8))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "CLAHE needs a frame of at least 8x8 pixels");
    if (nframes == 0 || width == 0 || height == 0) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    return queue_preprocess16(ctx, d_frames, frame_pitch, nframes, width, height, stride, do_clahe, blur_radius, d_out,
                              (hipStream_t)stream);  // (the stream used as given: NULL is HIP's default stream)
}

}  // extern "C"

// the work of mrgingham_amd_preprocess16_batch, its arguments checked (and frames of any size: the tile grid of a frame
// below 8 pixels per side is 8 tiles of one pixel, as the one-image path of the command-line tool has always taken it)
int mrg::queue_preprocess16(mrgingham_amd_ctx* ctx, const uint16_t* d_frames, int64_t frame_pitch, int nframes, int width, int height,
                       int stride, int do_clahe, int blur_radius, uint8_t* d_out, hipStream_t s) {
    if (blur_radius < 0 || blur_radius > 64) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad blur radius");
    const size_t frame_bytes = (size_t)width * height;
    const int chunk = preprocess16_batch_chunk_frames();
    const int nf = nframes < chunk ? nframes : chunk;
    int rc;
    if (ctx->pre_fused) {
        uint8_t* tmp = nullptr;
        if (do_clahe && (rc = ensure(ctx, ctx->pre16_scratch, preprocess16_batch_scratch_bytes(nf)))) return rc;
        if (blur_radius > 1) {
            if ((rc = ensure(ctx, ctx->pre_tmp, frame_bytes * nframes))) return rc;
            tmp = (uint8_t*)ctx->pre_tmp.p;
        }
        if (!launch_preprocess16_batch(d_frames, (long long)frame_pitch, nframes, width, height, stride, do_clahe != 0, blur_radius,
                                       d_out, ctx->pre16_scratch.p, tmp, s, ctx->clk_on ? (unsigned long long*)ctx->clk.p : nullptr))
            return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "frame too small to tile");
    } else {
        // option "preprocess_fused" 0: the one-image kernels (preprocess16.hip) + launch_box_blur, chunk by chunk
        if (do_clahe && (rc = ensure(ctx, ctx->pre16_scratch, preprocess16_scratch_bytes(nf, width, height)))) return rc;
        uint8_t* eight = d_out;
        if (blur_radius > 0) {
            if ((rc = ensure(ctx, ctx->pre_tmp, frame_bytes * nf))) return rc;
            eight = (uint8_t*)ctx->pre_tmp.p;
        }
        for (int f0 = 0; f0 < nframes; f0 += nf) {
            const int n = nframes - f0 < nf ? nframes - f0 : nf;
            uint8_t* o = d_out + (size_t)f0 * frame_bytes;
            if (!launch_preprocess16(d_frames + (size_t)f0 * frame_pitch, (long long)frame_pitch, n, width, height, stride,
                                     do_clahe != 0, 8.0, blur_radius > 0 ? eight : o, ctx->pre16_scratch.p, s))
                return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "frame too small to tile");
            if (blur_radius > 0)
                launch_box_blur(FrameBatch{eight, (long long)frame_bytes, width, height, width}, blur_radius, o, 0, n, s);
        }
    }
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}
