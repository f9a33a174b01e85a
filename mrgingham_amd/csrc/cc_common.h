// Exact, order-preserving connected-component search on the GPU (gfx950).
//
// The reference (find_chessboard_corners.cc:159-267, :284-397) walks the clamped
// response in raster order and flood-fills with a LIFO whose running-maximum
// threshold makes the result depend on visiting order.  It is reproduced
// bit-exactly, in parallel, from two facts:
//
//  (1) only "hot" pixels (response > 15) are ever accumulated or expanded: a
//      pixel in (0,15] that gets pushed is popped, found invalid and zeroed with
//      no other effect (:243-247), so it can simply not be pushed;
//  (2) a fill never leaves the 4-connected region of hot pixels that contains
//      its seed (a "super-component"), responses only ever decrease to 0, and
//      the margin flag depends only on coordinates (:216-221).  Super-components
//      are therefore independent of each other; only WITHIN one must the
//      reference's sequence (raster order of seeds, push order +x,-x,+y,-y,
//      first-maximum-wins) be replayed, and that is done by a single lane.
//
// Two implementations of that, tried in this order per frame (CompTables::path says which one took it):
//   * out of LDS (cc_lds.hip): the hot list, the values of the listed pixels, a hash map and
//     the LIFOs of a frame -- or of a band of it -- in 40 KB; the common case;
//   * in global memory (cc.hip): one 512-thread workgroup per frame, every hand-off a workgroup barrier
//     (no cross-XCD traffic, no grid sync):
//       P0-P2 union-find over the hot list (left/up neighbours), flatten, per-root count / box / first pixel
//       P3    one lane per root: scan its box in raster order, replay the fills (detect)  |  group the points
//             that share super-components, one lane per group replays them in index order (refine)
//       P4    21x21 variance test of every surviving component (:50-88), same lane
//       P5    order by seed raster index (detect: bitonic sort) and emit coordinates.
//
// Floating point: centroid, level rescaling and the *1000 rounding are the
// reference's exact double expressions (:262-263, :278-279, :350-351); both units
// are compiled with -ffp-contract=off so no FMA changes a truncation.
#pragma once
#include "common.h"
#include "hotlist.h"
#include "kernels.h"

namespace mrg {

// Timing ablations and phase clocks (they change results or write debug data) exist only in builds made with
// -DMRG_EXPERIMENT (tools/build_variant.sh); the shipped library ignores those bits of CompTables::lds_path.
#ifdef MRG_EXPERIMENT
#define MRG_EXP(bits) ((bits) != 0)
#else
#define MRG_EXP(bits) false
#endif

constexpr int CC_THREADS = 256;

// Every table of a frame is only ever touched by ONE workgroup per kernel (the detect / refine kernels
// run one workgroup per frame), so the atomics on them are
// WORKGROUP scope: they execute in the XCD's L2.  Agent-scope atomics on this multi-XCD part go to
// the memory side instead; a few hundred thousand of them per level were slowing the HBM-streaming
// pixel kernels they run underneath by ~6 % (measured by replacing the labelling kernels with empty
// ones).  Kernel boundaries make the results visible to the next kernel.
#define MRG_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP
__device__ __forceinline__ int aload(const int32_t* p) { return __hip_atomic_load(p, MRG_WG); }
__device__ __forceinline__ int wg_min(int32_t* p, int v) { return __hip_atomic_fetch_min(p, v, MRG_WG); }
__device__ __forceinline__ int wg_max(int32_t* p, int v) { return __hip_atomic_fetch_max(p, v, MRG_WG); }
__device__ __forceinline__ int wg_add(int32_t* p, int v) { return __hip_atomic_fetch_add(p, v, MRG_WG); }
__device__ __forceinline__ int wg_or(int32_t* p, int v) { return __hip_atomic_fetch_or(p, v, MRG_WG); }
// status word of a hot-list overflow: the flag + the number of hot pixels the frame has, in units of 64, above bit 8
// (the host grows the tables to that, api.hip mrgingham_amd_sync)
__device__ __forceinline__ int hot_overflow_status(int hot_cnt) {
    const uint32_t units = ((uint32_t)hot_cnt + 63u) >> 6;
    return (int)((uint32_t)kStatusHotOverflow | ((units > 0x7fffffu ? 0x7fffffu : units) << 8));
}
// Reports it in the frame's status word: the flag bits are OR-ed, the demand field keeps the MAXIMUM -- status words
// accumulate until the host looks at them, and pipelined calls that reuse a scratch set must not OR two demands into a
// number neither frame asked for (the tables would over-grow by up to 2x).  One thread per frame calls this.
__device__ __forceinline__ void report_hot_overflow(int32_t* word, int hot_cnt) {
    const uint32_t want = (uint32_t)hot_overflow_status(hot_cnt);
    uint32_t old = (uint32_t)aload(word);
    while (true) {
        const uint32_t demand = (old >> 8) > (want >> 8) ? (old >> 8) : (want >> 8);
        const uint32_t merged = ((old | want) & 0xffu) | (demand << 8);
        if (merged == old) return;
        int32_t expected = (int32_t)old;
        if (__hip_atomic_compare_exchange_strong(word, &expected, (int32_t)merged, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP))
            return;
        old = (uint32_t)expected;  // somebody else's flag arrived in between: merge again
    }
}

__device__ __forceinline__ int uf_root(const int32_t* parent, int i) {
    int p = aload(parent + i);
    while (p != i) {
        i = p;
        p = aload(parent + i);
    }
    return i;
}

// Lock-free union by minimum index.  A failed atomicMin (the target stopped
// being a root meanwhile) still leaves the forest connected: continue with the
// displaced parent.
__device__ __forceinline__ void uf_unite(int32_t* parent, int a, int b) {
    while (true) {
        a = uf_root(parent, a);
        b = uf_root(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = wg_min(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

struct FrameView {
    int w, h, n;  // level size, number of hot pixels
    const uint8_t* img;
    int img_stride;
    int16_t* d;
    uint32_t* hot_xy;
    int32_t *parent, *comp_cnt, *roots, *comp_first;
    const uint2* gidx;
    int gw;
    int4* comp_box;
    uint32_t* arena;
    long long arena_cap;
    Cand* cand;
    int cand_cap;
    unsigned long long* sortkeys;
    int sort_cap;
    int32_t* status;
};

__device__ __forceinline__ FrameView make_view(const LevelBatch& lb, const CompTables& t, int frame) {
    FrameView v;
    v.w = lb.w;
    v.h = lb.h;
    v.img = lb.img + (long long)frame * lb.img_pitch;
    v.img_stride = lb.img_stride;
    v.d = lb.resp + (long long)frame * lb.resp_pitch;
    const long long e = (long long)frame * t.cap;
    v.hot_xy = t.hot_xy + e;
    v.parent = t.parent + e;
    v.comp_cnt = t.comp_cnt + e;
    v.roots = t.roots + e;
    v.comp_first = t.comp_first + e;
    v.comp_box = t.comp_box + e;
    v.gidx = t.gidx + (long long)frame * t.gidx_pitch;
    v.gw = t.gw;
    v.arena = t.arena + (long long)frame * t.arena_cap;
    v.arena_cap = t.arena_cap;
    v.cand = t.cand + (long long)frame * t.cand_cap;
    v.cand_cap = t.cand_cap;
    v.sortkeys = t.sortkeys + (long long)frame * t.sort_cap;
    v.sort_cap = t.sort_cap;
    v.status = t.status + frame;
    const int cnt = t.hot_cnt[frame];
    v.n = cnt < t.cap ? cnt : t.cap;
    return v;
}

// 512 threads at no more than 64 VGPRs: the two waves per SIMD of such a workgroup fit into the registers ONE
// retiring wave of the pixel kernels frees (128).  With 1024 threads the kernels -- which mostly only look at
// the path word and leave -- waited for two: 0.98 -> 1.06 ms per step.
constexpr int CCG_THREADS = 512;

struct Blob {
    unsigned long long srx, sry, sr;
    int npix, rmax, xpk, ypk;
    bool touched;
};

__device__ __forceinline__ bool blob_passes_cheap_tests(const Blob& b) {
    return !b.touched && b.npix >= kBlobMinPixels && b.rmax > kPeakMin;  // :259, :205-206
}

// The 21x21 window test of high_variance (:50-88), by the lane that owns the blob, in one
// pass: with S1 = sum(v), S2 = sum(v^2) and the reference's truncated mean m = S1/441,
// sum((v-m)^2) = S2 - 2*m*S1 + 441*m^2 exactly (all integers), so var = that / 441 with the
// same truncations.  The 84 loads of a window (8+8+4+1 bytes per row, never past the window)
// are independent of each other: one round trip instead of a wave-wide phase and a barrier.
__device__ __forceinline__ bool window_variance_high(const uint8_t* img, int stride, int w, int h, int x, int y) {
    constexpr int R = kVarWindowR, D = 2 * R + 1, NPIX = D * D;  // 441
    if (x - R < 0 || x + R >= w || y - R < 0 || y + R >= h) return false;  // :52-57
    const uint8_t* p = img + (long long)(y - R) * stride + (x - R);
    uint32_t s1 = 0, s2 = 0;
#pragma unroll 3
    for (int r = 0; r < D; ++r) {
        uint32_t q[5];
        __builtin_memcpy(q, p, 20);
        const uint32_t last = p[20];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            s1 = __builtin_amdgcn_udot4(q[k], 0x01010101u, s1, false);
            s2 = __builtin_amdgcn_udot4(q[k], q[k], s2, false);
        }
        s1 += last;
        s2 += last * last;
        p += stride;
    }
    const long long mean = s1 / NPIX;                                              // :69-70
    const long long ssd = (long long)s2 - 2 * mean * (long long)s1 + NPIX * mean * mean;
    return ssd / NPIX > kVarMin;                                                   // :80-87
}

// (p + 0.5) * scale - 0.5, find_chessboard_corners.cc:278-279
__device__ __forceinline__ double rescale_coord(double p, double scale) { return (p + 0.5) * scale - 0.5; }

// Block-wide bitonic sort of n_pad (power of two) 64-bit keys in global memory.
__device__ void bitonic_sort(unsigned long long* keys, int n_pad) {
    for (int k = 2; k <= n_pad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n_pad; i += (int)blockDim.x) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = keys[i], b = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { keys[i] = b; keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
}

// Candidates in output order -> coordinates (the reference's exact double expressions), and the chain's
// hand-over to the refinement.  keys[k] & 0xffffffff indexes v.cand; all threads of the workgroup call it.
__device__ __forceinline__ void emit_detect_outputs(const FrameView& v, const unsigned long long* keys, int nvalid,
                                                    int level, const DetectOut& out, int frame) {
    const double scale = (double)(uint16_t)(1u << level);  // :319
    int32_t* oxy = out.xy + (long long)frame * out.capacity * 2;
    const int nout = nvalid < out.capacity ? nvalid : out.capacity;
    // the chain's hand-over to refinement, fused: every candidate becomes a corner at this level
    // ((double)x / 1000, find_grid.cc:353-354; level tags, mrgingham.cc:81-85)
    const int npt = out.points ? (nout < out.points_pitch ? nout : out.points_pitch) : 0;
    double* opt = out.points ? out.points + (long long)frame * out.points_pitch * 2 : nullptr;
    signed char* olv = out.points ? out.levels + (long long)frame * out.points_pitch : nullptr;
    for (int k = threadIdx.x; k < nout; k += (int)blockDim.x) {
        const Cand& cd = v.cand[(uint32_t)(keys[k] & 0xffffffffu)];
        const double cx = (double)cd.sum_rx / (double)cd.sum_r;  // :262-263
        const double cy = (double)cd.sum_ry / (double)cd.sum_r;
        const double px = rescale_coord(cx, scale), py = rescale_coord(cy, scale);  // :346
        const int ix = (int)(0.5 + px * kGridScale), iy = (int)(0.5 + py * kGridScale);  // :350-351
        oxy[2 * k + 0] = ix;
        oxy[2 * k + 1] = iy;
        if (k < npt) {
            opt[2 * k + 0] = (double)ix / kGridScale;
            opt[2 * k + 1] = (double)iy / kGridScale;
            olv[k] = (signed char)level;
        }
    }
    if (threadIdx.x == 0) {
        out.counts[frame] = nvalid;
        if (out.points) out.npoints[frame] = npt;
    }
}

// the launchers of one unit that the other calls, and the kernel launch_cc_detect_levels (cc_lds.hip) launches out of cc.hip
void launch_cc_detect_lds(const LevelBatch& lb, const CompTables& t, int level, const DetectOut& out, int frame0,
                          int nframes, hipStream_t s);
void launch_cc_refine_lds(const LevelBatch& lb, const CompTables& t, int level, const RefineIO& io, int frame0,
                          int nframes, hipStream_t s);
__global__ __launch_bounds__(CCG_THREADS, 4) void cc_detect_levels_kernel(DetectLevels a);

}  // namespace mrg
