#pragma once
#include "cc_common.h"

namespace mrg {

// ===========================================================================
// LDS path.  A calibration frame has ~10^3 hot pixels per pyramid level (a dozen per corner), and the
// global-memory kernels (cc.hip) spend their time in chains of dependent global accesses (2-3 us each underneath a
// bandwidth-saturating pixel kernel): 50-100 us for the labelling, 100-260 us for the fills.  When a
// frame's hot list fits -- at most LN entries -- the whole search runs out of LDS instead: the list, the
// response VALUES of the listed pixels (the only responses the search ever uses, see (1) at the top), a
// hash map pixel -> entry for the neighbour lookups, labels, and the LIFOs.  Same sequence of
// operations as above, hence the same results bit for bit; the dense response is only read (once per
// hot pixel), never written.  Frames that do not fit (hot pixels, components or LIFO demand) are left
// to the global-memory kernels through CompTables::path.
//
// LDS per workgroup: 40 KB, the slot one ChESS workgroup leaves when it retires (39 952 B there, 40 960 B in
// allocation granules: four per CU).
//
// Frames with MORE hot pixels than the tables hold (a 14x14 board has ~2600 at level 0) are cut into
// horizontal BANDS of at most LN hot pixels each, separated by three consecutive rows without a hot pixel,
// and the same workgroup runs the search band after band on the same tables:
//   * no 4-connected component crosses a row without hot pixels, so every component -- and with it every
//     fill, its running maximum and its order of operations -- lies inside one band;
//   * the 3x3 seed window of a refined point spans three rows, so it cannot hold hot pixels of two bands
//     (they are at least four rows apart): a point is refined in the band its seeds are in, and points
//     that share a component share the band;
//   * the output order of detect is by seed position and is restored by the final sort.
// A frame whose rows do not offer such separators (or with more than kMaxBands * LN hot pixels, or more
// than kBandRows rows) goes to the global-memory kernels like before.  (Round 2 first had a second kernel
// with 4096-entry tables = 80 KB = two ChESS workgroup slots: it waited 100-900 us for two ADJACENT slots to
// fall free underneath the level-0 launch, and BASELINE config 3 as stated was bound by that wait.)
// ===========================================================================
constexpr int kMaxBands = 8;
template <int N>
struct LdsCCT {
    static constexpr int LN = N;              // hot-list entries
    static constexpr int LHASH = 2 * N;       // 16-bit hash slots (load factor <= 0.5)
    static constexpr int LSTK = 5 * N / 2;    // 16-bit LIFO words shared by the fills of a frame
    static constexpr int LROOTS = N / 4;      // super-components with >= 2 pixels (detect)
    static constexpr int LEPT = N / CC_THREADS;  // list entries per thread
    uint32_t xy[LN];              // (y << 16) | x, kHotDead for an unused slot
    int16_t val[LN];              // clamped response of the pixel; 0 once consumed by a fill
    int16_t lab[LN];              // smallest list index of the pixel's super-component
    uint32_t hashw[LHASH / 2];    // two 16-bit slots per word: list index, 0xffff = empty
    union {
        int16_t stk[LSTK];        // LIFOs (list indices)
        int32_t acc[LN];          // per-root accumulators / claim table, before the fills
        unsigned long long keys[LSTK / 4];  // sort keys, after the fills
    } u;
    union {
        // detect, per super-component with >= 2 pixels: list index of its root (later: offset of its member
        // list), pixel count, LIFO demand, list index of its pixel with the smallest raster position
        struct { int16_t root[LROOTS], cnt[LROOTS], soff[LROOTS], fidx[LROOTS]; } r;
        int16_t need16[LN + 512]; // refine: LIFO demand of the super-component, at its root; behind them lead16[LPTS]
    } w;
    int nroots, ncand, top, total, changed, nref, mtop, nload, leak;
    int nbands, best, band_y[kMaxBands + 1], shear;
    uint32_t edge[4];
};
constexpr int LPTS = 512;                    // points per frame the LDS refine kernel takes (LdsCCT::w.need16 has room for it)
constexpr int LPPT = LPTS / CC_THREADS;     // points per thread
// One workgroup slot of the pixel kernels, in LDS allocation granules (1280 B on this part: 39 952 B of a ChESS
// workgroup occupy 40 960, four of them the whole 160 KB): anything above 40 960 B would need two.
static_assert(sizeof(LdsCCT<2048>) <= 40960, "must fit into the LDS slot of one ChESS workgroup");
static_assert(offsetof(LdsCCT<2048>, nroots) >= (8192 + CC_THREADS / 64) * 4, "the band planner's key arrays overlay the tables");

// Fibonacci hashing with an independent multiplier per coordinate: the hot pixels of a calibration board sit on a
// lattice, and ONE multiplier on the packed (y << 16 | x) lets only the low 16 bits of the constant act on y --
// at level 1 of a 14x14 board at 4096x3072 that put the lattice in resonance with the table (11.6 probes per
// miss, 71 at worst; the fills ran 4x longer).  Measured on 16 board / level combinations: 1.03-1.3 probes per
// hit, 1.1-2.1 per miss (tools/hash_probe.py).
// The map is bucketed: a 32-bit word is a bucket of two 16-bit list indices (0xffff = empty), probing goes bucket
// by bucket, and an element sits in the first bucket of its probe sequence that had an empty half when it came.
// A wave pays for the LONGEST probe sequence among its 64 lanes; with two candidates per probe that maximum is
// ~40 % shorter than with one (bench frames, level 0: 2.95 -> 1.73 probes, 14x14 level 1: 6.2 -> 3.4), at the
// same two dependent LDS round trips per probe (the word, then both positions).
template <class LdsCC>
__device__ __forceinline__ uint32_t lds_hash(uint32_t e) {
    static_assert(LdsCC::LHASH == 4096, "the shift below takes the top 11 bits: LHASH / 2 buckets");
    return ((e & 0xffffu) * 0x9E3779B1u + (e >> 16) * 0x85EBCA77u) >> 21;
}
template <class LdsCC>
__device__ __forceinline__ uint32_t lds_next_bucket(uint32_t b) { return (b + 1u) & (uint32_t)(LdsCC::LHASH / 2 - 1); }

template <class LdsCC>
__device__ __forceinline__ void lds_insert(LdsCC& L, uint32_t e, int i) {
    uint32_t b = lds_hash<LdsCC>(e);
    while (true) {
        uint32_t* wp = &L.hashw[b];
        const uint32_t old = __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        uint32_t nw;
        if ((old & 0xffffu) == 0xffffu) nw = (old & 0xffff0000u) | (uint32_t)i;
        else if ((old >> 16) == 0xffffu) nw = (old & 0xffffu) | ((uint32_t)i << 16);
        else { b = lds_next_bucket<LdsCC>(b); continue; }
        if (atomicCAS(wp, old, nw) == old) return;  // else: the word changed under us, look again
    }
}

// One probe: the bucket's two candidates against pixel q.  Returns true when the lookup is settled (j = list
// index, or -1: a bucket with an empty half ends every probe sequence that reaches it).
template <class LdsCC>
__device__ __forceinline__ bool lds_probe(uint32_t wv, uint32_t xlo, uint32_t xhi, uint32_t q, int& j) {
    const uint32_t lo = wv & 0xffffu, hi = wv >> 16;
    if (lo != 0xffffu && xlo == q) { j = (int)lo; return true; }
    if (hi != 0xffffu && xhi == q) { j = (int)hi; return true; }
    if (lo == 0xffffu || hi == 0xffffu) { j = -1; return true; }
    return false;
}

// list index of pixel e, or -1 when it is not hot
template <class LdsCC>
__device__ __forceinline__ int lds_find(const LdsCC& L, uint32_t e) {
    uint32_t b = lds_hash<LdsCC>(e);
    while (true) {
        const uint32_t wv = L.hashw[b];
        const uint32_t xlo = L.xy[wv & (uint32_t)(LdsCC::LN - 1)], xhi = L.xy[(wv >> 16) & (uint32_t)(LdsCC::LN - 1)];
        int j;
        if (lds_probe<LdsCC>(wv, xlo, xhi, e, j)) return j;
        b = lds_next_bucket<LdsCC>(b);
    }
}

// The four neighbours of pixel e at once: the first probes of the four lookups are independent, so their bucket
// reads and then their position reads go out together (two dependent LDS round trips for all four in the
// common case); whatever is not settled by then continues on its own.
template <class LdsCC>
__device__ __forceinline__ void lds_find4(const LdsCC& L, uint32_t e, int (&j)[4]) {
    const uint32_t q[4] = {e + 1u, e - 1u, e + 0x10000u, e - 0x10000u};
    uint32_t b[4], wv[4], xlo[4], xhi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = lds_hash<LdsCC>(q[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) wv[k] = L.hashw[b[k]];
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // (any slot: compared in lds_probe)
        xlo[k] = L.xy[wv[k] & (uint32_t)(LdsCC::LN - 1)];
        xhi[k] = L.xy[(wv[k] >> 16) & (uint32_t)(LdsCC::LN - 1)];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (lds_probe<LdsCC>(wv[k], xlo[k], xhi[k], q[k], j[k])) continue;
        uint32_t bk = lds_next_bucket<LdsCC>(b[k]);
        while (true) {
            const uint32_t w2 = L.hashw[bk];
            const uint32_t y0 = L.xy[w2 & (uint32_t)(LdsCC::LN - 1)], y1 = L.xy[(w2 >> 16) & (uint32_t)(LdsCC::LN - 1)];
            if (lds_probe<LdsCC>(w2, y0, y1, q[k], j[k])) break;
            bk = lds_next_bucket<LdsCC>(bk);
        }
    }
}

// Band key of a pixel for shear k (in 1/32 pixels of y per pixel of x, |k| <= 32): k = 0 is the row.  A board
// that is rotated in the image has its corner rows on slanted lines, and no image row between them is free of
// hot pixels -- but a sheared "row" that follows the slant is.
__device__ __forceinline__ int band_key(uint32_t e, int k, int w) {
    const int x = (int)(e & 0xffffu), y = (int)(e >> 16);
    const int ak = k < 0 ? -k : k;
    return y + (((k >= 0 ? x : w - 1 - x) * ak) >> 5);
}
// Two pixels at most 2 apart in x and in y (4-neighbours; two seeds of one 3x3 window) differ in key by at most
// this much: a band boundary with that many empty keys keeps them in one band.
__device__ __forceinline__ int band_gap(int k) {
    const int ak = k < 0 ? -k : k;
    return 2 + (ak ? (2 * ak) / 32 + 1 : 0);
}
// One pass of the workgroup over a frame's hot list (entries that hold a pixel): eight independent loads per thread
// in flight at a time.  As `for (i = tid; i < n; i += CC_THREADS) f(hot[i])` the pass is one global round trip per
// iteration -- 2-3 us each underneath the pixel kernels, i.e. 0.5 ms for the 66 000 entries of a textured frame.
template <class F>
__device__ __forceinline__ void scan_hot_list(const uint32_t* hot, int n, F&& f) {
    constexpr int U = 8;
    for (int i0 = threadIdx.x; i0 < n; i0 += CC_THREADS * U) {
        uint32_t e[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * CC_THREADS;
            e[u] = i < n ? hot[i] : kHotDead;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (e[u] != kHotDead) f(e[u]);
    }
}

constexpr int kBandKeys = 8192;  // keys 0 .. h - 1 + (w - 1) * |k| / 32 must stay below this

// One attempt at cutting the frame into bands of at most LN hot pixels along shear k.  Leaves L.nbands,
// L.band_y[0 .. nbands] (key bounds) and L.shear; returns the number of bands, 0 (uniformly) when this shear
// offers no separators.  Uses the table storage as scratch.  All threads call it.  A thread owns 32 consecutive
// keys and keeps their counts, prefix sums and "a band may end here" bits in registers, so that a greedy step
// costs one LDS read, one LDS atomic and two barriers (~10 us per attempt; with every test read from LDS in
// dependent order it was 35-50).
template <class LdsCC>
__device__ __noinline__ int lds_try_bands(LdsCC& L, const FrameView& v, int nraw, int k) {
    constexpr int LN = LdsCC::LN;
    const int tid = threadIdx.x, w = v.w;
    const int nkeys = v.h + (((w - 1) * (k < 0 ? -k : k)) >> 5);
    if (nkeys > kBandKeys) return 0;
    uint32_t* rcw = reinterpret_cast<uint32_t*>(&L);  // hot pixels per key, two 16-bit counters per word
    uint32_t* cumw = rcw + kBandKeys / 2;             // hot pixels below the key, likewise
    uint32_t* part = cumw + kBandKeys / 2;            // per-wave totals
    constexpr int WPT = kBandKeys / 2 / CC_THREADS;   // words per thread = 16 (keys 32 * tid ..)
    static_assert(WPT == 16, "the register arrays below assume 32 keys per thread");
    {
        uint4* z = reinterpret_cast<uint4*>(rcw + WPT * tid);
        z[0] = z[1] = z[2] = z[3] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    scan_hot_list(v.hot_xy, nraw, [&](uint32_t e) {
        const int b = band_key(e, k, w);
        if (b < kBandKeys) atomicAdd(&rcw[b >> 1], 1u << ((b & 1) * 16));  // (n <= 16384: a counter cannot carry)
    });
    __syncthreads();
    uint32_t wv[WPT + 2];
    {
        const uint4* src = reinterpret_cast<const uint4*>(rcw + WPT * tid);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 x = src[q];
            wv[4 * q] = x.x; wv[4 * q + 1] = x.y; wv[4 * q + 2] = x.z; wv[4 * q + 3] = x.w;
        }
        wv[WPT] = tid + 1 < CC_THREADS ? rcw[WPT * (tid + 1)] : 0u;  // the four keys after mine (the gap test)
        wv[WPT + 1] = tid + 1 < CC_THREADS ? rcw[WPT * (tid + 1) + 1] : 0u;
    }
    uint32_t mine = 0;
    unsigned long long emptym = 0;  // bit q: key 32 * tid + q holds no pixel
#pragma unroll
    for (int q = 0; q < WPT + 2; ++q) {
        const uint32_t lo = wv[q] & 0xffffu, hi = wv[q] >> 16;
        if (q < WPT) mine += lo + hi;
        emptym |= (unsigned long long)(lo == 0) << (2 * q) | (unsigned long long)(hi == 0) << (2 * q + 1);
    }
    // exclusive prefix of `mine` over the workgroup
    uint32_t incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if ((tid & 63) >= d) incl += o;
    }
    if ((tid & 63) == 63) part[tid >> 6] = incl;
    __syncthreads();
    uint32_t run = incl - mine, total = 0;
    for (int q = 0; q < CC_THREADS / 64; ++q) {
        if (q < (tid >> 6)) run += part[q];
        total += part[q];
    }
    const uint32_t start = run;  // pixels below key 32 * tid
#pragma unroll
    for (int q = 0; q < WPT; ++q) {
        const uint32_t lo = run, hi = run + (wv[q] & 0xffffu);
        cumw[WPT * tid + q] = lo | (hi << 16);  // (<= 16384: fits)
        run = hi + (wv[q] >> 16);
    }
    // a band may end at key r when keys r .. r + gap - 1 hold no pixel (keys past the frame hold none)
    const int gap = band_gap(k);
    unsigned long long sepm = emptym;
    for (int g = 1; g < gap; ++g) sepm &= emptym >> g;
    const uint32_t sep = (uint32_t)sepm;
    __syncthreads();
    int y0 = 0, nb = 0;
    while (true) {
        if (tid == 0) L.best = -1;
        __syncthreads();
        const uint32_t base = (cumw[y0 >> 1] >> ((y0 & 1) * 16)) & 0xffffu;
        int end = nkeys;
        if (total - base > (uint32_t)LN) {
            // the last key r > y0 the band [y0, r) may end at with at most LN hot pixels in it
            uint32_t ok = 0, below = start;  // pixels below key r
#pragma unroll
            for (int q = 0; q < 2 * WPT; ++q) {
                const int r = 2 * WPT * tid + q;
                ok |= (uint32_t)(r > y0 && r < nkeys && below - base <= (uint32_t)LN) << q;
                below += (q & 1) ? wv[q >> 1] >> 16 : wv[q >> 1] & 0xffffu;
            }
            ok &= sep;
            if (ok) atomicMax(&L.best, 2 * WPT * tid + 31 - __builtin_clz(ok));
            __syncthreads();
            end = L.best;
            if (end < 0) return 0;
        }
        if (tid == 0) L.band_y[nb] = y0;
        ++nb;
        y0 = end;
        if (end >= nkeys) break;
        if (nb == kMaxBands) return 0;
        __syncthreads();  // everybody has read L.best
    }
    if (tid == 0) { L.band_y[nb] = nkeys; L.nbands = nb; L.shear = k; }
    __syncthreads();
    return nb;
}

// Cut the frame into bands of at most LN hot pixels (see the top of this section): rows first, then sheared
// rows along the slopes of the upper and the lower edge of the hot pixels (a rotated board) and between them.
// Returns the number of bands, 0 (uniformly) when the frame cannot be banded.  All threads call it.
template <class LdsCC>
__device__ __noinline__ int lds_plan_bands(LdsCC& L, const FrameView& v, int nraw) {
    constexpr int LN = LdsCC::LN;
    const int tid = threadIdx.x, w = v.w, h = v.h;
    if (nraw <= LN) {
        if (tid == 0) { L.nbands = 1; L.band_y[0] = 0; L.band_y[1] = h; L.shear = 0; }
        __syncthreads();
        return 1;
    }
    if (nraw > LN * kMaxBands || h > kBandKeys) return 0;
    int nb = lds_try_bands(L, v, nraw, 0);
    if (nb) return nb;
    // upper / lower edge of the hot pixels in the left and in the right third of the frame
    if (tid < 4) L.edge[tid] = (tid & 1) ? 0u : 0xffffffffu;  // [0] min left, [1] max left, [2] min right, [3] max right
    __syncthreads();
    {
        uint32_t mn[2] = {0xffffffffu, 0xffffffffu}, mx[2] = {0u, 0u};
        scan_hot_list(v.hot_xy, nraw, [&](uint32_t e) {
            const int x = (int)(e & 0xffffu);
            const int side = 3 * x < w ? 0 : (3 * x >= 2 * w ? 1 : -1);
            if (side >= 0) {
                mn[side] = min(mn[side], e);
                mx[side] = max(mx[side], e);
            }
        });
        for (int sd = 0; sd < 2; ++sd) {
            if (mn[sd] != 0xffffffffu) atomicMin(&L.edge[2 * sd], mn[sd]);
            if (mx[sd] != 0u) atomicMax(&L.edge[2 * sd + 1], mx[sd]);
        }
    }
    __syncthreads();
    const uint32_t e0 = L.edge[0], e1 = L.edge[1], e2 = L.edge[2], e3 = L.edge[3];
    __syncthreads();
    if (e0 == 0xffffffffu || e2 == 0xffffffffu) return 0;  // nothing in one of the thirds: not a board that spans the frame
    auto slope32 = [](uint32_t a, uint32_t b) {  // shear that takes pixel a (left) and pixel b (right) to the same key
        const int dx = (int)(b & 0xffffu) - (int)(a & 0xffffu), dy = (int)(b >> 16) - (int)(a >> 16);
        int k = dx > 0 ? (-dy * 32 + (dy < 0 ? dx / 2 : -dx / 2)) / dx : 0;
        return k < -32 ? -32 : (k > 32 ? 32 : k);
    };
    const int kt = slope32(e0, e2), kb = slope32(e1, e3), km = (kt + kb) / 2;
    const int cand[9] = {km, kt, kb, km + 1, km - 1, kt + 1, kt - 1, kb + 1, kb - 1};
    for (int c = 0; c < 9; ++c) {
        const int k = cand[c];
        if (k == 0 || k < -32 || k > 32) continue;
        bool seen = false;
        for (int p = 0; p < c; ++p) seen = seen || cand[p] == k;
        if (seen) continue;
        nb = lds_try_bands(L, v, nraw, k);
        if (nb) return nb;
    }
    return 0;
}

// follow_connected_component (:236-256) on the LDS tables; the LIFO holds list indices.  The four neighbours of
// every entry have been looked up beforehand (lds_build_neighbours): a pop is two dependent LDS round trips
// (entry: value, position, neighbours; then the neighbours' values) instead of eleven through the hash map; the
// refine kernel's fills went from 58 to 36 us per launch with it (level 0 of the bench frames).
constexpr uint32_t kNoNb = 0xfffu;  // 12 bits per neighbour: a list index (< 2048) or this
template <class LdsCC>
__device__ __forceinline__ int drain_nb(LdsCC& L, const uint32_t* nlo, const uint16_t* nhi, int w, int h, int16_t* stk, int sp,
                                        Blob& b) {
    b.srx = b.sry = b.sr = 0;
    b.npix = 0;
    b.rmax = 0;
    b.xpk = b.ypk = 0;
    b.touched = false;
    int consumed = 0;
    while (sp > 0) {
        const int i = stk[--sp];
        const int v = L.val[i];
        const uint32_t e = L.xy[i];
        const uint32_t lo = nlo[i], hi = nhi[i];
        if (v <= 0) continue;  // visited already
        const int x = (int)(e & 0xffffu), y = (int)(e >> 16);
        const uint32_t jxp = lo & 0xfffu, jxm = (lo >> 12) & 0xfffu, jyp = (lo >> 24) | ((hi & 0xfu) << 8), jym = hi >> 4;
        // the neighbours' values do not depend on v: read together
        const int vxp = jxp != kNoNb ? (int)L.val[jxp] : 0, vxm = jxm != kNoNb ? (int)L.val[jxm] : 0;
        const int vyp = jyp != kNoNb ? (int)L.val[jyp] : 0, vym = jym != kNoNb ? (int)L.val[jym] : 0;
        L.val[i] = 0;  // :245 / :250
        ++consumed;    // every listed pixel is hot
        if (!(v > (b.rmax >> 4))) continue;                    // :159-171 with :27 (v > 15 holds)
        if (v > b.rmax) { b.rmax = v; b.xpk = x; b.ypk = y; }  // :176-181, first maximum wins
        b.srx += (unsigned long long)(v * x);
        b.sry += (unsigned long long)(v * y);
        b.sr += (unsigned long long)v;
        b.npix++;
        // :252-255 then :216-226; a neighbour is worth pushing only while it is hot and unvisited
        if (x + 1 >= w - kMargin) b.touched = true;
        else if (vxp > 0) stk[sp++] = (int16_t)jxp;
        if (x - 1 < kMargin) b.touched = true;
        else if (vxm > 0) stk[sp++] = (int16_t)jxm;
        if (y + 1 >= h - kMargin) b.touched = true;
        else if (vyp > 0) stk[sp++] = (int16_t)jyp;
        if (y - 1 < kMargin) b.touched = true;
        else if (vym > 0) stk[sp++] = (int16_t)jym;
    }
    return consumed;
}

// The neighbour table of drain_nb: 48 bits per entry (+x, -x, +y, -y at 12 bits each), the low 32 over the hash
// map (which must be dead, and a barrier behind its last reader), the high 16 wherever the caller has 2 bytes per
// entry to spare (refine: the labels; detect: the front of the LIFO space).  The loader has looked the neighbours up
// for the labelling already and parked them in global scratch; every thread fetches its own entries back (one
// coalesced round trip: 2-3 us where looking them up a second time took 9-25).  All threads call it.
template <class LdsCC>
__device__ __forceinline__ void lds_build_neighbours(LdsCC& L, const FrameView& v, int n, uint16_t* nhi) {
    constexpr int LEPT = LdsCC::LEPT;
    static_assert(sizeof(L.hashw) >= (size_t)LdsCC::LN * 4, "32 bits per entry over the hash map");
    static_assert(LdsCC::LN <= (int)kNoNb, "12-bit list indices");
    const int tid = threadIdx.x;
    const uint2* parked = reinterpret_cast<const uint2*>(v.arena);
    uint32_t* nlo = L.hashw;
    static_assert(LEPT % 4 == 0, "four entries at a time");
#pragma unroll
    for (int k0 = 0; k0 < LEPT; k0 += 4) {
        uint2 p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + CC_THREADS * (k0 + k);
            p[k] = i < n ? parked[i] : make_uint2(0, 0);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + CC_THREADS * (k0 + k);
            if (i < n) {
                nlo[i] = p[k].x;
                nhi[i] = (uint16_t)p[k].y;
            }
        }
    }
    __syncthreads();
}

// Load the hot pixels with band keys in [y0, y1) (`banded`; otherwise the whole list as it stands) into LDS,
// label the super-components (lab = smallest list index) and leave in L.u.acc, at every root, (pixels of the
// super-component) | (sum of hot-neighbour counts << 13): the latter bounds the pushes of any fill of it.
// n = entries loaded.  Returns false (uniformly) when they do not fit.  All threads call it.
// Window mode of the loader (refinement of frames with far more hot pixels than the tables hold -- a textured
// scene): only the hot pixels in the CELLS around the points to refine are loaded.  `WinSel` is a bitmap over cells
// of 2^cs x 2^cs pixels (cw cells per row); the cell of every refinable point and its eight neighbours are marked, so
// a point's 3x3 seeds are at least 2^cs pixels away from the edge of what is loaded.  A super-component that
// reaches that edge -- a member with a hot 4-neighbour in an unmarked cell -- is flagged "open" at its root
// (`openbits`); the caller declines the frame if a seed falls into an open one (its fill could leave the loaded
// set).  Everything else about the search only ever looks at the super-components of the seeds, so leaving the
// rest of the frame's hot pixels out changes nothing.
struct WinSel {
    const uint32_t* bits;  // LDS
    uint32_t* openbits;    // LDS, LN bits
    int cs;                // cells of 2^cs pixels, on the grid that starts at pixel (0, 0); -1: no selection
    int ox, oy, cw, chh;   // the bitmap covers cells ox .. ox + cw - 1, oy .. oy + chh - 1 (nothing outside is marked)
    // BOXED = false: the bitmap spans the frame from cell (0, 0) (the dense schedule's selection): no bounds to check,
    // and the kernel that only ever asks this way does not keep the span in registers.  BOXED = true is a level of a
    // sparse chain: the dense response only holds the marked cells, and a neighbour in an unmarked cell is taken to be
    // hot.  (A template parameter, not a flag in here: as a run-time flag in the two scans over a textured frame's 6e4
    // hot pixels it cost the dense schedule 95 us per refinement launch.)
    template <bool BOXED>
    __device__ __forceinline__ bool marked(int x, int y) const {
        int c;
        if (!BOXED) {
            c = (y >> cs) * cw + (x >> cs);
        } else {
            const int cx = (x >> cs) - ox, cy = (y >> cs) - oy;
            if ((unsigned)cx >= (unsigned)cw || (unsigned)cy >= (unsigned)chh) return false;
            c = cy * cw + cx;
        }
        return (bits[c >> 5] >> (c & 31)) & 1u;
    }
};

template <bool BOXED = false, class LdsCC>
__device__ __forceinline__ bool lds_load_and_label(LdsCC& L, const FrameView& v, int nraw, int cap, bool banded, int y0,
                                                   int y1, int& n, const WinSel* win = nullptr, bool preloaded = false) {
    constexpr int LN = LdsCC::LN, LHASH = LdsCC::LHASH, LEPT = LdsCC::LEPT;
    const int tid = threadIdx.x;
    n = 0;
    if (win) banded = true;  // a selection out of the frame's list, like a band
    if (nraw > cap || (!banded && nraw > LN)) return false;
    const int w = v.w;
    for (int k = tid; k < LHASH / 2; k += CC_THREADS) L.hashw[k] = 0xffffffffu;
    const int shear = L.shear;
    if (tid == 0) { L.nroots = 0; L.top = 0; L.total = 0; L.changed = 0; L.mtop = 0; L.nload = 0; L.leak = 0; }
    __syncthreads();
    if (preloaded) {  // (sparse refinement: the whole frame's pixels, all in marked cells, are in L.xy already)
        n = nraw;
    } else if (banded) {
        scan_hot_list(v.hot_xy, nraw, [&](uint32_t e) {
            bool take = true;
            if (win) take = win->template marked<BOXED>((int)(e & 0xffffu), (int)(e >> 16));
            // (BOXED: cells AND a band for a frame of a sparse level whose cells hold more than the tables)
            if (!win || (BOXED && y1 > y0)) {
                const int y = band_key(e, shear, w);
                take = take && y >= y0 && y < y1;
            }
            if (take) {
                const int slot = atomicAdd(&L.nload, 1);
                if (slot < LN) L.xy[slot] = e;
            }
        });
        __syncthreads();
        n = L.nload;
        if (n > LN) return false;  // bands: the planner counted the same pixels, cannot happen; windows: too many
    } else {
        n = nraw;
    }
    uint32_t own[LEPT];
#pragma unroll
    for (int k = 0; k < LEPT; ++k) {
        const int i = tid + CC_THREADS * k;
        own[k] = kHotDead;
        if (i < n) {
            const uint32_t e = banded ? L.xy[i] : v.hot_xy[i];
            own[k] = e;
            L.xy[i] = e;
            L.lab[i] = (int16_t)i;
            L.u.acc[i] = 0;
            if (e != kHotDead) {
                L.val[i] = v.d[(int)(e >> 16) * w + (int)(e & 0xffffu)];
                lds_insert(L, e, i);
            } else {
                L.val[i] = 0;
            }
        }
    }
    __syncthreads();
    // the four neighbours of every entry, 12 bits each (kNoNb = none), packed like the table of drain_nb
    uint32_t nlo[LEPT];
    uint16_t nhi[LEPT];
#pragma unroll
    for (int k = 0; k < LEPT; ++k) {
        const uint32_t e = own[k];
        int f[4] = {-1, -1, -1, -1};
        if (e != kHotDead) lds_find4(L, e, f);
        uint32_t j[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) j[q] = f[q] < 0 ? kNoNb : (uint32_t)f[q];
        nlo[k] = j[0] | (j[1] << 12) | (j[2] << 24);
        nhi[k] = (uint16_t)((j[2] >> 8) | (j[3] << 4));
        // parked for lds_build_neighbours (same thread, same entries) in the LIFO arena of the global-memory
        // kernels, which nothing uses while a frame is searched out of LDS: 2 words per entry of >= 16384
        const int i = tid + CC_THREADS * k;
        if (i < n) reinterpret_cast<uint2*>(v.arena)[i] = make_uint2(nlo[k], nhi[k]);
    }
    auto nb_of = [&](int k, int q) -> uint32_t {  // q static after unrolling
        return q == 0 ? nlo[k] & 0xfffu : q == 1 ? (nlo[k] >> 12) & 0xfffu
             : q == 2 ? (nlo[k] >> 24) | (((uint32_t)nhi[k] & 0xfu) << 8) : (uint32_t)nhi[k] >> 4;
    };
    // min-label propagation with shortcutting; labels only ever decrease and always name a member of
    // the same super-component, so unsynchronised reads within a round are harmless
    while (true) {
        bool ch = false;
#pragma unroll
        for (int k = 0; k < LEPT; ++k) {
            if (own[k] == kHotDead) continue;
            const int i = tid + CC_THREADS * k;
            const int cur = L.lab[i];
            int m = cur;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t jq = nb_of(k, q);
                if (jq != kNoNb) m = min(m, (int)L.lab[jq]);
            }
            m = min(m, (int)L.lab[m]);
            if (m < cur) { L.lab[i] = (int16_t)m; ch = true; }
        }
        if (ch) L.changed = 1;
        __syncthreads();
        const int c = L.changed;
        __syncthreads();
        if (!c) break;
        if (tid == 0) L.changed = 0;
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < LEPT; ++k) {
        if (own[k] == kHotDead) continue;
        const int i = tid + CC_THREADS * k;
        int deg = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) deg += nb_of(k, q) != kNoNb;
        atomicAdd(&L.u.acc[L.lab[i]], 1 + (deg << 13));
    }
    __syncthreads();
    if (win) {
        // open super-components (a pass of its own, rolled: the unrolled loops above hold eight entries' state in
        // registers).  A neighbour that is not in the list is either not hot (its cell is loaded) or was not loaded;
        // the neighbours come back from where the loop above parked them.
        const uint2* parked = reinterpret_cast<const uint2*>(v.arena);
#pragma unroll 1
        for (int i = tid; i < n; i += CC_THREADS) {
            const uint32_t e = L.xy[i];
            if (e == kHotDead) continue;
            const uint2 pk = parked[i];
            const uint32_t nb[4] = {pk.x & 0xfffu, (pk.x >> 12) & 0xfffu, (pk.x >> 24) | ((pk.y & 0xfu) << 8), (pk.y >> 4) & 0xfffu};
            const int x = (int)(e & 0xffffu), y = (int)(e >> 16);
            bool open = false;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int nx = x + (q == 0) - (q == 1), ny = y + (q == 2) - (q == 3);
                if (nb[q] == kNoNb && nx >= 0 && nx < w && ny >= 0 && ny < v.h && !win->template marked<BOXED>(nx, ny) &&
                    (BOXED || v.d[ny * w + nx] > kRespMin))  // (BOXED: a sparse level, nothing computed there -- taken to be hot)
                    open = true;
            }
            if (open) {
                const int r = L.lab[i];
                atomicOr(&win->openbits[r >> 5], 1u << (r & 31));
            }
        }
        __syncthreads();
    }
    return true;
}

}  // namespace mrg
