// The cells of a sparse level: which ones to compute (cell lists, subsets of points) and their hot pixels afterwards.
#pragma once
#include "cc_lds.h"

namespace mrg {

// Marks the cells around the refinable points of a frame (see WinSel).  All threads call these.
// TIGHT (sparse refinement): the cells that overlap the square of half a cell around every seed instead of the
// seed's cell and its eight neighbours -- at most 2 x 2 per seed, a seed is then >= 2^(cs-1) pixels from the
// edge of what is marked -- and the bitmap only spans the box around the points, which buys cells of 16 pixels
// instead of 32 for a board that fills a quarter of a 12 MP frame (the response is computed in every marked cell).
struct NoCellSink { __device__ __forceinline__ void operator()(int, int, int) const {} };
// A listed cell: (cell y << 16) | (subset << 12) | cell x -- cells are >= 16 pixels, a side is < 32768, so x and y are < 2048;
// the subset (0 .. kSubsets - 1) is the workgroup of the refinement kernel that owns the cell (below: "Several workgroups").
__device__ __forceinline__ int cell_x(uint32_t c) { return (int)(c & 0xfffu); }
__device__ __forceinline__ int cell_y(uint32_t c) { return (int)(c >> 16); }
__device__ __forceinline__ int cell_sub(uint32_t c) { return (int)((c >> 12) & 0xfu); }
constexpr int kWinWords = 1280;  // cell bitmap: 40 960 cells (sizeof(LdsCCT<2048>::w) / 4)

// the nine seed positions of point i exactly as the seeding loop forms them (int16 conversions of is_valid included)
template <class F>
__device__ __forceinline__ void for_each_seed(int w, int h, const double* pts, int i, int level, F f) {
    const uint16_t coord_scale = (uint16_t)(1u << level);
    const double lx = rescale_coord(pts[2 * i + 0], 1.0 / coord_scale);
    const double ly = rescale_coord(pts[2 * i + 1], 1.0 / coord_scale);
    const int x = (int)(lx + 0.5), y = (int)(ly + 0.5);
    for (int sdx = -1; sdx <= 1; ++sdx)
        for (int sdy = -1; sdy <= 1; ++sdy) {
            const int sx = (int16_t)(x + sdx), sy = (int16_t)(y + sdy);
            if (sx >= 0 && sx < w && sy >= 0 && sy < h) f(sx, sy);
        }
}

// Cell size and span of the bitmap for the pixel box [x0, x1] x [y0, y1] that the seeds can reach.  cs = -1: the bitmap
// cannot hold it.
__device__ __forceinline__ void win_cells_of_box(WinSel& ws, int x0, int y0, int x1, int y1, int max_words, bool TIGHT) {
    ws.cs = TIGHT ? 4 : 5;
    while (true) {
        const int half = TIGHT ? 1 << (ws.cs - 1) : 0;
        ws.ox = max(x0 - half, 0) >> ws.cs;
        ws.oy = max(y0 - half, 0) >> ws.cs;
        ws.cw = ((x1 + half) >> ws.cs) - ws.ox + 1;
        ws.chh = ((y1 + half) >> ws.cs) - ws.oy + 1;
        if ((ws.cw * ws.chh + 31) / 32 <= max_words) break;
        if (++ws.cs > 15) { ws.cs = -1; break; }
    }
}

// Geometry: cell size and the span of the bitmap.  `box` = 4 words of LDS.  cs = -1: the bitmap cannot hold the frame.
__device__ __forceinline__ WinSel win_geometry(int w, int h, const double* pts, const signed char* lv, int npts, int level,
                                               int max_words, bool TIGHT, uint32_t* box) {
    WinSel ws;
    ws.bits = nullptr;
    ws.openbits = nullptr;
    int x0 = 0, y0 = 0, x1 = w - 1, y1 = h - 1;  // pixels the marked cells can reach
    if (TIGHT) {
        if (threadIdx.x < 4) box[threadIdx.x] = (threadIdx.x & 1) ? 0u : 0xffffffffu;  // min x, max x, min y, max y
        __syncthreads();
        uint32_t mnx = 0xffffffffu, mxx = 0, mny = 0xffffffffu, mxy = 0;
        for (int i = threadIdx.x; i < npts; i += CC_THREADS) {
            if (lv[i] != level + 1) continue;
            for_each_seed(w, h, pts, i, level, [&](int sx, int sy) {
                mnx = min(mnx, (uint32_t)sx); mxx = max(mxx, (uint32_t)sx);
                mny = min(mny, (uint32_t)sy); mxy = max(mxy, (uint32_t)sy);
            });
        }
        if (mnx != 0xffffffffu) {
            atomicMin(&box[0], mnx); atomicMax(&box[1], mxx);
            atomicMin(&box[2], mny); atomicMax(&box[3], mxy);
        }
        __syncthreads();
        const uint32_t b0 = box[0], b1 = box[1], b2 = box[2], b3 = box[3];
        __syncthreads();
        if (b0 == 0xffffffffu) { x0 = y0 = 0; x1 = y1 = 0; }  // nothing to refine: one cell
        else { x0 = (int)b0; x1 = (int)b1; y0 = (int)b2; y1 = (int)b3; }
    }
    win_cells_of_box(ws, x0, y0, x1, y1, max_words, TIGHT);
    return ws;
}

// Marking, with the geometry given: `bits` must hold (cw * chh + 31) / 32 words.  `sink(cell x, cell y)` (cells on
// the frame's grid) is called by the thread that sets a cell's bit first.
// `psub` != NULL: only the points of subset `sub` (psub[i] == sub) mark.  `outside` (one word of LDS, or NULL): the mask value 4
// is OR-ed in when a cell a seed reaches lies outside the span.
template <int LNBITS, class Sink = NoCellSink>
__device__ __forceinline__ void win_mark(WinSel& ws, int w, int h, const double* pts, const signed char* lv, int npts, int level,
                                         uint32_t* bits, uint32_t* openbits, bool TIGHT, Sink sink = Sink(),
                                         const int32_t* psub = nullptr, int sub = 0, int* outside = nullptr) {
    ws.bits = bits;
    ws.openbits = openbits;
    const int nw = (ws.cw * ws.chh + 31) / 32;
    for (int k = threadIdx.x; k < nw; k += CC_THREADS) bits[k] = 0;
    if (openbits)
        for (int k = threadIdx.x; k < LNBITS / 32; k += CC_THREADS) openbits[k] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < npts; i += CC_THREADS) {
        if (lv[i] != level + 1) continue;
        if (psub && psub[i] != sub) continue;
        for_each_seed(w, h, pts, i, level, [&](int sx, int sy) {
            const int half = 1 << (ws.cs - 1);
            const int ax0 = TIGHT ? max(sx - half, 0) >> ws.cs : (sx >> ws.cs) - 1;
            const int ax1 = TIGHT ? (sx + half) >> ws.cs : (sx >> ws.cs) + 1;
            const int ay0 = TIGHT ? max(sy - half, 0) >> ws.cs : (sy >> ws.cs) - 1;
            const int ay1 = TIGHT ? (sy + half) >> ws.cs : (sy >> ws.cs) + 1;
            for (int ay = ay0; ay <= ay1; ++ay)
                for (int ax = ax0; ax <= ax1; ++ax) {
                    const int cx = TIGHT ? ax - ws.ox : ax, cy = TIGHT ? ay - ws.oy : ay;  // (not TIGHT: the span starts at cell (0, 0))
                    if ((unsigned)cx >= (unsigned)ws.cw || (unsigned)cy >= (unsigned)ws.chh) {
                        // a span that was not made from these points (a split level's, list_cells_split): the cell cannot
                        // be listed, the seeds in it would look "not hot" -- the caller gives the frame up instead
                        if (outside) atomicOr(outside, 4);
                        continue;
                    }
                    const int c = cy * ws.cw + cx;
                    const uint32_t bit = 1u << (c & 31);
                    if (!(bits[c >> 5] & bit) && !(atomicOr(&bits[c >> 5], bit) & bit)) sink(ax, ay, i);
                }
        });
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------
// Several workgroups per frame (round 5).  The refinement of a sparse level is a latency chain whose length grows with the
// frame's hot pixels and points (tools/sparse_phases.py: a 5x5 board's frame takes 53 us, a 10x10's 95, a 14x14's 245), and
// one workgroup per frame leaves the chip 94 % empty.  Points whose marked cells do not touch cannot share a
// super-component (a fill never leaves the 4-connected hot region of its seeds, find_chessboard_corners.cc:356-397, and a
// region that reaches an unmarked cell is "open": the frame is given up), so a frame's points are cut into up to kSubsets
// SUBSETS that are far enough apart, every listed cell carries the subset of the point that marked it, and workgroup
// (frame, s) of the refinement kernel loads the cells, seeds the points and fills the components of subset s alone --
// outputs go to the points' own slots, so the order of the list is untouched.
//   * The cut is made by a workgroup that owns the whole frame (sparse_cells_kernel for the first sparse level, the
//     refinement kernel of the level above while it is not split): a point with no other point within kLinkDist pixels (at
//     the level's coordinates, either axis) can go to any subset, all the others stay together in subset 0.  At 16-pixel
//     cells the cells of a point lie within 24 pixels of it: points >= 64 apart have cells that do not even touch.
//   * A split level hands ITS subsets on to the next level (nobody sees the whole frame any more) after checking that
//     they stay apart: a point's refined position lies inside its marked cells, i.e. within 24 pixels of where it was;
//     each workgroup compares its own refined points with every point of the other subsets (read while those workgroups
//     may still be writing: old or new position) and asks for ONE workgroup at the next level (kFlagSingle) when any pair
//     is closer than kKeepDist -- 48.5 for cells that stay disjoint whatever the other point does, a cell more to be sure.
//   * Cells of more than 16 pixels (a box of more than 40 960 cells), fewer than kSplitMinPoints points, a single
//     cluster: one workgroup, as before.  A subset whose cells hold more hot pixels than the tables gives the frame up
//     (the dense repeat takes it), like every other case the LDS kernel cannot take.
// Header of a level's list, kCellHdr words per frame: [0] cells (-1: given up), [1] log2 cell size, [2..5] span of the
// bitmap, [6] subsets (<= 1: one workgroup), [7] flags.  sparse_cells_kernel zeroes [0], [6], [7] of every level below
// the first; a split level ADDS its cells to [0].
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kSubsets = 4;
constexpr int kHdrSub = 6, kHdrFlags = 7;
constexpr int kFlagGivenUp = 1, kFlagSingle = 2;
constexpr int kSplitMinPoints = 128;  // (a 10x10 board: one workgroup is faster -- more workgroups in flight slow the pixel stream by more than the shorter chain gains; 14x14: -15 %)
constexpr float kLinkDist = 64.f, kKeepDist = 64.f;

struct PartScratch {  // LDS of partition_points
    float x[LPTS], y[LPTS];
    int16_t lab[LPTS];
    int nroots, nlive;
};

// Subsets of the points to refine at `level` (lv[i] == level + 1), from their positions now: psub[i] for every point of the
// frame (0 for the others), returns how many subsets (uniform; 1 = no cut).  All threads of the workgroup.
__device__ __forceinline__ int partition_points(const double* pts, const signed char* lv, int npts, int level, int32_t* psub,
                                                PartScratch& S, int max_sub) {
    const int tid = threadIdx.x;
    if (npts > LPTS || max_sub < 2) {
        for (int i = tid; i < npts; i += CC_THREADS) psub[i] = 0;
        return 1;
    }
    const float inv = 1.0f / (float)(1 << level);
    if (tid == 0) { S.nroots = 0; S.nlive = 0; }
    __syncthreads();
    for (int i = tid; i < npts; i += CC_THREADS) {
        const bool live = lv[i] == level + 1;
        S.x[i] = live ? ((float)pts[2 * i] + 0.5f) * inv : 1e30f;
        S.y[i] = live ? ((float)pts[2 * i + 1] + 0.5f) * inv : 1e30f;
        S.lab[i] = (int16_t)i;
        if (live) atomicAdd(&S.nlive, 1);
    }
    __syncthreads();
    const int nlive = S.nlive;
    if (nlive < kSplitMinPoints) {  // (uniform)
        for (int i = tid; i < npts; i += CC_THREADS) psub[i] = 0;
        return 1;
    }
    // No clustering proper: a point with no other point within kLinkDist is a subset candidate of its own, ALL the others
    // go together (several clusters in one subset are as good as one; label propagation over a board whose points are all
    // linked -- a coarse level -- took 80 us of a 100-us kernel).  One pass over the pairs.
    for (int i = tid; i < npts; i += CC_THREADS) {
        const float xi = S.x[i], yi = S.y[i];
        if (xi > 1e29f) { S.lab[i] = -1; continue; }
        bool linked = false;
        for (int j = 0; j < npts; ++j)
            linked |= j != i && fabsf(S.x[j] - xi) < kLinkDist && fabsf(S.y[j] - yi) < kLinkDist;
        S.lab[i] = linked ? 1 : 0;   // -1 not to be refined, 0 on its own, 1 with the rest
        if (linked) atomicAdd(&S.nroots, 1);
    }
    __syncthreads();
    const int nrest = S.nroots, niso = nlive - nrest;
    int nsub = min(min(kSubsets, max_sub), niso + (nrest > 0 ? 1 : 0));
    if (nsub < 2) nsub = 1;
    // the rest is subset 0; the points on their own are dealt out so that the subsets come out even
    const bool rest_full = nrest * nsub >= nlive;
    for (int i = tid; i < npts; i += CC_THREADS) {
        int sb = 0;
        if (S.lab[i] == 0 && nsub > 1) {
            int r = 0;
            for (int j = 0; j < i; ++j) r += S.lab[j] == 0;
            sb = rest_full ? 1 + r % (nsub - 1) : (r + nrest) % nsub;
        }
        psub[i] = sb;
    }
    __threadfence_block();
    __syncthreads();
    return nsub > 1 ? nsub : 1;
}

// Sparse refinement, step 1: the cells around the points of a frame to refine at `level`, as a list for the kernel
// that computes the response there (chess_cells_kernel): cnt[0] = how many (-1: more than the list or the mask area
// holds, the refinement kernel reports the frame), cnt[1] = their size (log2), cnt[2..5] = the span of the bitmap,
// list = (cell y << 16) | (subset << 12) | cell x.  The refinement kernel marks exactly the listed cells for itself.  All
// threads of the workgroup, which owns the WHOLE frame; `bits` = kWinWords words, `box` = 4 words, `n` = one word of LDS.
// `psub` / `nsub`: the cut of partition_points (nsub <= 1: none); cells of more than 16 pixels are not cut.
__device__ __forceinline__ void list_cells(int w, int h, const double* pts, const signed char* lv, int npts, int level,
                                           uint32_t* bits, uint32_t* box, int* n, uint32_t* list, int list_pitch,
                                           long long max_items, int32_t* cnt, const int32_t* psub = nullptr, int nsub = 1) {
    if (threadIdx.x == 0) *n = 0;
    WinSel ws = win_geometry(w, h, pts, lv, npts, level, kWinWords, true, box);  // (a barrier first: *n is 0 below)
    const bool cut = nsub > 1 && ws.cs == 4;
    auto sink = [&](int ax, int ay, int i) {
        const int k = atomicAdd(n, 1);
        if (k < list_pitch) list[k] = ((uint32_t)ay << 16) | (cut ? (uint32_t)psub[i] << 12 : 0u) | (uint32_t)ax;
    };
    if (ws.cs >= 0) win_mark<2048>(ws, w, h, pts, lv, npts, level, bits, nullptr, true, sink);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int k = *n;
        const bool ok = ws.cs >= 0 && k <= list_pitch && ((long long)k << (2 * (ws.cs - 4))) <= max_items;
        cnt[0] = ok ? k : -1;
        cnt[1] = ws.cs;
        cnt[2] = ws.ox; cnt[3] = ws.oy; cnt[4] = ws.cw; cnt[5] = ws.chh;
        cnt[kHdrSub] = cut ? nsub : 1;
        cnt[kHdrFlags] = ok ? 0 : kFlagGivenUp;
    }
}

// The same by workgroup `sub` of a SPLIT level, for the next level down: the cells of its own points, ADDED to the list the
// workgroups of the frame share (cnt[0], zero before the kernel); the geometry every workgroup must agree on comes from this
// level's span (`hdr`: a refined point lies inside the cells that were marked for it, so twice the span holds every seed of
// the next level); the subsets are kept if they stay apart (see above), else the next level runs as one workgroup.
// `tmp`: LDS, `tmp_cap` words.
__device__ __forceinline__ void list_cells_split(int w, int h, const double* pts, const signed char* lv, int npts, int level,
                                                 uint32_t* bits, int* n, uint32_t* tmp, int tmp_cap, const int32_t* hdr,
                                                 uint32_t* list, int list_pitch, long long max_items, int32_t* cnt,
                                                 const int32_t* psub, int sub, int nsub) {
    const int tid = threadIdx.x;
    if (tid == 0) { n[0] = 0; n[1] = 0; }
    WinSel ws;
    ws.bits = nullptr;
    ws.openbits = nullptr;
    {
        const int pcs = hdr[1], X0 = hdr[2] << pcs, Y0 = hdr[3] << pcs, X1 = ((hdr[2] + hdr[4]) << pcs) - 1, Y1 = ((hdr[3] + hdr[5]) << pcs) - 1;
        win_cells_of_box(ws, max(2 * X0 - 2, 0), max(2 * Y0 - 2, 0), min(2 * X1 + 3, w - 1), min(2 * Y1 + 3, h - 1), kWinWords, true);
    }
    __syncthreads();
    auto sink = [&](int ax, int ay, int) {
        const int k = atomicAdd(&n[0], 1);
        if (k < tmp_cap) tmp[k] = ((uint32_t)ay << 16) | ((uint32_t)sub << 12) | (uint32_t)ax;
    };
    if (ws.cs >= 0) win_mark<2048>(ws, w, h, pts, lv, npts, level, bits, nullptr, true, sink, psub, sub, &n[1]);
    // do the subsets stay apart?  own points as they are now against every point of the others (level + 1 coordinates: the
    // level this kernel has just refined).  n[1], mask values: 1 = a pair closer than kKeepDist -> one workgroup at the next level;
    // 2 = a pair so close that both can mark the SAME cell (a cell of 2^cs pixels is marked by seeds up to half a cell
    // beyond either edge: seeds less than 2 * 2^cs apart at this level, i.e. points less than 2^cs (+ rounding and the
    // seed ring) apart at level + 1) -- every workgroup keeps a bitmap of its own, so the shared list would then hold the
    // cell twice and the one workgroup of the next level would expand its hot pixels twice: the frame is given up (the
    // dense repeat takes it); 4 = a seed's cell outside the span the workgroups agreed on (win_mark).
    {
        const float inv = 1.0f / (float)(2 << level);
        const float dup = ws.cs >= 0 ? (float)(1 << min(ws.cs, 15)) + 2.f : 0.f;
        bool close = false, twice = false;
        for (int i = tid; i < npts; i += CC_THREADS) {
            if (psub[i] != sub || lv[i] != level + 1) continue;
            const float xi = ((float)pts[2 * i] + 0.5f) * inv, yi = ((float)pts[2 * i + 1] + 0.5f) * inv;
            for (int j = 0; j < npts; ++j)
                if (psub[j] != sub && lv[j] <= level + 2) {  // (lv > level + 2: never refined again)
                    const float dx = fabsf(((float)pts[2 * j] + 0.5f) * inv - xi), dy = fabsf(((float)pts[2 * j + 1] + 0.5f) * inv - yi);
                    close |= dx < kKeepDist && dy < kKeepDist;
                    twice |= dx < dup && dy < dup;
                }
        }
        if (close || twice) atomicOr(&n[1], (close ? 1 : 0) | (twice ? 2 : 0));
    }
    __syncthreads();
    const int k = n[0];
    __syncthreads();
    if (tid == 0) {
        int flags = (ws.cs != 4 || (n[1] & 1)) ? kFlagSingle : 0;
        int base = 0;
        if (ws.cs < 0 || k > tmp_cap || (n[1] & 6)) {
            flags |= kFlagGivenUp;
        } else {
            base = atomicAdd(&cnt[0], k);
            if (base + k > list_pitch || ((long long)(base + k) << (2 * (ws.cs - 4))) > max_items) flags |= kFlagGivenUp;
        }
        if (flags) atomicOr(&cnt[kHdrFlags], flags);
        cnt[1] = ws.cs;  // (the same values from every workgroup of the frame)
        cnt[2] = ws.ox; cnt[3] = ws.oy; cnt[4] = ws.cw; cnt[5] = ws.chh;
        cnt[kHdrSub] = nsub;
        n[0] = (flags & kFlagGivenUp) ? -1 : base;
    }
    __syncthreads();
    const int base = n[0];
    if (base >= 0)
        for (int q = tid; q < k; q += CC_THREADS) list[base + q] = tmp[q];
}

// Sparse refinement, step 3a: the hot pixels of a frame out of the masks chess_cells_kernel left (32 bytes per 16 x 16
// micro-tile, byte 2 * row + half = the 8 pixels x .. x + 7).  One workgroup per frame, no counter shared with
// anybody.  The entries go straight into the LDS list (`lds_xy`, `lds_cap` entries: the frame is then loaded, see
// lds_load_and_label's `preloaded`); only if there are more -- a frame that needs bands -- a second pass writes the
// global list the band planner and the loader read, like a dense level's.  Returns the number of hot pixels
// (uniform), -1 when the frame was given up by whoever listed the cells.  `cnt` = one word of LDS.
// `only` >= 0: the cells of that subset alone (a split level).
template <class Put>
__device__ __forceinline__ void expand_masks(const uint32_t* masks, const uint32_t* list, int nwords, int cs, int* cnt, Put put,
                                             int only = -1) {
    const int sub = cs - 4;
    constexpr int U = 8;  // (a clean 10x10 board at 16-pixel cells: ~3800 words, two rounds of 256 x 8)
    for (int k0 = threadIdx.x; k0 < nwords; k0 += CC_THREADS * U) {
        uint32_t m[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + u * CC_THREADS;
            m[u] = (k < nwords && (only < 0 || cell_sub(list[(k >> 3) >> (2 * sub)]) == only)) ? masks[k] : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!m[u]) continue;
            const int k = k0 + u * CC_THREADS, it = k >> 3, j = k & 7;
            const uint32_t c = list[it >> (2 * sub)];
            const int si = it & ((1 << (2 * sub)) - 1);
            const int xt = (cell_x(c) << cs) + 16 * (si & ((1 << sub) - 1));
            const int yt = (cell_y(c) << cs) + 16 * (si >> sub);
            int slot = atomicAdd(cnt, __popc(m[u]));
            uint32_t mm = m[u];
            while (mm) {
                const int b = __ffs(mm) - 1;  // byte q = b >> 3: row 2j + (q >> 1), half q & 1; pixel b & 7 of its group
                mm &= mm - 1;
                const int q = b >> 3;
                put(slot++, ((uint32_t)(yt + 2 * j + (q >> 1)) << 16) | (uint32_t)(xt + 8 * (q & 1) + (b & 7)));
            }
        }
    }
}
// the cell bitmap of a frame straight from its list: what is marked IS what was computed
__device__ __forceinline__ void mark_listed_cells(const WinSel& ws, const uint32_t* list, int ncell, uint32_t* bits,
                                                  uint32_t* openbits, int nopen_words, int only = -1) {
    const int nw = (ws.cw * ws.chh + 31) / 32;
    for (int k = threadIdx.x; k < nw; k += CC_THREADS) bits[k] = 0;
    for (int k = threadIdx.x; k < nopen_words; k += CC_THREADS) openbits[k] = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < ncell; k += CC_THREADS) {
        const uint32_t c = list[k];
        if (only >= 0 && cell_sub(c) != only) continue;  // (another subset's cell: unmarked here, i.e. "not computed")
        const int cx = cell_x(c) - ws.ox, cy = cell_y(c) - ws.oy;
        if ((unsigned)cx < (unsigned)ws.cw && (unsigned)cy < (unsigned)ws.chh) {
            const int b = cy * ws.cw + cx;
            atomicOr(&bits[b >> 5], 1u << (b & 31));
        }
    }
    __syncthreads();
}
// -> number of hot pixels (uniform; -1: the frame was given up), `ws` = the selection (cells marked in `bits`)
// `only` >= 0 (a split level): the cells of that subset; `hot_xy` / `cap` are then the subset's part of the frame's global list.
__device__ __forceinline__ int hot_list_from_masks(const RefineIO& io, const CompTables& t, int frame, uint32_t* hot_xy, int cap, int* cnt,
                                                   uint32_t* lds_xy, int lds_cap, WinSel& ws, uint32_t* bits, uint32_t* openbits,
                                                   int nopen_words, int only = -1) {
    const int32_t* hdr = io.cell_cnt + kCellHdr * frame;
    const int ncell = (hdr[kHdrFlags] & kFlagGivenUp) ? -1 : hdr[0];
    ws.cs = hdr[1]; ws.ox = hdr[2]; ws.oy = hdr[3]; ws.cw = hdr[4]; ws.chh = hdr[5];
    ws.bits = bits;
    ws.openbits = openbits;
    if (threadIdx.x == 0) *cnt = 0;
    __syncthreads();
    if (ncell < 0 || ws.cs < 4 || (ws.cw * ws.chh + 31) / 32 > kWinWords) return -1;
    const int nwords = (ncell << (2 * (ws.cs - 4))) * 8;
    const uint32_t* list = io.cell_list + (long long)frame * io.list_pitch;
    const uint32_t* masks = reinterpret_cast<const uint32_t*>(t.gidx + (long long)frame * t.gidx_pitch);
    mark_listed_cells(ws, list, ncell, bits, openbits, nopen_words, only);
    expand_masks(masks, list, nwords, ws.cs, cnt, [&](int slot, uint32_t e) { if (slot < lds_cap) lds_xy[slot] = e; }, only);
    __syncthreads();
    const int n = *cnt;
    __syncthreads();
    if (n <= lds_cap) return n;
    if (threadIdx.x == 0) *cnt = 0;
    __syncthreads();
    expand_masks(masks, list, nwords, ws.cs, cnt, [&](int slot, uint32_t e) { if (slot < cap) hot_xy[slot] = e; }, only);
    __threadfence();  // the list is read back by other waves of this workgroup
    __syncthreads();
    return n;
}

}  // namespace mrg
