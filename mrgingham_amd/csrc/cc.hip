// The component search in global memory and the dense repeat of flagged frames (the method: cc_common.h).
#include "cc_common.h"

namespace mrg {

// P0, P1 and P2 open the global-memory kernels below, which run one 512-thread workgroup per frame (so that
// workgroup-scope atomics suffice, see above): at full resolution a noisy frame has tens of thousands
// of hot pixels, nearly all of them isolated, which P1 flags so that P2 skips them.  (They were a kernel of
// their own until the LDS path made these kernels the rare case: one launch per level less on the component
// stream, whose kernels mostly find their frames done and leave.)
// P0: reset the per-entry tables (the pixel kernel only writes the hot list and the pixel -> index
// map); P1: union-find over the hot list (left / up neighbours); P2: flatten (parent[i] = root of i),
// per-root pixel count, bounding box and smallest raster position.  Workgroup barriers in between; all
// threads of the workgroup call it.
__device__ __forceinline__ void label_frame(const FrameView& v) {
    const int w = v.w;
    for (int i = threadIdx.x; i < v.n; i += CCG_THREADS) {
        v.parent[i] = i;
        v.comp_cnt[i] = 0;
        v.comp_box[i] = make_int4(0x7fffffff, 0x7fffffff, -1, -1);
        v.roots[i] = 0x7fffffff;
        v.comp_first[i] = 0x7fffffff;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < v.n; i += CCG_THREADS) {
        const uint32_t e = v.hot_xy[i];
        if (e == kHotDead) continue;  // unused slot: flagged already (bit 31), P2 skips it
        const int x = (int)(e & 0xffffu), y = (int)(e >> 16);
        const int p = y * w + x;
        // all four neighbours lie inside the image (p is in [7,w-7) x [7,h-7)); the frame is zero
        const bool l = v.d[p - 1] > kRespMin, u = v.d[p - w] > kRespMin;
        const bool r = v.d[p + 1] > kRespMin, dn = v.d[p + w] > kRespMin;
        // the hot pixels of an aligned group of 8 are consecutive list entries in ascending x
        if (l) uf_unite(v.parent, i, (x & 7) ? i - 1 : hot_index_of(v.gidx, v.gw, x - 1, y));
        if (u) uf_unite(v.parent, i, hot_index_of(v.gidx, v.gw, x, y - 1));
        // An isolated hot pixel is a finished super-component of size one: flag it so that P2 does
        // not spend five atomics on it (at full resolution most hot pixels are isolated noise).
        if (!(l || u || r || dn)) v.hot_xy[i] = e | kHotSingleton;
    }
    __syncthreads();  // every union of the frame is done (the tables are only touched by this workgroup)
    for (int i = threadIdx.x; i < v.n; i += CCG_THREADS) {
        const uint32_t e = v.hot_xy[i];
        if (e & kHotSingleton) continue;  // its own root, count 0: never a blob, never shared
        const int r = uf_root(v.parent, i);
        // other threads may still walk through i: r is an ancestor, so their walks stay valid
        __hip_atomic_store(v.parent + i, r, MRG_WG);
        const int x = (int)(e & 0xffffu), y = (int)(e >> 16);
        int* box = reinterpret_cast<int*>(v.comp_box + r);
        wg_min(box + 0, x);
        wg_min(box + 1, y);
        wg_max(box + 2, x);
        wg_max(box + 3, y);
        wg_add(v.comp_cnt + r, 1);
        wg_min(v.comp_first + r, (int)e);  // (y << 16) | x orders like the raster index
    }
    __syncthreads();
}

// Hot list of a CALLER-SUPPLIED response (mrgingham_amd_cc_on_response_batch, the entry point the
// rule tests drive): copies it into the level scratch the way the component search expects it --
// negatives clamped to 0 (find_chessboard_corners.cc:527-529), the 7-pixel frame zero (:506) -- and
// appends the hot pixels exactly as the ChESS epilogue does (same list / map format).
// One wave = 64 aligned groups of 8 pixels of one row.
__global__ __launch_bounds__(256) void hot_from_response_kernel(const int16_t* src, LevelBatch lb, CompTables t,
                                                                int frame0) {
    const int frame = frame0 + blockIdx.z;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= lb.h) return;  // wave-uniform
    const int w = lb.w, h = lb.h;
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 8;
    const int16_t* in = src + (long long)frame * w * h + (long long)y * w;
    int16_t* out = lb.resp + (long long)frame * lb.resp_pitch + (long long)y * w;
    const bool row_in = y >= kMargin && y < h - kMargin;
    uint32_t bits = 0;
    for (int i = 0; i < 8; ++i) {
        const int x = x0 + i;
        if (x >= w) break;
        int v = in[x];
        if (v < 0 || !row_in || x < kMargin || x >= w - kMargin) v = 0;
        out[x] = (int16_t)v;
        bits |= (uint32_t)(v > kRespMin) << i;
    }
    append_groups_wave(t, frame, bits, ((uint32_t)y << 16) | (uint32_t)x0);
}

void launch_hot_from_response(const int16_t* src, const LevelBatch& lb, const CompTables& t, int frame0, int nframes,
                              hipStream_t s) {
    if (nframes <= 0 || lb.w <= 0 || lb.h <= 0) return;
    const dim3 grid((t.gw + 63) / 64, (lb.h + 3) / 4, nframes);
    hipLaunchKernelGGL(hot_from_response_kernel, grid, dim3(256), 0, s, src, lb, t, frame0);
}

// Drains the LIFO exactly like follow_connected_component (:236-256) and returns how many hot
// pixels it consumed (zeroed).  Latency is what matters here (one lane, dependent global
// accesses, usually underneath a bandwidth-saturating pixel kernel), so per pop there is ONE
// round trip for the pixel and its four neighbours together (their addresses do not depend on
// the pixel's value) and the top of the stack lives in a register (the entry pushed last is the
// one popped next).
__device__ __forceinline__ int drain_lifo(int16_t* d, int w, int h, uint32_t* stk, int sp, Blob& b) {
    b.srx = b.sry = b.sr = 0;
    b.npix = 0;
    b.rmax = 0;
    b.xpk = b.ypk = 0;
    b.touched = false;
    int consumed = 0;
    uint32_t top = 0;
    bool has_top = false;
    auto push = [&](uint32_t e) {
        if (has_top) stk[sp++] = top;
        top = e;
        has_top = true;
    };
    while (true) {
        uint32_t e;
        if (has_top) { e = top; has_top = false; }
        else if (sp > 0) e = stk[--sp];
        else break;
        const int x = (int)(e & 0xffffu), y = (int)(e >> 16);
        const int q = y * w + x;
        // q is inside the fill region [7,w-7) x [7,h-7), so all four neighbours are inside the image
        const int v = d[q], vxp = d[q + 1], vxm = d[q - 1], vyp = d[q + w], vym = d[q - w];
        if (v <= 0) continue;                                  // visited already: d[q] = 0 is a no-op
        d[q] = 0;                                              // :245 / :250
        consumed += v > kRespMin;
        if (!(v > kRespMin && v > (b.rmax >> 4))) continue;    // :159-171 with :27
        if (v > b.rmax) { b.rmax = v; b.xpk = x; b.ypk = y; }  // :176-181, first maximum wins
        b.srx += (unsigned long long)(v * x);
        b.sry += (unsigned long long)(v * y);
        b.sr += (unsigned long long)v;
        b.npix++;
        // :252-255 then :216-226 (only hot pixels are worth pushing, see (1) above)
        if (x + 1 >= w - kMargin) b.touched = true;
        else if (vxp > kRespMin) push(e + 1u);
        if (x - 1 < kMargin) b.touched = true;
        else if (vxm > kRespMin) push(e - 1u);
        if (y + 1 >= h - kMargin) b.touched = true;
        else if (vyp > kRespMin) push(e + 0x10000u);
        if (y - 1 < kMargin) b.touched = true;
        else if (vym > kRespMin) push(e - 0x10000u);
    }
    return consumed;
}

// ---------------------------------------------------------------------------
// Detect: process_connected_components, points_scaled_out branch (:330-355)
// ---------------------------------------------------------------------------
// (the body: cc_detect_kernel runs it for one level, cc_detect_levels_kernel for several levels in one grid)
__device__ __forceinline__ void cc_detect_frame(const LevelBatch& lb, const CompTables& t, int level, const DetectOut& out,
                                                int frame) {
    __shared__ int s_nroots, s_ncand, s_arena_full;
    __shared__ unsigned long long s_arena_top;
    // latency-bound and tiny next to the pixel kernels it shares CUs with: take issue priority
    __builtin_amdgcn_s_setprio(3);
    if (t.lds_path && t.path[frame] == 1) return;  // done out of LDS
    if (t.hot_cnt[frame] > t.cap) {  // table overflow: report (with what the frame asked for), produce nothing
        if (threadIdx.x == 0) {
            report_hot_overflow(t.status + frame, t.hot_cnt[frame]);
            out.counts[frame] = -1;
        }
        return;
    }
    const FrameView v = make_view(lb, t, frame);
    if (threadIdx.x == 0) { s_nroots = 0; s_ncand = 0; s_arena_top = 0; s_arena_full = 0; }
    label_frame(v);

    // P3a: compact the roots.  A super-component of a single hot pixel can only ever give a
    // one-pixel blob, which the size test rejects (:205), and nothing else can reach it: skipped.
    for (int i = threadIdx.x; i < v.n; i += CCG_THREADS)
        if (v.parent[i] == i && v.comp_cnt[i] >= kBlobMinPixels) v.roots[atomicAdd(&s_nroots, 1)] = i;
    __syncthreads();
    const int nroots = s_nroots;

    // P3b: one lane per super-component replays the reference's sequence
    const int w = v.w, h = v.h;
    for (int k = threadIdx.x; k < nroots; k += CCG_THREADS) {
        const int r = v.roots[k];
        const int4 box = v.comp_box[r];
        const int cnt = v.comp_cnt[r];
        const unsigned long long off = atomicAdd(&s_arena_top, (unsigned long long)(4 * cnt + 1));
        if (off + (unsigned long long)(4 * cnt + 1) > (unsigned long long)v.arena_cap) { s_arena_full = 1; continue; }
        uint32_t* stk = v.arena + off;
        // seeds live in [8, w-8) x [8, h-8) (:332-333)
        const int ylo = max(box.y, kMargin + 1), yhi = min(box.w, h - kMargin - 2);
        const int xlo = max(box.x, kMargin + 1), xhi = min(box.z, w - kMargin - 2);
        int left = cnt;  // hot pixels of this super-component not consumed yet
        auto fill_from = [&](int x, int y) {
            stk[0] = (uint32_t)x | ((uint32_t)y << 16);  // :338
            Blob b;
            left -= drain_lifo(v.d, w, h, stk, 1, b);
            if (!blob_passes_cheap_tests(b)) return;
            if (!window_variance_high(v.img, v.img_stride, w, h, b.xpk, b.ypk)) return;  // :207
            const int c = atomicAdd(&s_ncand, 1);
            if (c < v.cand_cap) {
                Cand cd;
                cd.sum_rx = b.srx; cd.sum_ry = b.sry; cd.sum_r = b.sr;
                cd.seed = (y << 16) | x;  // orders like the raster index of the seed
                cd.x_peak = (uint16_t)b.xpk; cd.y_peak = (uint16_t)b.ypk;
                cd.ok = 1; cd.pad = 0;
                v.cand[c] = cd;
            }
        };
        // The raster scan meets this super-component first at its smallest raster index.  If that
        // pixel may seed, fill from it straight away; in the common case the fill consumes every
        // hot pixel of the super-component and no scan of the bounding box is needed at all.
        {
            const int e = v.comp_first[r];
            const int y = e >> 16, x = e & 0xffff;
            if (x >= xlo && x <= xhi && y >= ylo && y <= yhi) fill_from(x, y);
        }
        for (int y = ylo; y <= yhi && left > 0; ++y)
            for (int x = xlo; x <= xhi && left > 0; ++x) {
                if (!(v.d[y * w + x] > kRespMin)) continue;                  // is_valid(.., NULL), :335
                if (v.parent[hot_index_of(v.gidx, v.gw, x, y)] != r) continue;  // someone else's super-component
                fill_from(x, y);
            }
    }
    __syncthreads();
    if (s_ncand > v.cand_cap || s_arena_full) {
        if (threadIdx.x == 0) { wg_or(v.status, kStatusCandOverflow); out.counts[frame] = -1; }
        return;
    }
    const int nvalid = s_ncand;

    // P5: order by seed raster index = the reference's output order (:332-353)
    for (int c = threadIdx.x; c < nvalid; c += CCG_THREADS)
        v.sortkeys[c] = ((unsigned long long)(uint32_t)v.cand[c].seed << 32) | (uint32_t)c;
    int n_pad = 1;
    while (n_pad < nvalid) n_pad <<= 1;
    for (int i = nvalid + threadIdx.x; i < n_pad; i += CCG_THREADS) v.sortkeys[i] = ~0ull;
    __syncthreads();
    bitonic_sort(v.sortkeys, n_pad);
    emit_detect_outputs(v, v.sortkeys, nvalid, level, out, frame);
}
__global__ __launch_bounds__(CCG_THREADS, 4) void cc_detect_kernel(LevelBatch lb, CompTables t, int level,
                                                               DetectOut out, int frame0) {
    cc_detect_frame(lb, t, level, out, frame0 + blockIdx.x);
}
// Several levels of the same frames in ONE grid (blockIdx.y = the level's slot): the first pass of the full detector
// searches levels 3, 2 and 1 at once, and three launches of 64 workgroups one behind the other were three times the
// latency of one of 192 (a single frame through find_chessboard: 165 -> 65 us).
__global__ __launch_bounds__(CCG_THREADS, 4) void cc_detect_levels_kernel(DetectLevels a) {
    const int k = blockIdx.y;
    cc_detect_frame(a.lb[k], a.t[k], a.level[k], a.out[k], blockIdx.x);
}

void launch_cc_detect(const LevelBatch& lb, const CompTables& t, int level, const DetectOut& out, int frame0,
                      int nframes, hipStream_t s) {
    if (nframes <= 0) return;
    launch_cc_detect_lds(lb, t, level, out, frame0, nframes, s);
    hipLaunchKernelGGL(cc_detect_kernel, dim3(nframes), dim3(CCG_THREADS), 0, s, lb, t, level, out, frame0);
}

// ---------------------------------------------------------------------------
// Refine: process_connected_components, points_refinement branch (:356-397)
// ---------------------------------------------------------------------------
// (the body: cc_refine_kernel runs it for one level, cc_refine_flagged_levels_kernel level after level)
__device__ __forceinline__ void cc_refine_frame(const LevelBatch& lb, const CompTables& t, int level, const RefineIO& io,
                                                int frame) {
    __shared__ int s_changed, s_nref, s_arena_full;
    __shared__ unsigned long long s_arena_top;
    if (t.lds_path && t.path[frame] == 1) return;  // done out of LDS
    if (t.hot_cnt[frame] > t.cap) {
        if (threadIdx.x == 0) {
            report_hot_overflow(t.status + frame, t.hot_cnt[frame]);
            if (io.nrefined) io.nrefined[frame] = -1;
        }
        return;
    }
    const FrameView v = make_view(lb, t, frame);
    if (threadIdx.x == 0) { s_changed = 0; s_nref = 0; s_arena_top = 0; s_arena_full = 0; }
    label_frame(v);  // (presets v.roots[] to INT_MAX: it is the claim table here)

    const int w = v.w, h = v.h;
    const int npts = min(io.npoints[frame], io.pitch);
    const long long pb = (long long)frame * io.pitch;
    double* pts = io.points + 2 * pb;
    signed char* lv = io.levels + pb;
    int32_t* leader = io.leader + pb;
    int32_t* need = io.need + pb;
    int32_t* nseeds = io.nseeds + pb;
    uint32_t* seeds = io.seeds + 9 * pb;
    int32_t* sroot = io.sroot + 9 * pb;
    const uint16_t coord_scale = (uint16_t)(1u << level);

    // R1: seeds of every refinable point (:362-382), in the reference's push order, and the
    // super-component (root) each seed belongs to
    for (int i = threadIdx.x; i < npts; i += CCG_THREADS) {
        int ns = -1;  // -1: not refinable at this level
        if (lv[i] == level + 1) {
            ns = 0;
            const double lx = rescale_coord(pts[2 * i + 0], 1.0 / coord_scale);  // :369
            const double ly = rescale_coord(pts[2 * i + 1], 1.0 / coord_scale);
            const int x = (int)(lx + 0.5), y = (int)(ly + 0.5);  // :371-372
            for (int dx = -1; dx <= 1; ++dx)
                for (int dy = -1; dy <= 1; ++dy) {
                    const int sx = (int16_t)(x + dx), sy = (int16_t)(y + dy);  // is_valid takes int16_t
                    if (sx < 0 || sx >= w || sy < 0 || sy >= h) continue;
                    const int p = sy * w + sx;
                    if (!(v.d[p] > kRespMin)) continue;
                    seeds[9 * i + ns] = (uint32_t)sx | ((uint32_t)sy << 16);
                    sroot[9 * i + ns] = v.parent[hot_index_of(v.gidx, v.gw, sx, sy)];
                    ++ns;
                }
        }
        nseeds[i] = ns;
        leader[i] = i;
        need[i] = 0;
    }
    __syncthreads();

    // R2: points whose seeds share a super-component must be replayed in index
    // order by one lane; label-propagate the minimum point index over the
    // bipartite graph points <-> super-components until nothing changes.
    while (true) {
        for (int i = threadIdx.x; i < npts; i += CCG_THREADS) {
            const int ns = nseeds[i];
            if (ns <= 0) continue;
            int m = leader[i];
            for (int k = 0; k < ns; ++k) m = min(m, aload(v.roots + sroot[9 * i + k]));
            bool changed = m < leader[i];
            for (int k = 0; k < ns; ++k)
                if (wg_min(v.roots + sroot[9 * i + k], m) > m) changed = true;
            leader[i] = m;
            if (changed) s_changed = 1;
        }
        __syncthreads();
        const int changed = s_changed;
        __syncthreads();
        if (!changed) break;
        if (threadIdx.x == 0) s_changed = 0;
        __syncthreads();
    }

    // R3: stack demand of each group = 4 * (hot pixels of its super-components), counted once
    for (int i = threadIdx.x; i < npts; i += CCG_THREADS) {
        const int ns = nseeds[i];
        for (int k = 0; k < ns; ++k) {
            const int old = wg_or(v.comp_cnt + sroot[9 * i + k], (int)0x80000000);
            if (old >= 0) wg_add(need + leader[i], 4 * old);
        }
    }
    __syncthreads();

    // R4: one lane per group, members in index order (:358); accepted points are written in place
    for (int i = threadIdx.x; i < npts; i += CCG_THREADS) {
        if (nseeds[i] < 0 || leader[i] != i) continue;
        const unsigned long long off = atomicAdd(&s_arena_top, (unsigned long long)(need[i] + 10));
        if (off + (unsigned long long)(need[i] + 10) > (unsigned long long)v.arena_cap) { s_arena_full = 1; continue; }
        uint32_t* stk = v.arena + off;
        for (int j = i; j < npts; ++j) {
            if (nseeds[j] < 0 || leader[j] != i) continue;
            const int ns = nseeds[j];
            for (int k = 0; k < ns; ++k) stk[k] = seeds[9 * j + k];
            Blob b;
            drain_lifo(v.d, w, h, stk, ns, b);
            if (!blob_passes_cheap_tests(b)) continue;
            if (!window_variance_high(v.img, v.img_stride, w, h, b.xpk, b.ypk)) continue;  // :207
            const double cx = (double)b.srx / (double)b.sr;  // :262-263
            const double cy = (double)b.sry / (double)b.sr;
            pts[2 * j + 0] = rescale_coord(cx, (double)coord_scale);  // :390
            pts[2 * j + 1] = rescale_coord(cy, (double)coord_scale);
            lv[j] = (signed char)level;  // :393
            atomicAdd(&s_nref, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_arena_full) wg_or(v.status, kStatusCandOverflow);  // points refined so far stay refined; the call fails
        // path 2: the LDS kernel refined the points of the bands it finished before it gave up (their count
        // is in nrefined already); what is refined here is the rest
        const int before = (t.lds_path && t.path[frame] == 2 && io.nrefined) ? io.nrefined[frame] : 0;
        if (io.nrefined) io.nrefined[frame] = s_arena_full ? -1 : before + s_nref;
    }
}

__global__ __launch_bounds__(CCG_THREADS, 4) void cc_refine_kernel(LevelBatch lb, CompTables t, int level,
                                                               RefineIO io, int frame0) {
    __builtin_amdgcn_s_setprio(3);
    cc_refine_frame(lb, t, level, io, frame0 + blockIdx.x);
}

// The dense repeat of the frames a sparse chain reported, in one launch (kernels.h, launch_cc_refine_flagged_levels).
struct RefineLevels {
    LevelBatch lb[kRefineLevelsMax];  // indexed by level
    CompTables t[kRefineLevelsMax];
    int n;
    RefineIO io;
    SparseRestore restore;
    const int32_t* list;  // the frames (launch_sparse_flag_list)
    int32_t* status0;
    int level_stride;
    int32_t* counter;
};
constexpr int kFlaggedSlots = 8;  // workgroups of cc_refine_flagged_levels_kernel: workgroup b takes frames b, b + 8, ... of the list
__global__ __launch_bounds__(CCG_THREADS, 8) void cc_refine_flagged_levels_kernel(RefineLevels a) {  // (<= 64 VGPRs: see CCG_THREADS)
    __builtin_amdgcn_s_setprio(3);
    const int nlisted = a.list[0];
    for (int li = blockIdx.x; li < nlisted; li += kFlaggedSlots) {
        const int frame = a.list[1 + li];
        {   // the points as they were before the first sparse level
            const int n = min(a.io.npoints[frame], a.io.pitch);
            const long long pb = (long long)frame * a.io.pitch;
            for (int i = threadIdx.x; i < n; i += CCG_THREADS) {
                if (a.restore.xy) {  // emit_detect_outputs' hand-over, again
                    const int32_t* xy = a.restore.xy + ((long long)frame * a.restore.xy_pitch + i) * 2;
                    a.io.points[2 * (pb + i) + 0] = (double)xy[0] / kGridScale;
                    a.io.points[2 * (pb + i) + 1] = (double)xy[1] / kGridScale;
                    a.io.levels[pb + i] = (signed char)a.restore.level;
                } else {
                    a.io.points[2 * (pb + i) + 0] = a.restore.pts0[2 * (pb + i) + 0];
                    a.io.points[2 * (pb + i) + 1] = a.restore.pts0[2 * (pb + i) + 1];
                    a.io.levels[pb + i] = a.restore.lv0[pb + i];
                }
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int L = a.n - 1; L >= 0; --L) {
            cc_refine_frame(a.lb[L], a.t[L], L, a.io, frame);
            __syncthreads();  // the level below reads the points and level tags this one wrote
        }
        if (threadIdx.x == 0) {
            for (int L = 0; L < a.n; ++L) atomicAnd(a.status0 + (long long)L * a.level_stride + frame, ~(int)kStatusSparse);
            if (a.counter) atomicAdd(a.counter, 1);
        }
    }
}
void launch_cc_refine_flagged_levels(const LevelBatch* lbs, const CompTables* ts, int nlevels, const RefineIO& io,
                                     const SparseRestore& restore, const int32_t* list, int32_t* status_level0,
                                     int level_stride, int32_t* counter, hipStream_t s) {
    if (nlevels <= 0 || nlevels > kRefineLevelsMax) return;
    RefineLevels a;
    for (int L = 0; L < kRefineLevelsMax; ++L) {
        a.lb[L] = lbs[L < nlevels ? L : 0];
        a.t[L] = ts[L < nlevels ? L : 0];
        a.t[L].lds_path = 0;  // every listed frame is this kernel's
        a.t[L].only = nullptr;
    }
    a.n = nlevels;
    a.io = io;
    a.restore = restore;
    a.list = list;
    a.status0 = status_level0;
    a.level_stride = level_stride;
    a.counter = counter;
    hipLaunchKernelGGL(cc_refine_flagged_levels_kernel, dim3(kFlaggedSlots), dim3(CCG_THREADS), 0, s, a);
}
// The frames a sparse chain reported, as a list: list[0] = how many, list[1 ..] = which (any order).  One workgroup.
__global__ __launch_bounds__(256) void sparse_flag_list_kernel(const int32_t* status0, int nframes, int32_t* list) {
    __shared__ int n;
    if (threadIdx.x == 0) n = 0;
    __syncthreads();
    for (int f = threadIdx.x; f < nframes; f += 256)
        if (status0[f] & kStatusSparse) list[1 + atomicAdd(&n, 1)] = f;
    __syncthreads();
    if (threadIdx.x == 0) list[0] = n;
}
void launch_sparse_flag_list(const int32_t* status_level0, int nframes, int32_t* list, hipStream_t s) {
    hipLaunchKernelGGL(sparse_flag_list_kernel, dim3(1), dim3(256), 0, s, status_level0, nframes, list);
}

void launch_cc_refine(const LevelBatch& lb, const CompTables& t, int level, const RefineIO& io, int frame0,
                      int nframes, hipStream_t s) {
    if (nframes <= 0) return;
    launch_cc_refine_lds(lb, t, level, io, frame0, nframes, s);
    // (sparse refinement: nothing for the global-memory kernel to work on -- a frame the LDS kernel cannot take is reported)
    if (!(t.lds_path & kLdsPathSparse))
        hipLaunchKernelGGL(cc_refine_kernel, dim3(nframes), dim3(CCG_THREADS), 0, s, lb, t, level, io, frame0);
}

}  // namespace mrg
