// The component search out of LDS: the detect and refine kernels, the cell lister of the sparse schedule, launchers.
#include "cc_lds.h"
#include "cc_sparse.h"

namespace mrg {

// What a declining kernel leaves behind: the frame stays with the global-memory kernels (path 0).  A kernel
// that declines after its first band has already appended candidates (detect: scratch the fallback
// overwrites) or refined the points of the bands it finished (refine: their level is updated, so the
// fallback skips them, and their components are disjoint from what is left -- same result).
// Sparse refinement (lds_path bit 1024): there is no global-memory kernel to leave the frame to (the dense response
// only holds the cells around the points): the frame is reported instead (kStatusSparse -> the caller repeats the
// call without the option).
constexpr int kLdsSparse = kLdsPathSparse;
// (`next_hdr`: the header of the next level's cell list, or NULL -- nobody lists that level's cells now)
__device__ __forceinline__ void lds_decline(const CompTables& t, int frame, int32_t* next_hdr = nullptr) {
    if (threadIdx.x != 0) return;
    if (t.lds_path & kLdsSparse) {
        t.path[frame] = 1;
        atomicOr(t.status + frame, kStatusSparse);  // (device scope: a frame may have several workgroups)
        if (next_hdr) atomicOr(next_hdr + kHdrFlags, kFlagGivenUp);
    } else {
        t.path[frame] = 0;
    }
}
// refine after the first band: path 2 = "the global-memory kernel finishes the frame and ADDS to nrefined"
__device__ __forceinline__ void lds_decline_refine(const CompTables& t, int frame, int band, const RefineIO& io, int nref) {
    if (threadIdx.x != 0) return;
    if (t.lds_path & kLdsSparse) {
        t.path[frame] = 1;
        atomicOr(t.status + frame, kStatusSparse);
        if (io.next_cnt) atomicOr(io.next_cnt + kCellHdr * frame + kHdrFlags, kFlagGivenUp);
        return;
    }
    t.path[frame] = band > 0 ? 2 : 0;
    if (band > 0 && io.nrefined) io.nrefined[frame] = nref;
}

// (launch bounds: at most 128 VGPRs, so that a wave of these kernels fits into what ONE retiring wave of the pixel
// kernels frees on a SIMD -- at 129 VGPRs the refine kernel waited for two, 80 -> 270 us per launch)
template <int N>
__device__ __forceinline__ void cc_detect_lds_frame(const LevelBatch& lb, const CompTables& t, int level, const DetectOut& out,
                                                    int frame) {
    using LdsCC = LdsCCT<N>;
    constexpr int LROOTS = LdsCC::LROOTS, LEPT = LdsCC::LEPT;
    constexpr int LSTKD = LdsCC::LSTK - LdsCC::LN;  // LIFO words of the fills: the neighbour table takes the first LN
    extern __shared__ __attribute__((aligned(16))) char lds_cc_raw[];
    LdsCC& L = *reinterpret_cast<LdsCC*>(lds_cc_raw);
    if (!MRG_EXP(t.lds_path & 16)) __builtin_amdgcn_s_setprio(3);
    const int tid = threadIdx.x;
    const int nraw = t.hot_cnt[frame];
    FrameView v = make_view(lb, t, frame);
    const int w = v.w, h = v.h;
    int nbands = 0;  // cc_lds bit 256: no banding (test hook)
    if (nraw <= t.cap && !(nraw > LdsCC::LN && (t.lds_path & 256))) nbands = lds_plan_bands(L, v, nraw);
    if (nbands == 0) {
        lds_decline(t, frame);
        return;
    }
    if (tid == 0) L.ncand = 0;
    // seeds live in [8, w-8) x [8, h-8) (:332-333)
    auto seedable = [&](uint32_t e) {
        const int x = (int)(e & 0xffffu), y = (int)(e >> 16);
        return x > kMargin && x < w - kMargin - 1 && y > kMargin && y < h - kMargin - 1;
    };
    for (int band = 0; band < nbands; ++band) {
        int n;
        if (!lds_load_and_label(L, v, nraw, t.cap, nbands > 1, L.band_y[band], L.band_y[band + 1], n)) {
            lds_decline(t, frame);
            return;
        }
        if (MRG_EXP(t.lds_path & 8)) { if (tid == 0) { t.path[frame] = 1; out.counts[frame] = 0; } return; }  // ablation (timing only)
        // roots with >= 2 pixels (a single hot pixel can only give a one-pixel blob, :205); each gets a LIFO of
        // (sum of hot-neighbour counts + 1) words, which bounds the pushes of all fills of it together
        for (int i = tid; i < n; i += CC_THREADS) {
            if (L.xy[i] == kHotDead || L.lab[i] != i) continue;
            const int a = L.u.acc[i], cnt = a & 0x1fff, need = (a >> 13) + 1;
            if (cnt < kBlobMinPixels) continue;
            const int r = atomicAdd(&L.nroots, 1);
            if (need > LSTKD) L.total = 1;  // one super-component alone wants more LIFO than there is
            if (r < LROOTS) { L.w.r.root[r] = (int16_t)i; L.w.r.cnt[r] = (int16_t)cnt; L.w.r.soff[r] = (int16_t)min(need, LSTKD); }
        }
        __syncthreads();
        if (L.nroots > LROOTS || L.total) {  // does not fit
            lds_decline(t, frame);
            return;
        }
        const int nroots = L.nroots;
        // smallest raster position of every super-component: the first seed the raster scan meets
        for (int i = tid; i < n; i += CC_THREADS) L.u.acc[i] = 0x7fffffff;
        __syncthreads();
        for (int i = tid; i < n; i += CC_THREADS)
            if (L.xy[i] != kHotDead) atomicMin(&L.u.acc[L.lab[i]], (int)L.xy[i]);
        __syncthreads();
        // ... as a list index: the fills below have no hash map any more
        for (int r = tid; r < nroots; r += CC_THREADS)
            L.w.r.fidx[r] = (int16_t)lds_find(L, (uint32_t)L.u.acc[L.w.r.root[r]]);
        __syncthreads();
        // member lists (list indices of the pixels of a super-component, unordered): what the "raster scan goes
        // on" step below walks instead of the whole hot list.  They take over the storage of the labels.
        int mylab[LEPT];
#pragma unroll
        for (int k = 0; k < LEPT; ++k) {
            const int i = tid + CC_THREADS * k;
            mylab[k] = (i < n && L.xy[i] != kHotDead) ? (int)L.lab[i] : -1;
        }
        for (int i = tid; i < n; i += CC_THREADS) L.u.acc[i] = -1;
        __syncthreads();
        for (int r = tid; r < nroots; r += CC_THREADS) {
            const int mo = atomicAdd(&L.mtop, (int)L.w.r.cnt[r]);
            L.u.acc[L.w.r.root[r]] = mo;      // running write position of this list
            L.w.r.root[r] = (int16_t)mo;      // the root's list index is not needed any more
        }
        __syncthreads();
        int16_t* members = L.lab;
#pragma unroll
        for (int k = 0; k < LEPT; ++k) {
            if (mylab[k] < 0 || L.u.acc[mylab[k]] < 0) continue;  // (acc only grows: a list's slot stays >= 0)
            members[atomicAdd(&L.u.acc[mylab[k]], 1)] = (int16_t)(tid + CC_THREADS * k);
        }
        __syncthreads();  // the accumulators are dead: their storage becomes the LIFOs
        // neighbour table of the fills (drain_nb): low words over the hash map, high halves in the first LN words of
        // the LIFO space, the LIFOs behind them
        uint16_t* nhi = reinterpret_cast<uint16_t*>(L.u.stk);
        lds_build_neighbours(L, v, n, nhi);
        int16_t* lifo = L.u.stk + LdsCC::LN;

        // The fills of a band share LSTKD LIFO words.  When the super-components together want more (a 14x14 board:
        // ~150 of them per band at ~50 words each), they run in rounds: every pending root asks for its words, the
        // ones that still fit run, the others wait for the next round (the first to ask always fits).
        static_assert(LROOTS <= 2 * CC_THREADS, "a thread owns at most two roots");
        bool pending[2] = {tid < nroots, tid + CC_THREADS < nroots};
        while (true) {
        if (tid == 0) { L.top = 0; L.changed = 0; }
        __syncthreads();
        for (int rr = 0; rr < 2; ++rr) {
            if (!pending[rr]) continue;
            const int r = tid + CC_THREADS * rr;
            const int need = L.w.r.soff[r];
            const int so = atomicAdd(&L.top, need);
            if (so + need > LSTKD) { L.changed = 1; continue; }
            pending[rr] = false;
            const int cnt = L.w.r.cnt[r], mo = L.w.r.root[r];
            int left = cnt;
            int16_t* stk = lifo + so;
            int si = L.w.r.fidx[r];
            uint32_t seed = L.xy[si];
            bool have = seedable(seed);
            while (true) {
                if (!have) {
                    // the raster scan goes on: the smallest seedable position among what is left of this
                    // super-component (pixels below the running-maximum threshold are consumed but not
                    // expanded, so the fringe of a blob is often left over)
                    uint32_t best = kHotDead;
                    for (int q = 0; q < cnt; ++q) {
                        const int i = members[mo + q];
                        const uint32_t e = L.xy[i];
                        if (L.val[i] > 0 && seedable(e) && e < best) { best = e; si = i; }
                    }
                    if (best == kHotDead) break;
                    seed = best;
                }
                have = false;
                stk[0] = (int16_t)si;  // :338
                Blob b;
                if (MRG_EXP(t.lds_path & 4)) { b.touched = true; left = 0; }  // ablation (timing only)
                else left -= drain_nb(L, L.hashw, nhi, w, h, stk, 1, b);
                if (blob_passes_cheap_tests(b) &&
                    (MRG_EXP(t.lds_path & 2) || window_variance_high(v.img, v.img_stride, w, h, b.xpk, b.ypk))) {  // :207
                    const int c = atomicAdd(&L.ncand, 1);
                    if (c < v.cand_cap) {
                        Cand cd;
                        cd.sum_rx = b.srx; cd.sum_ry = b.sry; cd.sum_r = b.sr;
                        cd.seed = (int32_t)seed;
                        cd.x_peak = (uint16_t)b.xpk; cd.y_peak = (uint16_t)b.ypk;
                        cd.ok = 1; cd.pad = 0;
                        v.cand[c] = cd;
                    }
                }
                if (left <= 0) break;
            }
        }
        __syncthreads();
        if (!L.changed) break;
        __syncthreads();  // everybody has read the flag before it is reset
        }
    }
    // order by seed position = the reference's output order (:332-353), sorted in LDS.  The tables are dead:
    // the keys take the whole allocation (one band: at most LN / 2 candidates; several: whatever they gave)
    const int nvalid = L.ncand;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(lds_cc_raw);
    constexpr int kMaxKeys = 4096;
    static_assert(kMaxKeys * 8 <= (int)offsetof(LdsCC, nroots), "the sort keys must not reach the counters");
    if (nvalid > kMaxKeys || nvalid > v.cand_cap) {
        lds_decline(t, frame);
        return;
    }
    __syncthreads();  // every thread has read L.ncand before the keys overwrite the tables
    if (tid == 0) t.path[frame] = 1;
    int n_pad = 1;
    while (n_pad < nvalid) n_pad <<= 1;
    for (int c = tid; c < n_pad; c += CC_THREADS)
        keys[c] = c < nvalid ? (((unsigned long long)(uint32_t)v.cand[c].seed << 32) | (uint32_t)c) : ~0ull;
    __syncthreads();
    bitonic_sort(keys, n_pad);
    emit_detect_outputs(v, keys, nvalid, level, out, frame);
}
template <int N>
__global__ __launch_bounds__(CC_THREADS, 4) void cc_detect_lds_kernel(LevelBatch lb, CompTables t, int level,
                                                                   DetectOut out, int frame0) {
    cc_detect_lds_frame<N>(lb, t, level, out, frame0 + blockIdx.x);
}
template <int N>  // several levels in one grid: see cc_detect_levels_kernel
__global__ __launch_bounds__(CC_THREADS, 4) void cc_detect_lds_levels_kernel(DetectLevels a) {
    const int k = blockIdx.y;
    cc_detect_lds_frame<N>(a.lb[k], a.t[k], a.level[k], a.out[k], blockIdx.x);
}

// SPARSE: the instantiation behind a level of a sparse chain (kLdsPathSparse).  Two kernels, so that what the sparse
// schedule adds (mask expansion, the next level's cell list) costs the dense one neither registers nor spills.
template <int N, bool SPARSE>
__global__ __launch_bounds__(CC_THREADS, 4) void cc_refine_lds_kernel(LevelBatch lb, CompTables t, int level,
                                                                   RefineIO io, int frame0) {
    using LdsCC = LdsCCT<N>;
    constexpr int LN = LdsCC::LN, LSTK = LdsCC::LSTK;
    extern __shared__ __attribute__((aligned(16))) char lds_cc_raw[];
    LdsCC& L = *reinterpret_cast<LdsCC*>(lds_cc_raw);
    if (!MRG_EXP(t.lds_path & 16)) __builtin_amdgcn_s_setprio(3);
    const int frame = frame0 + blockIdx.x, tid = threadIdx.x;
    // phase clock (cc_lds bit 512, mrgingham_amd_debug_refine_clock, tools/cc_phases.py): thread 0 of the first
    // frame leaves 100 MHz ticks of the phase boundaries of its first band in the scratch of the global-memory kernel
    const bool clk = MRG_EXP(t.lds_path & 512) && blockIdx.x == 0 && tid == 0;
    long long* tk = reinterpret_cast<long long*>(io.sroot);  // (scratch of the global-memory kernel, unused here)
    auto tick = [&](int k) { if (clk) tk[k] = wall_clock64(); };
    tick(0);
    constexpr bool sparse = SPARSE;  // the response exists in the cells around the points only
    const int npts = min(io.npoints[frame], io.pitch);
    FrameView v = make_view(lb, t, frame);
    // several workgroups per frame ("Several workgroups" above): this one is subset `sub` of `nsub`
    int nsub = 1;
    const int sub = sparse ? (int)blockIdx.y : 0;
    if (sparse) {
        const int32_t* hdr = io.cell_cnt + kCellHdr * frame;
        nsub = hdr[kHdrSub];
        if (nsub < 1 || (hdr[kHdrFlags] & kFlagSingle)) nsub = 1;
        if (sub >= nsub) return;  // (nothing of the frame is this workgroup's: no header, no status is touched)
    }
    const bool split = nsub > 1;
    const int32_t* psub = io.leader + (long long)frame * io.pitch;  // (scratch of the global-memory kernel: here the points' subsets)
    int32_t* const next_hdr = (sparse && io.next_cnt) ? io.next_cnt + kCellHdr * frame : nullptr;
    // its own part of the frame's LIFO arena (lds_load_and_label parks there) and of its global hot list (a subset with more
    // hot pixels than the LDS list holds goes band by band over it, like a whole frame does)
    const int cap = split ? t.cap / kSubsets : t.cap;
    if (split) {
        v.arena += (long long)sub * (2 * LN);
        v.hot_xy += (long long)sub * cap;
    }
    // The cell bitmap lives in L.w (dead until the LIFO demands are written), the open flags behind the
    // accumulators in L.u (dead until the fills).
    WinSel ws;
    ws.cs = -1;
    uint32_t* const wbits = reinterpret_cast<uint32_t*>(&L.w);
    uint32_t* const obits = reinterpret_cast<uint32_t*>(L.u.stk) + LN;
    static_assert(sizeof(L.u) >= (size_t)LN * 4 + (size_t)LN / 8, "open flags behind the accumulators");
    static_assert(sizeof(L.w) / 4 == kWinWords, "list_cells sizes the bitmap for kWinWords");
    const int nraw = sparse ? hot_list_from_masks(io, t, frame, v.hot_xy, cap, &L.nload, L.xy, LN, ws, wbits, obits, LN / 32, split ? sub : -1)
                            : t.hot_cnt[frame];
    const bool preloaded = sparse && nraw <= LN;
    if (npts > LPTS || nraw < 0) {  // the LDS kernel does not take that many points (sparse: nor that many cells)
        lds_decline(t, frame, next_hdr);
        return;
    }
    const int w = v.w, h = v.h;
    const long long pb = (long long)frame * io.pitch;
    double* pts = io.points + 2 * pb;
    signed char* lv = io.levels + pb;
    int nbands = 0;  // cc_lds bit 256: no banding, no windows (test hook)
    const bool may_select = nraw <= cap && !(nraw > LN && (t.lds_path & 256));
    // More hot pixels than the tables hold: first try to load only the cells around the points (one pass over the
    // list; a textured scene has 10^4 - 10^5 hot pixels of which the refinement needs ~10^3), then bands.
    // (sparse refinement: the selection is what was computed, marked above, and every listed pixel is in it)
    bool windowed = sparse && nraw <= LN;
    // a list only a little longer than the tables is a large board on a flat background (14x14: 2600): every hot
    // pixel is near a point, the cells would hold them all -- bands first there, cells only if no band cut exists
    const bool bands_first = !sparse && nraw <= LN + LN / 2;
    auto try_windows = [&]() {
        ws = win_geometry(w, h, pts, lv, npts, level, kWinWords, false, L.edge);
        if (ws.cs < 0) return;
        win_mark<LN>(ws, w, h, pts, lv, npts, level, wbits, obits, false);
        // do the marked cells hold few enough hot pixels?  (one more pass over the list)
        if (tid == 0) L.nload = 0;
        __syncthreads();
        int cnt = 0;
        scan_hot_list(v.hot_xy, nraw, [&](uint32_t e) { cnt += ws.template marked<false>((int)(e & 0xffffu), (int)(e >> 16)); });
        if (cnt) atomicAdd(&L.nload, cnt);
        __syncthreads();
        windowed = L.nload <= LN;
        __syncthreads();
    };
    if (may_select && !sparse && nraw > LN && !bands_first) try_windows();
    if (!windowed && may_select && !sparse) nbands = lds_plan_bands(L, v, nraw);
    if (!windowed && nbands == 0 && may_select && nraw > LN && bands_first) try_windows();
    // sparse refinement, the cells hold more hot pixels than the tables (a 14x14 board at level 1: 3000): bands of the
    // list -- everything in it is in a marked cell --, the cells marked again before every band (the bitmap shares its
    // LDS with the LIFO demands of the band before).  A band boundary may cross hot pixels that are not in the list;
    // those are in unmarked cells, which is exactly what the open check looks for.
    bool win_bands = false;
    if (sparse && !windowed && may_select && ws.cs >= 0) {
        nbands = lds_plan_bands(L, v, nraw);
        win_bands = windowed = nbands > 0;
    } else if (windowed) {
        if (tid == 0) { L.band_y[0] = 0; L.band_y[1] = 0; L.shear = 0; }
        nbands = 1;
        __syncthreads();
    }
    if (nbands == 0) {
        lds_decline(t, frame, next_hdr);
        return;
    }
    if (tid == 0) L.nref = 0;
    tick(1);
    uint32_t* seeds = io.seeds + 9 * pb;  // here: list indices, read back by the group's leader lane
    int32_t* nseeds = io.nseeds + pb;
    int32_t* gneed = io.need + pb;  // per leader
    const uint16_t coord_scale = (uint16_t)(1u << level);
    // the group leader of every point, -1 for a point that is not refinable at this level: behind
    // need16[] in the same union (LN * 2 bytes used of 2.5 LN), npts <= LPTS entries
    int16_t* lead16 = L.w.need16 + LN;
    static_assert(sizeof(L.w) >= (size_t)LN * 2 + (size_t)LPTS * 2, "lead16 must fit behind need16");

    for (int band = 0; band < nbands; ++band) {
        int n;
        if (win_bands) {
            __syncthreads();
            mark_listed_cells(ws, io.cell_list + (long long)frame * io.list_pitch, io.cell_cnt[kCellHdr * frame], wbits, obits, LN / 32,
                              split ? sub : -1);
        }
        if (!lds_load_and_label<SPARSE>(L, v, nraw, cap, nbands > 1, L.band_y[band], L.band_y[band + 1], n,
                                        windowed ? &ws : nullptr, preloaded)) {
            // (window mode: the cells around the points hold more hot pixels than the tables do -- band 0, plain decline)
            lds_decline_refine(t, frame, band, io, L.nref);
            return;
        }
        if (MRG_EXP(t.lds_path & 8)) { if (tid == 0) t.path[frame] = 1; return; }  // ablation (timing only)
        if (band == 0) tick(2);
        // LIFO demand of every super-component at its root, then the accumulators become the claim table
        for (int i = tid; i < n; i += CC_THREADS) L.w.need16[i] = (int16_t)((L.u.acc[i] >> 13) + 1);
        __syncthreads();
        int32_t* claim = L.u.acc;
        for (int i = tid; i < n; i += CC_THREADS) claim[i] = 0x7fffffff;

        // R1: seeds of every refinable point (:362-382), in the reference's push order.  A thread owns points
        // tid and tid + 256 and keeps their seed roots, seed counts and leaders in registers.  (With bands: a
        // point finds its seeds in exactly one band -- the hash only holds this band's pixels -- and is not
        // refinable any more once a band has refined it.)
        int ns_[LPPT], lead_[LPPT];
        short sroot_[LPPT][9];
#pragma unroll
        for (int q = 0; q < LPPT; ++q) {
            const int i = tid + CC_THREADS * q;
            int ns = -1;  // -1: not refinable at this level (or no such point)
            if (i < npts && lv[i] == level + 1 && (!split || psub[i] == sub)) {
                ns = 0;
                const double lx = rescale_coord(pts[2 * i + 0], 1.0 / coord_scale);  // :369
                const double ly = rescale_coord(pts[2 * i + 1], 1.0 / coord_scale);
                const int x = (int)(lx + 0.5), y = (int)(ly + 0.5);  // :371-372
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy) {
                        const int sx = (int16_t)(x + dx), sy = (int16_t)(y + dy);  // is_valid takes int16_t
                        int j = -1;
                        if (sx >= 0 && sx < w && sy >= 0 && sy < h)
                            j = lds_find(L, ((uint32_t)sy << 16) | (uint32_t)sx);  // hot <=> listed (nothing consumed yet)
                        if (j >= 0) {
                            seeds[9 * i + ns] = (uint32_t)j;
                            const int r = L.lab[j];
#pragma unroll
                            for (int k = 0; k < 9; ++k)  // static register index
                                if (k == ns) sroot_[q][k] = (short)r;
                            ++ns;
                            // window mode: a seed in a super-component that reaches the edge of what was loaded
                            if (windowed && ((ws.openbits[r >> 5] >> (r & 31)) & 1u)) L.leak = 1;
                        }
                    }
                nseeds[i] = ns;
            }
            ns_[q] = ns;
            lead_[q] = i;
        }
        __syncthreads();
        if (windowed && L.leak) {  // (uniform) nothing has been refined yet: the global-memory kernel takes the frame
            lds_decline(t, frame, next_hdr);
            return;
        }
        if (band == 0) tick(3);

        // R2: points whose seeds share a super-component are replayed in index order by one lane:
        // propagate the minimum point index over the bipartite graph points <-> super-components
        while (true) {
            bool changed = false;
#pragma unroll
            for (int q = 0; q < LPPT; ++q) {
                if (ns_[q] <= 0) continue;
                int m = lead_[q];
#pragma unroll
                for (int k = 0; k < 9; ++k)
                    if (k < ns_[q])
                        m = min(m, __hip_atomic_load(&claim[sroot_[q][k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                changed |= m < lead_[q];
#pragma unroll
                for (int k = 0; k < 9; ++k)
                    if (k < ns_[q] && atomicMin(&claim[sroot_[q][k]], m) > m) changed = true;
                lead_[q] = m;
            }
            if (changed) L.changed = 1;
            __syncthreads();
            const int c = L.changed;
            __syncthreads();
            if (!c) break;
            if (tid == 0) L.changed = 0;
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < LPPT; ++q) {
            const int i = tid + CC_THREADS * q;
            if (i < npts) lead16[i] = (int16_t)(ns_[q] < 0 ? -1 : lead_[q]);
        }

        if (band == 0) tick(4);
        // R3: LIFO demand of each group = sum over its super-components, each counted once; groups take
        // their LIFOs in the order of a running counter
#pragma unroll
        for (int q = 0; q < LPPT; ++q) {
            const int i = tid + CC_THREADS * q;
            if (i < npts && (!split || psub[i] == sub)) gneed[i] = 0;  // (a group's leader is one of the subset's own points)
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < LPPT; ++q) {
            if (ns_[q] <= 0) continue;  // nothing hot around the point (in this band): :383-384, no fill
            const int i = tid + CC_THREADS * q, ld = lead_[q];
            int add = ld == i ? 10 : 0;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                if (k >= ns_[q]) continue;
                const int root = sroot_[q][k];
                if (atomicCAS(&claim[root], ld, ld | 0x40000000) == ld) add += (int)L.w.need16[root];
            }
            // bits 20..: members of the group (so that its lane knows when it has seen the last one)
            wg_add(gneed + ld, add + (1 << 20));
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < LPPT; ++q) {
            const int i = tid + CC_THREADS * q;
            if (ns_[q] > 0 && lead_[q] == i) atomicMax(&L.total, aload(gneed + i) & 0xfffff);
        }
        __syncthreads();
        if (L.total > LSTK) {  // one group alone wants more LIFO than there is
            lds_decline_refine(t, frame, band, io, L.nref);
            return;
        }
        __syncthreads();  // the claim table is dead: its storage becomes the LIFOs
        // (here rather than behind R1, where labels and hash map die: the seed roots of R1-R3 are out of the
        // registers by now)
        uint16_t* nhi = reinterpret_cast<uint16_t*>(L.lab);  // (the labels are dead as well)
        lds_build_neighbours(L, v, n, nhi);

        if (band == 0) tick(5);
        // R4: one lane per group, members in index order (:358); accepted points are written in place.  The
        // groups share LSTK LIFO words and run in rounds when together they want more (see the detect kernel).
        bool pending[LPPT];
#pragma unroll
        for (int q = 0; q < LPPT; ++q) pending[q] = ns_[q] > 0 && lead_[q] == tid + CC_THREADS * q;
        while (true) {
        if (tid == 0) { L.top = 0; L.changed = 0; }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < LPPT; ++q) {
            const int i = tid + CC_THREADS * q;
            if (!pending[q]) continue;
            const int gn = aload(gneed + i), need = gn & 0xfffff;
            const int so = atomicAdd(&L.top, need);
            if (so + need > LSTK) { L.changed = 1; continue; }
            pending[q] = false;
            int16_t* stk = L.u.stk + so;
            int left = gn >> 20;  // members not met yet: most groups are one point, and the walk ends at once
            for (int j = i; left > 0; ++j) {
                if (lead16[j] != i) continue;
                --left;
                const int ns = j == i ? ns_[q] : aload(nseeds + j);
                for (int k = 0; k < ns; ++k) stk[k] = (int16_t)__hip_atomic_load(&seeds[9 * j + k], MRG_WG);
                Blob b;
                if (MRG_EXP(t.lds_path & 4)) continue;  // ablation (timing only)
                drain_nb(L, L.hashw, nhi, w, h, stk, ns, b);
                if (!blob_passes_cheap_tests(b)) continue;
                if (!MRG_EXP(t.lds_path & 2) && !window_variance_high(v.img, v.img_stride, w, h, b.xpk, b.ypk)) continue;  // :207
                const double cx = (double)b.srx / (double)b.sr;  // :262-263
                const double cy = (double)b.sry / (double)b.sr;
                pts[2 * j + 0] = rescale_coord(cx, (double)coord_scale);  // :390
                pts[2 * j + 1] = rescale_coord(cy, (double)coord_scale);
                lv[j] = (signed char)level;  // :393
                atomicAdd(&L.nref, 1);
            }
        }
        __syncthreads();
        if (!L.changed) break;
        __syncthreads();  // everybody has read the flag before it is reset
        }
        if (band == 0) tick(6);
        __threadfence_block();
        __syncthreads();  // the next band reads the levels this one wrote
        // Several bands: what this band's fills consumed goes back into the dense response, like the
        // global-memory kernel leaves it.  If a later band has to give the frame up, that kernel finishes
        // it, and a point of THIS band that was rejected because an earlier point had consumed its
        // component must find it consumed again.
        if (nbands > 1) {
            for (int i = tid; i < n; i += CC_THREADS)
                if (L.val[i] == 0) v.d[(int)(L.xy[i] >> 16) * w + (int)(L.xy[i] & 0xffffu)] = 0;
            __syncthreads();
        }
    }
    if (tid == 0) {
        t.path[frame] = 1;
        if (io.nrefined) {
            if (split) atomicAdd(io.nrefined + frame, L.nref);  // (zeroed by the launcher)
            else io.nrefined[frame] = L.nref;
        }
    }
    if (sparse && io.next_cnt) {
        // the cells of the next level down, around the points as they are now (the barrier at the end of the last band
        // has made them visible): saves a launch -- and its dependent round trips under a saturated HBM -- per level.
        // They go into the OTHER list buffer: a workgroup of a split level may get here while the others still read
        // this level's.  The tables are dead: the cut of the next level's points and the split list build in them.
        uint32_t* const nlist = io.next_list + (long long)frame * io.list_pitch;
        if (!split) {
            static_assert(sizeof(L.u) >= sizeof(PartScratch), "partition_points works in the LIFO storage");
            const int nnext = partition_points(pts, lv, npts, level - 1, io.leader + (long long)frame * io.pitch,
                                               *reinterpret_cast<PartScratch*>(&L.u), io.subsets);
            list_cells(io.next_w, io.next_h, pts, lv, npts, level - 1, reinterpret_cast<uint32_t*>(&L.w), L.edge, &L.nload,
                       nlist, io.list_pitch, io.next_max_items, next_hdr, psub, nnext);
        } else {
            list_cells_split(io.next_w, io.next_h, pts, lv, npts, level - 1, reinterpret_cast<uint32_t*>(&L.w), &L.nload, L.xy, LN,
                             io.cell_cnt + kCellHdr * frame, nlist, io.list_pitch, io.next_max_items, next_hdr, psub, sub, nsub);
        }
    }
    if (clk) {
        tick(7);
        tk[8] = nraw; tk[9] = npts; tk[10] = nbands; tk[11] = level;
    }
}

// One workgroup per frame: the cells of the first level below the start level (its points come from the detection;
// below that the refinement kernel of a level lists the cells of the next one itself), the cut of its points into
// subsets, and the headers of the levels below it zeroed (cnt_all: [level][frame][kCellHdr]).
__global__ __launch_bounds__(CC_THREADS) void sparse_cells_kernel(int w, int h, int level, RefineIO io, uint32_t* cell_list,
                                                               int32_t* cell_cnt, int list_pitch, long long max_items,
                                                               int frame0, int32_t* cnt_all, int nframes_all) {
    __shared__ uint32_t bits[kWinWords];
    __shared__ uint32_t box[4];
    __shared__ int n;
    __shared__ PartScratch part;
    const int frame = frame0 + blockIdx.x;
    const long long pb = (long long)frame * io.pitch;
    if (cnt_all && threadIdx.x < level) {
        int32_t* hd = cnt_all + ((size_t)threadIdx.x * nframes_all + frame) * kCellHdr;
        hd[0] = 0; hd[kHdrSub] = 0; hd[kHdrFlags] = 0;
    }
    const int npts = min(io.npoints[frame], io.pitch);
    const int nsub = partition_points(io.points + 2 * pb, io.levels + pb, npts, level, io.leader + pb, part, io.subsets);
    list_cells(w, h, io.points + 2 * pb, io.levels + pb, npts, level, bits, box, &n,
               cell_list + (long long)frame * list_pitch, list_pitch, max_items, cell_cnt + kCellHdr * frame, io.leader + pb, nsub);
}

template <int N, class K, class... A>
static void launch_lds_grid(K kernel, dim3 grid, hipStream_t s, A... args) {
    // MRGINGHAM_AMD_CC_LDS_PAD: extra bytes of dynamic LDS per workgroup of every LDS kernel, the several-levels detect
    // kernel included (experiment: where does the allocation stop fitting into one slot of the pixel kernels?)
#ifdef MRG_EXPERIMENT
    static const int pad = [] { const char* e = getenv("MRGINGHAM_AMD_CC_LDS_PAD"); return e ? atoi(e) : 0; }();
#else
    constexpr int pad = 0;
#endif
    static bool once = ((void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(LdsCCT<N>) + pad), true);
    (void)once;
    hipLaunchKernelGGL(kernel, grid, dim3(CC_THREADS), sizeof(LdsCCT<N>) + pad, s, args...);
}
template <int N, class K, class... A>
static void launch_lds(K kernel, int nframes, hipStream_t s, A... args) { launch_lds_grid<N>(kernel, dim3(nframes), s, args...); }

void launch_cc_detect_lds(const LevelBatch& lb, const CompTables& t, int level, const DetectOut& out, int frame0,
                          int nframes, hipStream_t s) {
    if (!t.lds_path || nframes <= 0) return;
    launch_lds<2048>(cc_detect_lds_kernel<2048>, nframes, s, lb, t, level, out, frame0);
}

void launch_cc_detect_levels(const LevelBatch* lbs, const CompTables* ts, const int* levels, const DetectOut* outs, int nlevels,
                             int nframes, hipStream_t s) {
    if (nframes <= 0 || nlevels <= 0) return;
    if (nlevels == 1 || nlevels > kDetectLevelsMax) {
        for (int k = 0; k < nlevels; ++k) launch_cc_detect(lbs[k], ts[k], levels[k], outs[k], 0, nframes, s);
        return;
    }
    DetectLevels a;
    bool lds = true;
    for (int k = 0; k < kDetectLevelsMax; ++k) {
        const int q = k < nlevels ? k : 0;
        a.lb[k] = lbs[q];
        a.t[k] = ts[q];
        a.level[k] = levels[q];
        a.out[k] = outs[q];
        lds = lds && ts[q].lds_path;
    }
    if (lds) launch_lds_grid<2048>(cc_detect_lds_levels_kernel<2048>, dim3(nframes, nlevels), s, a);
    hipLaunchKernelGGL(cc_detect_levels_kernel, dim3(nframes, nlevels), dim3(CCG_THREADS), 0, s, a);
}

void launch_sparse_cells(const LevelBatch& lb, const CompTables& t, int level, const RefineIO& io, uint32_t* cell_list,
                         int32_t* cell_cnt, int list_pitch, int frame0, int nframes, hipStream_t s, int32_t* cnt_all, int nframes_all) {
    if (nframes <= 0) return;
    // the masks of chess_cells_kernel (32 B per micro-tile) go where the pixel -> index map of a dense level is
    hipLaunchKernelGGL(sparse_cells_kernel, dim3(nframes), dim3(CC_THREADS), 0, s, lb.w, lb.h, level, io, cell_list, cell_cnt,
                       list_pitch, t.gidx_pitch / 4, frame0, cnt_all, nframes_all);
}

void launch_cc_refine_lds(const LevelBatch& lb, const CompTables& t, int level, const RefineIO& io, int frame0,
                          int nframes, hipStream_t s) {
    if (!t.lds_path || nframes <= 0) return;
    if (t.lds_path & kLdsPathSparse) {
        // up to kSubsets workgroups per frame (those that find no subset of theirs leave at once); they ADD to nrefined
        if (io.nrefined) (void)hipMemsetAsync(io.nrefined + frame0, 0, (size_t)nframes * 4, s);
        const int ky = io.subsets < 1 ? 1 : (io.subsets > kSubsets ? kSubsets : io.subsets);
        launch_lds_grid<2048>(cc_refine_lds_kernel<2048, true>, dim3(nframes, ky), s, lb, t, level, io, frame0);
    } else {
        launch_lds<2048>(cc_refine_lds_kernel<2048, false>, nframes, s, lb, t, level, io, frame0);
    }
}

}  // namespace mrg
