// Host side of libmrgingham_amd.so, the detector's stream scheduling: what a detect / refine / chain call puts on the
// pixel stream and on its component stream, the events between the two (kernel timing included), the sparse schedule,
// and the entry points mrgingham_amd_detect_batch, _refine_batch, _chain_batch and _cc_on_response_batch.
// api.hip holds the context these work on (ctx.h).  See include/mrgingham_amd.h for the contract of every entry point.
#include "ctx.h"

namespace mrg {

// KERNEL TIMING (mrgingham_amd_chess_kernel_ms): a pair of events around "the dominant launch" of a call.  Every
// hipEventRecord on the pixel stream is a packet of its own between two kernels (~4 us each in the kernel trace), so
// a boundary gets ONE: where a level's component search waits for the launch that is timed, the closing mark is that
// level's hand-over event as well, and a mark that stands between two launches closes nothing and opens the next pair.
hipEvent_t timing_event(mrgingham_amd_ctx* ctx) {
    TimingEvents& te = ctx->timing_events;
    if (te.idle.empty()) {
        Event fresh;
        if (fresh.create(hipEventDefault) != hipSuccess) return nullptr;
        te.idle.push_back(fresh);
        te.all.push_back(std::move(fresh));
    }
    const hipEvent_t e = te.idle.back();
    te.idle.pop_back();
    return e;
}
// the opening mark of a pair on `s` when `on` (else NULL): `recorded` if the caller has one on the stream already
static hipEvent_t timing_open(mrgingham_amd_ctx* ctx, hipStream_t s, bool on, hipEvent_t recorded = nullptr) {
    if (!on) return nullptr;
    if (recorded) return recorded;
    hipEvent_t e0 = timing_event(ctx);
    hipEventRecord(e0, s);
    return e0;
}
// Behind the launch: closes the pair `e0` opened (it is read and recycled by mrgingham_amd_chess_kernel_ms); without one
// (timing off) records `handover` if the caller needs an event there at all.  Returns the event that was recorded:
// whoever waits for the launch waits for that.
static hipEvent_t timing_close(mrgingham_amd_ctx* ctx, hipStream_t s, hipEvent_t e0, hipEvent_t handover) {
    hipEvent_t e1 = e0 ? timing_event(ctx) : handover;
    if (e1) hipEventRecord(e1, s);
    if (e0) ctx->timing_events.pairs.emplace_back(e0, e1);
    return e1;
}

void launch_chess_any(mrgingham_amd_ctx* ctx, const LevelBatch& lb, const CompTables& t, int n, bool clamp, bool hot,
                      hipStream_t s, bool time_it) {
    hipEvent_t e0 = timing_open(ctx, s, time_it && ctx->timing);
    if (lb.w > 0 && lb.h > 0 && n > 0) {
#ifdef MRG_EXPERIMENT
        if (ctx->use_v0) launch_chess_v0(lb, t, 0, n, clamp, hot, s);
        else
#endif
        if (!hot && ((ctx->chess_variant == 0 && chess16_pays(lb, n)) || (ctx->chess_variant == 16 && chess16_ok(lb)))) launch_chess16(lb, 0, n, clamp, s, ctx->chess16_seg);
#ifdef MRG_EXPERIMENT
        else if (hot && (ctx->chess_variant_hot & 16) && !t.only && chess16_ok(lb)) launch_chess16_hot(lb, t, 0, n, s);
#endif
        else launch_chess(lb, t, 0, n, clamp, hot, s, ctx->chess_seg);
    }
    timing_close(ctx, s, e0, nullptr);
}

// Every detect / refine / chain call starts here: the pixel stream must not
// overwrite level scratch the component stream of the previous call still reads.
void begin_op(mrgingham_amd_ctx* ctx, int max_level) {
    (void)max_level;
    ctx->cur = (ctx->cur + 1) % ctx->nsets;  // this set was last used nsets calls ago
    ctx->status_copied[ctx->cur] = false;    // (until this op's end_op has queued its copy)
    ctx->pixel_stage.valid = false;          // (mrgingham_amd_debug_pixel_products: the scratch is about to change)
    if (ctx->cc_pending[ctx->cur]) hipStreamWaitEvent(ctx->pix, ctx->ev_cc_done[ctx->cur], 0);
    // The hot-pixel counters of this set are zero here: they are zeroed at allocation and again by
    // end_op behind the component kernels that consumed them -- on the component stream, off the
    // pixel stream's critical path.  (Status words only ever accumulate; mrgingham_amd_sync reads
    // and clears them.)
}
// Registers the caller-owned device buffers this call writes (w) and reads (r) and makes its
// component stream wait for every earlier call still pending on ANOTHER scratch set (each set has a
// component stream of its own; the set's own earlier call is ordered by the stream) whose written
// spans overlap what this call reads or writes, or whose read spans overlap what it writes.  Call after begin_op.
void order_after_previous(mrgingham_amd_ctx* ctx, std::initializer_list<mrgingham_amd_ctx::Span> w,
                          std::initializer_list<mrgingham_amd_ctx::Span> r) {
    const int cur = ctx->cur;
    auto overlaps = [](const mrgingham_amd_ctx::Span& a, const mrgingham_amd_ctx::Span& b) {
        return a.p && b.p && a.n && b.n && a.p < b.p + b.n && b.p < a.p + a.n;
    };
    for (int prev = 0; prev < kMaxSets; ++prev) {  // every call that may still be running on another component stream
        if (prev == cur || !ctx->cc_pending[prev]) continue;
        bool dep = false;
        for (const auto& pw : ctx->last_w[prev]) {
            for (const auto& x : w) dep |= overlaps(x, pw);
            for (const auto& x : r) dep |= overlaps(x, pw);
        }
        for (const auto& pr : ctx->last_r[prev])
            for (const auto& x : w) dep |= overlaps(x, pr);
        if (dep) hipStreamWaitEvent(ctx->ccs[cur], ctx->ev_cc_done[prev], 0);
    }
    ctx->last_w[cur].assign(w.begin(), w.end());
    ctx->last_r[cur].assign(r.begin(), r.end());
}
// the caller's buffers of a detection (both written) ...
static void order_detect_buffers(mrgingham_amd_ctx* ctx, int nframes, const DetectOut& o) {
    order_after_previous(ctx, {{(const char*)o.xy, (size_t)nframes * o.capacity * 8}, {(const char*)o.counts, (size_t)nframes * 4}}, {});
}
// ... and of a refinement or a chain: points and levels are written; of the per-frame counts one is written (a chain's
// point counts, a refinement's optional nrefined) and one read (a refinement's point counts; NULL: none)
static void order_point_buffers(mrgingham_amd_ctx* ctx, int nframes, int pitch, const double* d_points, const signed char* d_levels,
                                const int32_t* counts_w, const int32_t* counts_r) {
    const size_t np = (size_t)nframes * pitch;
    order_after_previous(ctx, {{(const char*)d_points, np * 16}, {(const char*)d_levels, np},
                               {(const char*)counts_w, counts_w ? (size_t)nframes * 4 : 0}},
                         {{(const char*)counts_r, counts_r ? (size_t)nframes * 4 : 0}});
}
void end_op(mrgingham_amd_ctx* ctx) {
    const int set = ctx->cur;
    hipMemsetAsync(ctx->counters2[set].p, 0, (size_t)(kMaxLevel + 1) * ctx->counters_nf * sizeof(int32_t), cur_cc(ctx));
    hipEventRecord(ctx->ev_cc_done[set], cur_cc(ctx));
    ctx->cc_pending[set] = true;
    // the set's status words, behind everything of this op that can set one (behind the event too: whoever waits for
    // the op does not wait for the copy; mrgingham_amd_sync waits for the stream) into their page-locked mirror
    // (ensure_level_set allocates it; without one, or when the copy cannot be queued, the sync makes a blocking copy)
    ctx->status_copied[set] = false;
    if (!ctx->status_pin[set].p) return;
    if (hipMemcpyAsync(ctx->status_pin[set].p, status_of(ctx, 0), ctx->status_pin[set].bytes, hipMemcpyDeviceToHost,
                       cur_cc(ctx)) == hipSuccess)
        ctx->status_copied[set] = true;
    else
        (void)hipGetLastError();  // (not left behind for the next call that asks)
}

static PyramidOut pyramid_out_of(mrgingham_amd_ctx* ctx, int max_level) {
    PyramidOut po{};
    const int top = max_level < 3 ? max_level : 3;
    for (int L = 1; L <= top; ++L) {
        po.out[L - 1] = (uint8_t*)cur_levels(ctx)[L].img.p;
        po.w[L - 1] = cur_levels(ctx)[L].w;
        po.h[L - 1] = cur_levels(ctx)[L].h;
    }
    return po;
}
// Level images of levels [1, max_level] of the batch into the level scratch, on the pixel stream.
// `levels_1_to_3` false: those come out of the level-0 response kernel (launch_chess_pyramid)
void queue_level_images(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int max_level, bool levels_1_to_3,
                        bool gentle) {
    const FrameBatch fb{fr->frames, fr->frame_pitch, fr->width, fr->height, fr->stride};
    const int top = max_level < 3 ? max_level : 3;
    if (top >= 1 && levels_1_to_3) launch_pyramid(fb, pyramid_out_of(ctx, max_level), top, fr->nframes, ctx->pix, gentle);
    for (int L = 4; L <= max_level; ++L)
        launch_decimate(fb, L, (uint8_t*)cur_levels(ctx)[L].img.p, (long long)cur_levels(ctx)[L].w * cur_levels(ctx)[L].h,
                        cur_levels(ctx)[L].w, cur_levels(ctx)[L].h, 0, fr->nframes, ctx->pix);
}

LevelBatch level_batch_of(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int level) {
    LevelScratch& L = cur_levels(ctx)[level];
    LevelBatch lb;
    lb.nframes = fr->nframes;
    lb.w = L.w;
    lb.h = L.h;
    if (level == 0) {
        lb.img = fr->frames;
        lb.img_pitch = fr->frame_pitch;
        lb.img_stride = fr->stride;
    } else {
        lb.img = (const uint8_t*)L.img.p;
        lb.img_pitch = (long long)L.w * L.h;
        lb.img_stride = L.w;
    }
    lb.resp = (int16_t*)L.resp.p;
    lb.resp_pitch = (long long)L.w * L.h;
    if (level == 0 && ctx->clk_on) lb.clk = (unsigned long long*)ctx->clk.p;  // (mrgingham_amd_sclk_mhz)
    return lb;
}
// ChESS response (+ hot list) of one level for the whole batch on the pixel
// stream; records ev_pix[level].  Level images of levels > 0 must already be queued.
LevelBatch queue_level_chess(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int level) {
    const LevelBatch lb = level_batch_of(ctx, fr, level);
    launch_chess_any(ctx, lb, tables_of(ctx, level), fr->nframes, true, true, ctx->pix, level == 0);
    hipEventRecord(ctx->ev_pix[level], ctx->pix);
    note_pending(ctx, level, fr->nframes);
    return lb;
}

// ChESS responses (+ hot lists) of levels hi .. lo of the batch on the pixel stream, top-down: lbs[L] = what was
// launched for level L, lev_ev[L] = the event its response is done behind; the levels are noted as pending.
// Levels 3 (or hi) .. lo go in ONE launch when the options and the shapes allow it, and share one event: a boundary
// gets one packet (see KERNEL TIMING); otherwise one launch per level.  `merge_l0` (chain_batch under option
// "multi_level_launch" 2, whose lo is 1): level 0 goes into that one launch as well -- it is not launched on its own
// here.  Returns the levels in the merged launch, 0 if there is none.
// Kernel timing brackets the merged launch when level 0 is inside it.  `l0_mark` (or NULL): level 0 follows on its own
// right behind these levels; with timing on, the event behind a merged launch is then a timing mark that the caller
// opens the level-0 pair with (*l0_mark) instead of recording another.
int queue_chess_levels(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int hi, int lo, bool merge_l0, LevelBatch* lbs,
                       hipEvent_t* lev_ev, hipEvent_t* l0_mark) {
    const int nf = fr->nframes;
    const int top = hi < 3 ? hi : 3;
    const int lowest = merge_l0 ? 0 : lo;  // lowest level inside the merged launch
    auto one_level = [&](int L) {
        lbs[L] = queue_level_chess(ctx, fr, L);
        lev_ev[L] = ctx->ev_pix[L];
    };
    bool merged = false;
    if (top - lowest >= 1 && !ctx->use_v0 && ctx->multi_level) {
        LevelBatch mlb[4];
        CompTables mt[4];
        int n = 0;
        for (int L = lowest; L <= top; ++L, ++n) {  // largest level first
            mlb[n] = level_batch_of(ctx, fr, L);
            mt[n] = tables_of(ctx, L);
        }
        // decided BEFORE anything is queued: a level must not be appended to its hot list twice
        if (chess_multi_ok(mlb, n, nf)) {
            for (int L = hi; L > top; --L) one_level(L);
            hipEvent_t e0 = timing_open(ctx, ctx->pix, merge_l0 && ctx->timing);  // all levels in one launch: that launch is what is timed
            merged =
#ifdef MRG_EXPERIMENT
                ((ctx->chess_variant_hot & 16) && launch_chess16_multi(mlb, mt, n, nf, ctx->pix)) ||
#endif
                launch_chess_multi(mlb, mt, n, nf, ctx->pix, ctx->chess_seg);
            if (merged) {
                hipEvent_t em;
                if (!e0 && l0_mark && ctx->timing) em = *l0_mark = timing_open(ctx, ctx->pix, true);
                else em = timing_close(ctx, ctx->pix, e0, ctx->ev_pix[top]);
                for (int L = top; L >= lowest; --L) {
                    lbs[L] = mlb[L - lowest];
                    lev_ev[L] = em;
                    note_pending(ctx, L, nf);
                }
            } else if (e0) {
                ctx->timing_events.idle.push_back(e0);
            }
        }
    }
    for (int L = merged ? lowest - 1 : hi; L >= lo; --L) one_level(L);
    return merged ? top - lowest + 1 : 0;
}

// SPARSE REFINEMENT of the points in `io` (at pyramid level `top`, level images of all levels in the current set's
// scratch) through levels top-1 .. 0, on the current set's component stream, level by level: list the cells around the
// points (sparse_cells_kernel for the first level, the refinement kernel of the level above for the others) ->
// response + hot masks in those cells (chess_cells_kernel) -> refinement out of LDS on exactly those hot pixels
// (window mode, `marked<BOXED = true>`).  A frame the LDS kernel cannot take (a blob that reaches the edge of its
// cells, > 512 points, > 2048 hot pixels in the cells that no band cut separates) sets kStatusSparse in its status
// words -- at that level and, because nobody lists its cells any more, at every level below -- and is REPEATED DENSELY
// behind the last sparse level, on the device, before the call completes: its points go back to where they started
// (`restore`), the ordinary response kernel computes its levels and the global-memory refinement replays them, on
// the flagged frames alone (see the end of this function), and the flags are cleared.  So the outputs are the dense
// schedule's on every frame, with no host round trip and nothing for the caller to repeat.
// `dense_only`: no sparse pass at all -- the ordinary kernels on every frame, level by level, on the component stream
// (the refinement of find_boards_submit when the sparse schedule is switched off or does not pay).
int queue_sparse_levels(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int top, RefineIO io,
                        const SparseRestore& restore, bool dense_only) {
    auto& ps = ctx->pts[ctx->cur];
    const int nf = fr->nframes;
    hipStream_t cc = cur_cc(ctx);
    LevelBatch lbs[kMaxLevel + 1];
    if (dense_only) {
        for (int L = top - 1; L >= 0; --L) {
            lbs[L] = level_batch_of(ctx, fr, L);
            const CompTables t = tables_of(ctx, L);
            launch_chess_any(ctx, lbs[L], t, nf, true, true, cc, false);
            launch_cc_refine(lbs[L], t, L, io, 0, nf, cc);
            note_pending(ctx, L, nf);
        }
        return 0;
    }
    const int list_pitch = kCellsPerPoint * io.pitch;
    io.subsets = ctx->sparse_subsets;
    uint32_t* const lists[2] = {(uint32_t*)ps.cell_list.p, (uint32_t*)ps.cell_list.p + (size_t)nf * list_pitch};
    io.list_pitch = list_pitch;
    int32_t* cnt = (int32_t*)ps.cell_cnt.p;  // [level][frame][kCellHdr]
    for (int L = top - 1; L >= 0; --L) {
        lbs[L] = level_batch_of(ctx, fr, L);
        CompTables t = tables_of(ctx, L);
        t.lds_path |= kLdsPathSparse;
        io.cell_list = lists[L & 1];
        io.next_list = lists[(L & 1) ^ 1];
        io.cell_cnt = cnt + (size_t)L * nf * kCellHdr;
        // the cells of this level: listed by the refinement kernel of the level above, by a kernel of its own
        // for the first one (its points come out of the detection / from the caller)
        if (L == top - 1)
            launch_sparse_cells(lbs[L], t, L, io, io.cell_list, cnt + (size_t)L * nf * kCellHdr, list_pitch, 0, nf, cc, cnt, nf);
        launch_chess_cells(lbs[L], t, io.cell_list, io.cell_cnt, list_pitch, 0, nf, cc);
        io.next_cnt = nullptr;
        if (L > 0) {
            const LevelScratch& nx = cur_levels(ctx)[L - 1];
            io.next_cnt = cnt + (size_t)(L - 1) * nf * kCellHdr;
            io.next_w = nx.w;
            io.next_h = nx.h;
            io.next_max_items = tables_of(ctx, L - 1).gidx_pitch / 4;
        }
        launch_cc_refine(lbs[L], t, L, io, 0, nf, cc);
        note_pending(ctx, L, nf);
    }
    // the dense repeat of what was reported (flag = the level-0 status word: a frame given up at any level is given up
    // at every level below it): three small launches -- the flagged frames as a list; their dense responses at every
    // level (one grid, laid out for kOnlySlots frames whatever the batch); per listed frame restore + the refinement of
    // every level + clear.  Every kernel boundary of this chain costs ~10 us whether or not a frame is flagged, and a
    // full-size grid of the response kernel that finds nothing to do still waits for LDS and registers on a chip the
    // pixel stream keeps full: eleven full-size launches were 8 % of a sparse step.
    // (Not queue_chess_levels: this runs on the component stream, over a frame list, with no event and nothing to note.)
    int32_t* flags = status_of(ctx, 0);
    int32_t* list = (int32_t*)ps.flag_list.p;
    launch_sparse_flag_list(flags, nf, list, cc);
    RefineIO dio = io;
    dio.cell_list = nullptr;
    dio.cell_cnt = nullptr;
    dio.list_pitch = 0;
    dio.next_cnt = nullptr;
    LevelBatch mlb[kRefineLevelsMax];   // largest level first (launch_chess_multi)
    CompTables mt[kRefineLevelsMax], lt[kRefineLevelsMax];
    for (int L = 0; L < top; ++L) {
        lt[L] = tables_of(ctx, L);
        mlb[L] = lbs[L];
        mt[L] = lt[L];
        mt[L].only = list;
    }
    const bool merged = top >= 2 && chess_multi_ok(mlb, top, nf) && launch_chess_multi(mlb, mt, top, nf, cc, ctx->chess_seg);
    if (!merged)
        for (int L = top - 1; L >= 0; --L) launch_chess(lbs[L], mt[L], 0, nf, true, true, cc, ctx->chess_seg);
    launch_cc_refine_flagged_levels(lbs, lt, top, dio, restore, list, flags, ctx->counters_nf, (int32_t*)ctx->sparse_stat.p, cc);
    return 0;
}

// ONE-LEVEL CALLS (detect_batch, refine_batch, cc_on_response_batch): what such a call leaves in the caller's buffers --
// the candidates of a detection, or the points it was given, refined
struct LevelCallOut {
    bool detect;
    DetectOut det;
    double* points;
    signed char* levels;
    const int32_t* npoints;
    int pitch;
    int32_t* nrefined;
};
static int check_level_call_out(mrgingham_amd_ctx* ctx, const LevelCallOut& o) {
    if (o.detect && (!o.det.xy || !o.det.counts || o.det.capacity < 0)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "NULL outputs");
    if (!o.detect && (!o.points || !o.levels || !o.npoints || o.pitch <= 0)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "NULL point buffers");
    return 0;
}
// the component stream of such a call and its end: behind the response of `lb` on the pixel stream (`ready`), the
// component search over the tables of scratch level `tl`; `level` is the pyramid level of the coordinates
static int finish_level_call(mrgingham_amd_ctx* ctx, const LevelBatch& lb, int tl, int level, hipEvent_t ready, const LevelCallOut& o) {
    if (o.detect) order_detect_buffers(ctx, lb.nframes, o.det);
    else order_point_buffers(ctx, lb.nframes, o.pitch, o.points, o.levels, o.nrefined, o.npoints);
    MRG_HIP_CHECK(hipStreamWaitEvent(cur_cc(ctx), ready, 0));
    if (o.detect) launch_cc_detect(lb, tables_of(ctx, tl), level, o.det, 0, lb.nframes, cur_cc(ctx));
    else launch_cc_refine(lb, tables_of(ctx, tl), level, refine_io_of(ctx, ctx->cur, o.points, o.levels, o.npoints, o.pitch, o.nrefined),
                          0, lb.nframes, cur_cc(ctx));
    end_op(ctx);
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}
// the scratch of such a call (`pitch` points per frame when it refines: `points`), its op begun, and its pixel stream:
// level image (w x h) and response of `level`
static int level_pixels(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int level, int w, int h, int pitch, bool points,
                        LevelBatch& lb) {
    int rc;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    if ((rc = choose_sets(ctx, fr))) return rc;
    if ((rc = ensure_level(ctx, level, fr->nframes, fr->width, fr->height, pitch))) return rc;
    if (points && (rc = ensure_points(ctx, fr->nframes, pitch))) return rc;
    begin_op(ctx, level);
    if (level > 0) launch_one_level_image(fr, level, (uint8_t*)cur_levels(ctx)[level].img.p, w, h, ctx->pix);
    lb = queue_level_chess(ctx, fr, level);
    return 0;
}
// detect_batch / refine_batch: level image and response of `level` on the pixel stream, its component search behind them
static int level_call(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int level, const LevelCallOut& o) {
    int rc = validate_frames(ctx, fr);
    if (rc) return rc;
    fb_drain(ctx);
    int w, h;
    if (level_dims(fr->width, fr->height, level, &w, &h))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "Got an unreasonable image_pyramid_level = %d", level);
    if (fr->nframes == 0) return 0;
    if ((rc = check_level_call_out(ctx, o))) return rc;
    LevelBatch lb;
    if ((rc = level_pixels(ctx, fr, level, w, h, o.detect ? 0 : o.pitch, !o.detect, lb))) return rc;
    return finish_level_call(ctx, lb, level, level, ctx->ev_pix[level], o);
}

// CHAIN CALLS.  What the pixel stream of a step hands to its component stream:
struct ChainPlan {
    LevelBatch lbs[kMaxLevel + 1];          // per level: what its response was launched over
    hipEvent_t lev_ev[kMaxLevel + 1] = {};  // per level: the pixel-stream event its response is done behind
    bool sparse = false;                    // only the start level is there: the levels below follow on the component stream
    bool fused = false;                     // level 0 ran FIRST on the pixel stream (it wrote the level images)
};

// SPARSE REFINEMENT.  The dense schedule computes the response of levels start-1 .. 0 for whole frames and then
// looks at it around ~100 points.  Here: every level image in one pass over the frames (pyramid kernel; the
// variance windows need them around any peak), the dense response only at the START level (its detection needs
// every component), and below it, level by level on the component stream: queue_sparse_levels.
static void chain_pixels_sparse(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int start_level, ChainPlan& p) {
    p.sparse = true;
    // what is timed in this mode (mrgingham_amd_chess_kernel_ms): the kernel that reads the frames, i.e. the launch
    // that writes the level images (the dominant kernel of a sparse step; 1 B/px read + 0.328 B/px written)
    hipEvent_t e0 = timing_open(ctx, ctx->pix, ctx->timing);
    queue_level_images(ctx, fr, start_level, true, true);
    timing_close(ctx, ctx->pix, e0, nullptr);
    p.lbs[start_level] = queue_level_chess(ctx, fr, start_level);
    p.lev_ev[start_level] = ctx->ev_pix[start_level];
    ctx->last_fused = 0;
    ctx->last_merged = -1;  // (mrgingham_amd_chain_info: a sparse step)
}

// The dense schedule.  Frames of whole 16 x 8 blocks (every BASELINE size): level 0 first, its kernel also
// writes the level images 1..3 out of the rows it holds in LDS anyway, so the batch is read from HBM
// once instead of twice; the small levels follow.  Other shapes: every level image in one pass over
// the frames (pyramid kernel), then the responses top-down, level 0 last.
static void chain_pixels_dense(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int start_level, ChainPlan& p) {
    const int nf = fr->nframes;
    const bool merge_l0 = ctx->multi_level == 2;  // level 0 inside the merged launch of the small levels, if there is one
    p.lbs[0] = level_batch_of(ctx, fr, 0);
    p.fused = ctx->fuse_pyramid && !ctx->use_v0 && start_level >= 1 && !merge_l0 && chess_pyramid_ok(p.lbs[0], nf);
    queue_level_images(ctx, fr, start_level, !p.fused);
    if (p.fused) {
        hipEvent_t e0 = timing_open(ctx, ctx->pix, ctx->timing);
#ifdef MRG_EXPERIMENT
        if (!((ctx->chess_variant_hot & 32) && launch_chess16_pyramid(p.lbs[0], tables_of(ctx, 0), pyramid_out_of(ctx, start_level), nf, ctx->pix)))
#endif
            launch_chess_pyramid(p.lbs[0], tables_of(ctx, 0), pyramid_out_of(ctx, start_level), nf, ctx->pix, ctx->chess_seg);
        // timing off: no event here, the one behind level 1 stands in (the component chain reaches level 0 last anyway)
        p.lev_ev[0] = timing_close(ctx, ctx->pix, e0, nullptr);
        note_pending(ctx, 0, nf);
    }
    // levels start .. 1: 3 (or the top), 2, 1 -- or all of them, level 0 included -- in one launch when the shapes allow it
    hipEvent_t before_l0 = nullptr;  // timing mode: an event recorded right before the level-0 launch, if there is one
    const int merged = queue_chess_levels(ctx, fr, start_level, 1, merge_l0, p.lbs, p.lev_ev, p.fused ? nullptr : &before_l0);
    if (p.fused) {
        if (!p.lev_ev[0]) p.lev_ev[0] = p.lev_ev[1];
    } else if (!(merged && merge_l0)) {  // level 0 on its own: the launch that is timed, its closing mark the hand-over event
        hipEvent_t e0 = timing_open(ctx, ctx->pix, ctx->timing, before_l0);
        launch_chess_any(ctx, p.lbs[0], tables_of(ctx, 0), nf, true, true, ctx->pix, false);
        p.lev_ev[0] = timing_close(ctx, ctx->pix, e0, ctx->ev_pix[0]);
        note_pending(ctx, 0, nf);
    }
    ctx->last_fused = p.fused;
    ctx->last_merged = merged;
}

// the scratch of a chain call, which schedule it takes (*sparse), and its op begun
static int chain_begin(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int start_level, int points_pitch, bool* sparse) {
    int rc;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    *sparse = sparse_applies(ctx, start_level, (long long)fr->width * fr->height * fr->nframes);
    if (*sparse) ctx->sparse_seen = true;
    if ((rc = choose_sets(ctx, fr))) return rc;
    for (int L = 0; L <= start_level; ++L)
        if ((rc = ensure_level(ctx, L, fr->nframes, fr->width, fr->height, points_pitch))) return rc;
    if ((rc = ensure_points(ctx, fr->nframes, points_pitch))) return rc;
    if (*sparse && !ctx->sparse_stat.p) {
        if ((rc = ensure(ctx, ctx->sparse_stat, 256))) return rc;
        MRG_HIP_CHECK(hipMemset(ctx->sparse_stat.p, 0, 256));
    }
    begin_op(ctx, start_level);
    return 0;
}
// the pixel stream of a chain call: the launch plan of the step
static void chain_pixels(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int start_level, bool sparse, ChainPlan& p) {
    if (sparse) chain_pixels_sparse(ctx, fr, start_level, p);
    else chain_pixels_dense(ctx, fr, start_level, p);
}

// component stream: detect at the top (mrgingham.cc:50), candidates -> corners
// (find_grid.cc:353-354), then refine level by level (mrgingham.cc:87-99)
static int chain_components(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int start_level, const ChainPlan& p,
                            const DetectOut& out, const RefineIO& io) {
    const int nf = fr->nframes;
    hipStream_t cc = cur_cc(ctx);
    if (p.sparse) {
        MRG_HIP_CHECK(hipStreamWaitEvent(cc, p.lev_ev[start_level], 0));
        launch_cc_detect(p.lbs[start_level], tables_of(ctx, start_level), start_level, out, 0, nf, cc);
        return queue_sparse_levels(ctx, fr, start_level, io, SparseRestore{out.xy, out.capacity, start_level, nullptr, nullptr});
    }
    // which pixel-stream event a level's search waits for: level 0 runs LAST on the pixel stream in the
    // classic order (cc_schedule 1 holds levels 1 and 0 back until then, 2 holds everything back) and
    // FIRST in the fused order (then level 1 is the last)
    auto gate_of = [&](int L) {
        if (p.fused) return p.lev_ev[ctx->cc_schedule == 2 ? 1 : (L > 1 ? L : 1)];
        return p.lev_ev[(ctx->cc_schedule == 1 && L <= 1) || ctx->cc_schedule == 2 ? 0 : L];
    };
    const bool no_cc = (ctx->cc_lds & 128) != 0;  // timing experiment only (tools/interference_ab.py): pixel kernels alone
    MRG_HIP_CHECK(hipStreamWaitEvent(cc, gate_of(start_level), 0));
    if (!no_cc) launch_cc_detect(p.lbs[start_level], tables_of(ctx, start_level), start_level, out, 0, nf, cc);
    for (int L = start_level - 1; L >= 0; --L) {
        MRG_HIP_CHECK(hipStreamWaitEvent(cc, gate_of(L), 0));
        if (!no_cc) launch_cc_refine(p.lbs[L], tables_of(ctx, L), L, io, 0, nf, cc);
    }
    return 0;
}

// cc_on_response_batch: the scratch of the call (`pitch` points per frame when it refines: `points`), its op begun, and
// its pixel stream: the caller's response into the scratch, its hot list beside it
static int response_pixels(mrgingham_amd_ctx* ctx, const int16_t* d_response, const uint8_t* d_level_image, int nframes, int w, int h,
                           int pitch, bool points, LevelBatch& lb) {
    int rc;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    // the level-0 scratch of a w x h "frame": the response is the level image's as far as the
    // component search is concerned; `level` only enters through the coordinate scale
    if ((rc = ensure_level(ctx, 0, nframes, w, h, pitch))) return rc;
    if (points && (rc = ensure_points(ctx, nframes, pitch))) return rc;
    begin_op(ctx, 0);
    lb.nframes = nframes;
    lb.w = w;
    lb.h = h;
    lb.img = d_level_image;
    lb.img_pitch = (long long)w * h;
    lb.img_stride = w;
    lb.resp = (int16_t*)cur_levels(ctx)[0].resp.p;
    lb.resp_pitch = (long long)w * h;
    launch_hot_from_response(d_response, lb, tables_of(ctx, 0), 0, nframes, ctx->pix);
    hipEventRecord(ctx->ev_pix[0], ctx->pix);
    note_pending(ctx, 0, nframes);
    return 0;
}

// TEST HOOK (mrgingham_amd_debug_pixel_stage): behind the pixel stream of an op that queued nothing else -- the hot
// counters to the host (end_op zeroes them for the set's next op), the op ended, everything waited for
static int finish_pixel_stage(mrgingham_amd_ctx* ctx, int nframes, unsigned img_levels, unsigned list_levels) {
    order_after_previous(ctx, {}, {});  // (this op touches no buffer of the caller's)
    MRG_HIP_CHECK(hipStreamSynchronize(ctx->pix));
    auto& ps = ctx->pixel_stage;
    ps.cnf = ctx->counters_nf;
    ps.hot_cnt.resize((size_t)(kMaxLevel + 1) * ps.cnf);
    MRG_HIP_CHECK(hipMemcpy(ps.hot_cnt.data(), hot_cnt_of(ctx, 0), ps.hot_cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    end_op(ctx);
    MRG_HIP_CHECK(hipGetLastError());
    ps.set = ctx->cur;
    ps.nframes = nframes;
    ps.img_levels = img_levels;
    ps.list_levels = list_levels;
    ps.valid = true;
    return mrgingham_amd_sync(ctx);
}

}  // namespace mrg

using namespace mrg;

extern "C" {

int mrgingham_amd_detect_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int level, int32_t* d_xy,
                               int capacity_per_frame, int32_t* d_counts) {
    return level_call(ctx, fr, level, LevelCallOut{true, DetectOut{d_xy, capacity_per_frame, d_counts}, nullptr, nullptr, nullptr, 0, nullptr});
}

int mrgingham_amd_refine_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int level, double* d_points,
                               signed char* d_levels, const int32_t* d_npoints, int points_pitch,
                               int32_t* d_nrefined) {
    return level_call(ctx, fr, level, LevelCallOut{false, DetectOut{}, d_points, d_levels, d_npoints, points_pitch, d_nrefined});
}

int mrgingham_amd_chain_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int start_level,
                              double* d_points, signed char* d_levels, int32_t* d_npoints, int points_pitch) {
    // checks and scratch
    int rc = validate_frames(ctx, fr);
    if (rc) return rc;
    fb_drain(ctx);
    int w, h;
    if (level_dims(fr->width, fr->height, start_level, &w, &h))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "Got an unreasonable image_pyramid_level = %d", start_level);
    if (fr->nframes == 0) return 0;
    if (!d_points || !d_levels || !d_npoints || points_pitch <= 0)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "NULL point buffers");
    bool sparse;
    if ((rc = chain_begin(ctx, fr, start_level, points_pitch, &sparse))) return rc;
    auto& ps = ctx->pts[ctx->cur];
    DetectOut out{(int32_t*)ps.cand_xy.p, points_pitch, (int32_t*)ps.cand_counts.p};
    out.points = d_points;
    out.levels = d_levels;
    out.npoints = d_npoints;
    out.points_pitch = points_pitch;
    const RefineIO io = refine_io_of(ctx, ctx->cur, d_points, d_levels, d_npoints, points_pitch, nullptr);
    order_point_buffers(ctx, fr->nframes, points_pitch, d_points, d_levels, d_npoints, nullptr);
    ChainPlan plan;
    chain_pixels(ctx, fr, start_level, sparse, plan);
    // the component stream, level by level behind it
    if ((rc = chain_components(ctx, fr, start_level, plan, out, io))) return rc;
    end_op(ctx);
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

int mrgingham_amd_cc_on_response_batch(mrgingham_amd_ctx* ctx, const int16_t* d_response,
                                       const uint8_t* d_level_image, int nframes, int w, int h, int level,
                                       int32_t* d_xy, int capacity_per_frame, int32_t* d_counts,
                                       double* d_points, signed char* d_levels, const int32_t* d_npoints,
                                       int points_pitch, int32_t* d_nrefined) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    fb_drain(ctx);
    const LevelCallOut o{d_xy != nullptr, DetectOut{d_xy, capacity_per_frame, d_counts}, d_points, d_levels, d_npoints, points_pitch, d_nrefined};
    if (o.detect == (d_points != nullptr)) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "exactly one of d_xy (detect) and d_points (refine)");
    if (nframes < 0 || w < 0 || h < 0 || w > 32767 || h > 32767 || level < 0 || level > kMaxLevel ||
        (nframes > 0 && (!d_response || !d_level_image)))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad response batch descriptor");
    int rc = check_level_call_out(ctx, o);
    if (rc) return rc;
    if (nframes == 0) return 0;
    LevelBatch lb;
    if ((rc = response_pixels(ctx, d_response, d_level_image, nframes, w, h, o.detect ? 0 : points_pitch, !o.detect, lb))) return rc;
    return finish_level_call(ctx, lb, 0, level, ctx->ev_pix[0], o);
}

int mrgingham_amd_debug_pixel_stage(mrgingham_amd_ctx* ctx, int mode, const mrgingham_amd_frames* fr, int level, int points_pitch,
                                    const int16_t* d_response) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (mode == MRGINGHAM_AMD_PIXELS_RESPONSE) {
        fb_drain(ctx);
        if (!fr || fr->nframes <= 0 || fr->width <= 0 || fr->height <= 0 || fr->width > 32767 || fr->height > 32767 || !d_response)
            return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad response batch descriptor");
        LevelBatch lb;
        const int rc = response_pixels(ctx, d_response, nullptr, fr->nframes, fr->width, fr->height, 0, false, lb);
        return rc ? rc : finish_pixel_stage(ctx, fr->nframes, 0, 1u);
    }
    if (mode != MRGINGHAM_AMD_PIXELS_CHAIN && mode != MRGINGHAM_AMD_PIXELS_LEVEL)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "unknown pixel stage %d", mode);
    int rc = validate_frames(ctx, fr);
    if (rc) return rc;
    fb_drain(ctx);
    int w, h;
    if (level_dims(fr->width, fr->height, level, &w, &h))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "Got an unreasonable image_pyramid_level = %d", level);
    if (fr->nframes == 0) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "no frames");
    if (mode == MRGINGHAM_AMD_PIXELS_LEVEL) {
        LevelBatch lb;
        if ((rc = level_pixels(ctx, fr, level, w, h, 0, false, lb))) return rc;
        return finish_pixel_stage(ctx, fr->nframes, level > 0 ? 1u << level : 0u, 1u << level);
    }
    if (points_pitch <= 0) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "points_pitch");
    bool sparse;
    if ((rc = chain_begin(ctx, fr, level, points_pitch, &sparse))) return rc;
    ChainPlan plan;
    chain_pixels(ctx, fr, level, sparse, plan);
    const unsigned all = (2u << level) - 1u;
    return finish_pixel_stage(ctx, fr->nframes, all & ~1u, sparse ? 1u << level : all);
}

int mrgingham_amd_debug_pixel_products(mrgingham_amd_ctx* ctx, int level, int frame, uint8_t* h_image, int16_t* h_response,
                                       int32_t* h_hot_cnt, int32_t* h_cap, uint32_t* h_hot_xy, uint32_t* h_gidx) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    const auto& ps = ctx->pixel_stage;
    if (!ps.valid) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "no pixel stage to read: mrgingham_amd_debug_pixel_stage comes first");
    const bool lists = h_response || h_hot_cnt || h_cap || h_hot_xy || h_gidx;
    if (level < 0 || level > kMaxLevel || frame < 0 || frame >= ps.nframes || (h_image && !(ps.img_levels >> level & 1u)) ||
        (lists && !(ps.list_levels >> level & 1u)) || (h_hot_xy && (!h_hot_cnt || !h_cap)))
    {
        ctx->err = "not a product of the last pixel stage";  // (quiet: callers probe with this)
        return MRGINGHAM_AMD_ERR_ARG;
    }
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    const LevelScratch& L = ctx->lvs[ps.set][level];
    const size_t px = (size_t)L.w * L.h, gpx = (size_t)((L.w + 7) / 8) * L.h;
    if (h_image) MRG_HIP_CHECK(hipMemcpy(h_image, (const uint8_t*)L.img.p + frame * px, px, hipMemcpyDeviceToHost));
    if (h_response) MRG_HIP_CHECK(hipMemcpy(h_response, (const int16_t*)L.resp.p + frame * px, px * 2, hipMemcpyDeviceToHost));
    if (h_hot_cnt) *h_hot_cnt = ps.hot_cnt[(size_t)level * ps.cnf + frame];
    if (h_cap) *h_cap = L.cap;
    if (h_hot_xy) {
        const size_t n = (size_t)(*h_hot_cnt < L.cap ? (*h_hot_cnt > 0 ? *h_hot_cnt : 0) : L.cap);
        if (n) MRG_HIP_CHECK(hipMemcpy(h_hot_xy, (const uint32_t*)L.hot_xy.p + (size_t)frame * L.cap, n * 4, hipMemcpyDeviceToHost));
    }
    if (h_gidx && gpx) MRG_HIP_CHECK(hipMemcpy(h_gidx, (const uint2*)L.gidx.p + frame * gpx, gpx * 8, hipMemcpyDeviceToHost));
    return MRGINGHAM_AMD_OK;
}

}  // extern "C"
