// Host side of libmrgingham_amd.so, the full board detector (mrgingham::find_chessboard_from_image_array over a
// batch): the synchronous level search, the pipelined submit / collect job and its statistics, and the one-frame board
// search of the reference symbols (find_board_on_device).
#include <stdio.h>
#include <string.h>

#include <chrono>

#include "ctx.h"
#include "grid_phases.h"

namespace mrg {

// Frame k of a batch as a batch of its own.
static mrgingham_amd_frames frame_of(const mrgingham_amd_frames& fr, int k) {
    return mrgingham_amd_frames{fr.frames + (size_t)k * fr.frame_pitch, fr.frame_pitch, 1, fr.width, fr.height, fr.stride};
}

// The single-frame context on the same device as `ctx` (see mrgingham_amd_ctx::one), made on first use; NULL, with the
// error on `ctx`, when it cannot be made.
static mrgingham_amd_ctx* same_device_ctx(mrgingham_amd_ctx* ctx) {
    if (!ctx->one) {
        ctx->one = mrgingham_amd_create(ctx->device);
        if (ctx->one) ctx->one->cap_shift = ctx->cap_shift;
        if (ctx->one) ctx->one->scratch_fill = ctx->scratch_fill;
        hipSetDevice(ctx->device);
    }
    if (!ctx->one) fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "no single-frame context");
    return ctx->one;
}

// Frames with more candidates than a batch buffer keeps (clutter), or whose component tables overflowed (dense texture,
// count -1): the reference runs the grid finder on ALL candidates (mrgingham.cc:50-51), so such a frame is detected again
// on its own, with exact capacity and the one-entry-per-pixel retry, on the single-frame context of this device.
// `index`: the frame's number in the caller's batch, for the message.
static int detect_full_capacity(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames& fr, int k, int level, int index,
                                std::vector<int32_t>& xy, int32_t* count) {
    mrgingham_amd_ctx* one = same_device_ctx(ctx);
    if (!one) return MRGINGHAM_AMD_ERR_DEVICE;
    const mrgingham_amd_frames f1 = frame_of(fr, k);
    if (!detect_one_frame_all(one, &f1, level, xy, count))
        return fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "frame %d, level %d: full-capacity detect failed", index, level);
    return 0;
}

// One board found at level L refined on its own, level by level, while something still refines (mrgingham.cc:81-99).
static void refine_board_alone(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, double* board, signed char* levels,
                               int N, int L, bool debug = false, const char* debug_image_filename = nullptr) {
    for (int l = L - 1; l >= 0; --l)
        if (refine_on_device(ctx, fr, board, levels, N, l, debug, debug_image_filename) <= 0) break;
}

// A board whose batch refinement overflowed the default tables (dense texture): refined on its own from level L down, on
// the single-frame context, which retries with a table entry per pixel.  Frame `index` of `h_levels` (may be NULL) gets
// its corners' levels.
static int refine_frame_alone(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames& fr, int k, double* board,
                              signed char* h_levels, int index, int N, int L) {
    mrgingham_amd_ctx* one = same_device_ctx(ctx);
    if (!one) return MRGINGHAM_AMD_ERR_DEVICE;
    const mrgingham_amd_frames f1 = frame_of(fr, k);
    std::vector<signed char> lv((size_t)N, (signed char)L);
    refine_board_alone(one, &f1, board, lv.data(), N, L);
    if (h_levels) memcpy(h_levels + (size_t)index * N, lv.data(), (size_t)N);
    return 0;
}

// The grid finder on n candidates (x, y) * 1000 (mrgingham.cc:51): true, and the gridn^2 corners in `out`, only when
// it found the whole board.  `scratch`: vectors a caller that runs it frame after frame reuses.
bool grid_of_candidates(const int32_t* xy, int n, int gridn, double* out, GridScratch* scratch) {
    GridScratch local;
    GridScratch& s = scratch ? *scratch : local;
    s.cand.resize((size_t)n);
    for (int i = 0; i < n; ++i) s.cand[i] = PointI{xy[2 * i], xy[2 * i + 1]};
    s.grid.clear();
    if (!find_grid_from_points(s.grid, s.cand, gridn) || (int)s.grid.size() != gridn * gridn) return false;
    memcpy(out, s.grid.data(), sizeof(double) * 2 * s.grid.size());
    return true;
}

// Option "find_boards_grid" 1: every host finder call of such a job starts its neighbour rings at the canonical neighbour
// (grid.cpp: GridPerturbation::canonical_start), the one ring rule of the device finder -- on this thread, while this lives
struct CanonicalRings {
    const bool saved = g_grid_perturbation.canonical_start;
    explicit CanonicalRings(bool on) { if (on) g_grid_perturbation.canonical_start = true; }
    ~CanonicalRings() { g_grid_perturbation.canonical_start = saved; }
};

static double fb_now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void add_elapsed_ms(double& total, hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (a && hipEventElapsedTime(&ms, a, b) == hipSuccess) total += ms;
}

// grid-finder threads of the find_boards calls: <= 0 = one per core the process may use, at most 32 (the grid finder
// takes ~0.1 ms per frame and level: a few dozen threads cover a batch)
int host_threads(int nthreads) {
    if (nthreads <= 0) {
        nthreads = (int)std::thread::hardware_concurrency();
        if (nthreads > 32) nthreads = 32;
    }
    return nthreads > 0 ? nthreads : 1;
}

// The level search of mrgingham_amd_find_boards_batch, SYNCHRONOUS form: per level from `first` down to `last` one
// batched device pass over the frames still open (`open0`, ascending; the others must have h_found_level >= 0
// already), the grid finder on host threads, the boards found at the level refined densely level by level.  The
// pipelined form (find_boards_submit / _collect below) uses it for what its first pass leaves open, and option
// "find_boards_pipeline" 0 for everything.
// `h_levels` (may be NULL): per frame the gridn^2 refinement levels of its corners (what the reference's
// refinement_level array holds, mrgingham.cc:81-99); `do_refine` false: the boards stay as the grid finder made them.
static int find_boards_sync_levels(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int gridn, int first, int last,
                                   double* h_boards, signed char* h_found_level, int nthreads, std::vector<int> open,
                                   bool do_refine = true, signed char* h_levels = nullptr, bool canonical = false) {
    int rc = 0;
    const int B = fr->nframes, N = gridn * gridn;
    const int cap = 4 * N + 64;  // candidates kept per frame for the grid finder
    nthreads = host_threads(nthreads);

    DevBuf &d_xy = ctx->fb_xy, &d_cnt = ctx->fb_cnt, &d_pts = ctx->fb_pts, &d_lv = ctx->fb_lv, &d_np = ctx->fb_np;
    if ((rc = ensure(ctx, d_xy, (size_t)B * cap * 8)) || (rc = ensure(ctx, d_cnt, (size_t)B * 4)) ||
        (rc = ensure(ctx, d_pts, (size_t)B * N * 16)) || (rc = ensure(ctx, d_lv, (size_t)B * N)) ||
        (rc = ensure(ctx, d_np, (size_t)B * 4)))
        return rc;
    std::vector<int32_t> h_xy((size_t)B * cap * 2), h_cnt(B), h_np(B, 0);
    std::vector<signed char> h_lv((size_t)B * N, 0);
    std::vector<double> h_pts((size_t)B * N * 2);

    // A dense copy of a few frames of the batch, so that a late level only runs on the frames that
    // still need it (one straggler must not cost the whole batch another two ChESS passes).
    const size_t frame_bytes = (size_t)fr->width * fr->height;
    auto gather = [&](DevBuf& buf, const std::vector<int>& idx, mrgingham_amd_frames* sub) -> int {
        int r = ensure(ctx, buf, frame_bytes * idx.size() + 64);
        if (r) return r;
        for (size_t k = 0; k < idx.size(); ++k)
            MRG_HIP_CHECK(copy_rows_async((char*)buf.p + k * frame_bytes, fr->width,
                                          fr->frames + (size_t)idx[k] * fr->frame_pitch, fr->stride, fr->width,
                                          fr->height, hipMemcpyDeviceToDevice, ctx->pix));
        *sub = mrgingham_amd_frames{(const uint8_t*)buf.p, (int64_t)frame_bytes, (int)idx.size(), fr->width, fr->height,
                                    fr->width};
        return 0;
    };

#ifdef MRG_EXPERIMENT
    static const bool dbg_t = getenv("MRG_DBG_FB") != nullptr;
#else
    constexpr bool dbg_t = false;
#endif
    double t_prev = fb_now();
    auto lap = [&](const char* what, int L, int n) { if (dbg_t) { const double t = fb_now(); fprintf(stderr, "  [fb] L%d %-14s %3d frames %7.3f ms\n", L, what, n, t - t_prev); t_prev = t; } };

    std::vector<int> cur_idx(B);             // original index of every frame of the batch the detector runs on
    for (int f = 0; f < B; ++f) cur_idx[f] = f;
    mrgingham_amd_frames cur = *fr, rsub;

    for (int L = first; L >= last && !open.empty(); --L) {
        // (a) candidates at level L of the frames still open (compacted once at most half are left)
        if (open.size() * 2 <= cur_idx.size()) {
            if ((rc = gather(ctx->fb_frames, open, &cur))) break;
            cur_idx = open;
        }
        const int nb = (int)cur_idx.size();
        if ((rc = mrgingham_amd_detect_batch(ctx, &cur, L, (int32_t*)d_xy.p, cap, (int32_t*)d_cnt.p))) break;
        rc = mrgingham_amd_sync(ctx);
        if (rc == MRGINGHAM_AMD_ERR_CAPACITY) rc = 0;  // the frames concerned report count -1: handled below
        if (rc) break;
        if (hipMemcpy(h_cnt.data(), d_cnt.p, (size_t)nb * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(h_xy.data(), d_xy.p, (size_t)nb * cap * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "candidate download failed");
            break;
        }
        // frames whose candidates did not fit: again at full capacity (detect_full_capacity)
        std::vector<std::vector<int32_t>> big(nb);
        for (int k = 0; k < nb && !rc; ++k)
            if (h_found_level[cur_idx[k]] < 0 && (h_cnt[k] < 0 || h_cnt[k] > cap))
                rc = detect_full_capacity(ctx, cur, k, L, cur_idx[k], big[k], &h_cnt[k]);
        if (rc) break;
        lap("detect+D2H", L, nb);
        // (b) grid finder on host threads (mrgingham.cc:51), for the frames still without a board
        std::vector<char> found_now(nb, 0);
        std::atomic<int> next{0};
        auto worker = [&]() {
            GridScratch scratch;
            const CanonicalRings rings(canonical);
            for (int k; (k = next.fetch_add(1)) < nb;) {
                const int f = cur_idx[k];
                if (h_found_level[f] >= 0 || h_cnt[k] < N) continue;
                const int32_t* src = big[k].empty() ? &h_xy[(size_t)k * cap * 2] : big[k].data();
                found_now[k] = grid_of_candidates(src, h_cnt[k], gridn, h_boards + (size_t)f * N * 2, &scratch);
            }
        };
        ctx->pool.run(nthreads < nb ? nthreads : nb, worker);
        std::vector<int> found_pos;  // positions within the current batch
        for (int k = 0; k < nb; ++k)
            if (found_now[k]) {
                h_found_level[cur_idx[k]] = (signed char)L;
                found_pos.push_back(k);
                if (h_levels) memset(h_levels + (size_t)cur_idx[k] * N, L, (size_t)N);
            }
        lap("grid finder", L, (int)found_pos.size());
        if (found_pos.empty()) continue;
        {
            std::vector<int> still;
            for (int f : open)
                if (h_found_level[f] < 0) still.push_back(f);
            open.swap(still);
        }
        if (L == 0 || !do_refine) continue;
        // (c) refine the boards found at this level down to level 0 (mrgingham.cc:81-99): on the current
        // batch with zero points for the other frames, or on a dense copy of just those frames
        const mrgingham_amd_frames* rb = &cur;
        std::vector<int> ridx;  // position in the refine batch -> original frame
        if (found_pos.size() * 2 <= (size_t)nb) {
            for (int k : found_pos) ridx.push_back(cur_idx[k]);
            if ((rc = gather(ctx->fb_frames2, ridx, &rsub))) break;
            rb = &rsub;
        } else {
            ridx = cur_idx;
        }
        const int nr = (int)ridx.size();
        for (int k = 0; k < nr; ++k) {
            const int f = ridx[k];
            const bool is_new = h_found_level[f] == L;
            h_np[k] = is_new ? N : 0;
            if (is_new) {
                memset(h_lv.data() + (size_t)k * N, L, (size_t)N);
                memcpy(h_pts.data() + (size_t)k * N * 2, h_boards + (size_t)f * N * 2, sizeof(double) * 2 * N);
            }
        }
        if (hipMemcpy(d_pts.p, h_pts.data(), (size_t)nr * N * 16, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_lv.p, h_lv.data(), (size_t)nr * N, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_np.p, h_np.data(), (size_t)nr * 4, hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "board upload failed");
            break;
        }
        for (int l = L - 1; l >= 0 && !rc; --l)  // (refining past "nothing refined" is a no-op, mrgingham.cc:97-98)
            rc = mrgingham_amd_refine_batch(ctx, rb, l, (double*)d_pts.p, (signed char*)d_lv.p, (const int32_t*)d_np.p,
                                            N, nullptr);
        if (!rc) rc = mrgingham_amd_sync(ctx);
        if (rc == MRGINGHAM_AMD_ERR_CAPACITY) {
            // a frame of the refine batch overflowed the default tables at some level: refine the boards
            // found at this level one frame at a time (that path retries with one entry per pixel)
            rc = 0;
            for (int k = 0; k < nr && !rc; ++k)  // (h_boards still holds the unrefined grids)
                if (h_np[k]) rc = refine_frame_alone(ctx, *rb, k, h_boards + (size_t)ridx[k] * N * 2, h_levels, ridx[k], N, L);
            if (rc) break;
            lap("refine 1-by-1", L, nr);
            continue;
        }
        if (rc) break;
        if (hipMemcpy(h_pts.data(), d_pts.p, (size_t)nr * N * 16, hipMemcpyDeviceToHost) != hipSuccess ||
            (h_levels && hipMemcpy(h_lv.data(), d_lv.p, (size_t)nr * N, hipMemcpyDeviceToHost) != hipSuccess)) {
            rc = fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "board download failed");
            break;
        }
        for (int k = 0; k < nr; ++k)
            if (h_np[k]) {
                memcpy(h_boards + (size_t)ridx[k] * N * 2, h_pts.data() + (size_t)k * N * 2, sizeof(double) * 2 * N);
                if (h_levels) memcpy(h_levels + (size_t)ridx[k] * N, h_lv.data() + (size_t)k * N, (size_t)N);
            }
        lap("refine+D2H", L, nr);
    }
    return rc;
}

/* ------------------------------------------------------------------------ */
/* The full detector over a batch, pipelined                                 */
/* ------------------------------------------------------------------------ */
// What mrgingham::find_chessboard_from_image_array does per frame (mrgingham.cc:106-140) is a chain of dependent
// steps that alternate between device and host: candidates at level 3 -> grid finder -> (none: level 2 -> grid
// finder ...) -> refinement of the found board level by level.  One batch at a time that leaves the device idle
// while the host threads run the grid finder and the host idle during the device passes (round 3: 3.8 ms per 64
// frames of 4096x3072 against 0.98 ms for the chain).  Here a batch is a JOB in three parts:
//   A  (device, queued by submit)  all level images in one pass over the frames, the responses + candidates of
//      levels 3, 2 AND 1 in one grid (levels 2 and 1 speculatively: together a third of a level-0 pass; 12 MP boards
//      are found at level 2, and the one frame in fifty that needs level 1 would otherwise hold up its whole batch),
//      candidates to pinned host memory;
//   H  (host, run inside the NEXT submit or by collect)  grid finder per frame, level 3 first, then 2, then 1
//      (mrgingham.cc:127-138) on the context's host threads -- started before that submit queues its own part A,
//      joined after it; the boards that were found go back to the device;
//   B  (device, queued by H on the job's component stream)  refinement of the found boards down to level 0
//      (mrgingham.cc:81-99) with the sparse schedule -- response only in the cells around the corners, frames it
//      cannot take repeated densely on the device (queue_sparse_levels) --, boards to pinned host memory.
// A job owns one scratch set from A to the end of B (B reads A's level images; its level sizes stay with that set, so
// jobs of different frame sizes can be in flight), so up to `scratch sets` jobs are in flight; submit completes the job
// that still holds the set it is about to take.  Frames without a board at levels 3-1 (no board in view, or one that
// only shows at full resolution) finish through the synchronous level search above on the single-frame context of the
// same device, which leaves the jobs in flight alone.  Results are the synchronous dense schedule's, double for double.

static int fb_complete(mrgingham_amd_ctx* ctx, mrgingham_amd_ctx::BoardsJob& job);
// Results of jobs that were completed before anybody collected them wait in done_tickets.  A caller that never collects
// (it may: the outputs are complete by then) must not make the list grow for ever: beyond 1024 entries the oldest go, and
// a _collect of such a ticket reports "no such ticket".
static void fb_remember(mrgingham_amd_ctx* ctx, int ticket, int status) {
    ctx->done_tickets.emplace_back(ticket, status);
    if (ctx->done_tickets.size() > 1024) ctx->done_tickets.erase(ctx->done_tickets.begin(), ctx->done_tickets.begin() + 512);
}
// phase clock of the find_boards calls (a dozen clock reads per batch; mrgingham_amd_find_boards_stats)
#define FB_LAP(i) do { const double t_ = fb_now(); ctx->fb_prof[i] += t_ - fb_t; fb_t = t_; } while (0)
#define FB_T0 double fb_t = fb_now()

static size_t fb_align(size_t v) { return (v + 255) & ~(size_t)255; }
struct FbPinned { int32_t *cnt, *xy; double* pts; signed char* lv; int32_t *np, *st; size_t bytes; };
static FbPinned fb_layout(void* base, int nlev, int B, int cap, int N) {
    FbPinned L;
    size_t o = 0;
    char* b = (char*)base;
    L.cnt = (int32_t*)(b + o); o += fb_align((size_t)nlev * B * 4);
    L.xy = (int32_t*)(b + o); o += fb_align((size_t)nlev * B * cap * 8);
    L.pts = (double*)(b + o); o += fb_align((size_t)B * N * 16);
    L.lv = (signed char*)(b + o); o += fb_align((size_t)B * N);
    L.np = (int32_t*)(b + o); o += fb_align((size_t)B * 4);
    L.st = (int32_t*)(b + o); o += fb_align((size_t)(kMaxLevel + 1) * B * 4);  // status words of the refinement, [level][frame]
    L.bytes = o;
    return L;
}

// part H, first half: waits for part A, deals with the frames whose candidate lists did not fit, and STARTS the grid
// finder (mrgingham.cc:51) on the context's host threads -- level by level per frame.  The caller may do something
// else before fb_host_end (submit queues the next batch's device passes there).
static void fb_grid_worker(mrgingham_amd_ctx::BoardsJob* job) {
    const int B = job->fr.nframes, N = job->gridn * job->gridn, cap = job->cap, nlev = job->nlev;
    const FbPinned pin = fb_layout(job->pin.p, nlev, B, cap, N);
    GridScratch scratch;
    const CanonicalRings rings(job->grid_device);
    // (with the device finder: its statuses and indices, [level][frame] like the counts)
    const int32_t* const dev_st = job->grid_device ? (const int32_t*)job->pin_grid.p : nullptr;
    const int32_t* const dev_idx = dev_st ? dev_st + fb_align((size_t)nlev * B * 4) / 4 : nullptr;
    const GridPhaseClock c0 = g_grid_clock;
    struct Leave {   // this thread's share of the batch's grid-finder time into the context's totals
        mrgingham_amd_ctx* ctx; GridPhaseClock c0;
        long long fallbacks = 0;
        ~Leave() {
            if (!ctx) return;
            const GridPhaseClock& c = g_grid_clock;
            std::lock_guard<std::mutex> lk(ctx->fb_stat_mu);
            ctx->fb_grid_fallbacks += fallbacks;
            ctx->fb_grid.graph_t += c.graph_t - c0.graph_t; ctx->fb_grid.adjacency_t += c.adjacency_t - c0.adjacency_t;
            ctx->fb_grid.sequences_t += c.sequences_t - c0.sequences_t; ctx->fb_grid.cycles_t += c.cycles_t - c0.cycles_t;
            ctx->fb_grid.calls += c.calls - c0.calls; ctx->fb_grid.found += c.found - c0.found;
        }
    } leave{job->owner, c0};
    for (int k; (k = job->next.fetch_add(1)) < B;) {
        for (int li = 0; li < nlev; ++li) {
            const int n = pin.cnt[(size_t)li * B + k];
            if (n < N) continue;
            const std::vector<int32_t>& bg = job->big[(size_t)li * B + k];
            const int32_t* src = bg.empty() ? pin.xy + ((size_t)li * B + k) * cap * 2 : bg.data();
            bool found;
            const int st = dev_st && bg.empty() ? dev_st[(size_t)li * B + k] : -1;
            if (st == 1) {  // the device's board: its candidates by index, scaled as find_grid.cc:353-354 scales them
                const int32_t* idx = dev_idx + ((size_t)li * B + k) * N;
                double* out = job->h_boards + (size_t)k * N * 2;
                for (int i = 0; i < N; ++i) {
                    out[2 * i] = (double)src[2 * idx[i]] / 1000.0;
                    out[2 * i + 1] = (double)src[2 * idx[i] + 1] / 1000.0;
                }
                found = true;
            } else if (st == 0) {
                found = false;
            } else {  // the host finder: no device finder, a list detected again at full capacity, or one the device declined
                leave.fallbacks += dev_st && bg.empty();
                found = grid_of_candidates(src, n, job->gridn, job->h_boards + (size_t)k * N * 2, &scratch);
            }
            if (found) {
                job->h_found[k] = (signed char)job->levs[li];
                if (job->h_levels) memset(job->h_levels + (size_t)k * N, job->levs[li], (size_t)N);
                break;
            }
        }
    }
}
static int fb_host_begin(mrgingham_amd_ctx* ctx, mrgingham_amd_ctx::BoardsJob& job) {
    const int B = job.fr.nframes, N = job.gridn * job.gridn, cap = job.cap, nlev = job.nlev;
    const mrgingham_amd_frames* fr = &job.fr;
    job.state = 2;
    job.refine_queued = false;
    job.grid_running = false;
    MRG_HIP_CHECK(hipEventSynchronize(job.ev_a));
    add_elapsed_ms(ctx->fb_dev_ms[0], job.ev_a0, job.ev_a);
    const FbPinned pin = fb_layout(job.pin.p, nlev, B, cap, N);
    int rc = 0;
    // Frames whose candidates did not fit: again at full capacity (detect_full_capacity); the tables of the level grow
    // for the batches to come.
    job.big.assign((size_t)nlev * B, std::vector<int32_t>());
    bool overflowed = false;
    for (int li = 0; li < nlev && !rc; ++li)
        for (int k = 0; k < B && !rc; ++k) {
            int32_t& c = pin.cnt[(size_t)li * B + k];
            if (c >= 0 && c <= cap) continue;
            overflowed |= c < 0;
            rc = detect_full_capacity(ctx, *fr, k, job.levs[li], k, job.big[(size_t)li * B + k], &c);
        }
    if (rc) return rc;
    if (overflowed)
        for (int li = 0; li < nlev; ++li) {
            int grew = 0;
            harvest_status(ctx, job.set, job.levs[li], &grew, true);
        }
    const int nthreads = host_threads(job.nthreads);
    job.next.store(0);
    job.nworkers = (nthreads < B ? nthreads : B) - 1;  // + the calling thread, in fb_host_end
    job.owner = ctx;
    ctx->fb_threads_used = job.nworkers + 1;
    mrgingham_amd_ctx::BoardsJob* jp = &job;
    if (job.nworkers > 0) {
        ctx->pool.start(job.nworkers, [jp] { fb_grid_worker(jp); });
        job.grid_running = true;
    }
    return 0;
}

// part H, second half: joins the grid finder and queues part B -- the boards found above level 0, refined level by level
// (mrgingham.cc:81-99) on the job's component stream.
static int fb_host_end(mrgingham_amd_ctx* ctx, mrgingham_amd_ctx::BoardsJob& job) {
    const int B = job.fr.nframes, N = job.gridn * job.gridn, cap = job.cap, nlev = job.nlev;
    const mrgingham_amd_frames* fr = &job.fr;
    FB_T0;
    fb_grid_worker(&job);
    if (job.grid_running) {
        ctx->pool.wait();
        job.grid_running = false;
    }
    FB_LAP(3);
    const FbPinned pin = fb_layout(job.pin.p, nlev, B, cap, N);
    int rc = 0;
    int top = 0, nref = 0;
    for (int k = 0; k < B && job.do_refine; ++k) {
        const int L = job.h_found[k];
        pin.np[k] = L >= 1 ? N : 0;
        if (L < 1) continue;
        ++nref;
        top = L > top ? L : top;
        memset(pin.lv + (size_t)k * N, L, (size_t)N);
        memcpy(pin.pts + (size_t)k * N * 2, job.h_boards + (size_t)k * N * 2, sizeof(double) * 2 * N);
    }
    if (nref > 0) {
        const int saved = ctx->cur;
        ctx->cur = job.set;  // (the helpers below address the current set)
        hipStream_t cc = cur_cc(ctx);
        const size_t pb = (size_t)B * N * 16, lb = (size_t)B * N;
        // boards | levels | point counts: one block on both sides
        char* const d_pts = (char*)job.d_pts.p;
        char* const d_lv = d_pts + fb_align(pb);
        char* const d_np = d_lv + fb_align(lb);
        char* const d_pts0 = (char*)job.d_pts0.p;
        const bool sparse = sparse_applies(ctx, top, (long long)fr->width * fr->height * B);  // (top >= 1: nref > 0)
        hipEventRecord(job.ev_b0, cc);
        hipError_t e = hipMemcpyAsync(d_pts, pin.pts, fb_align(pb) + fb_align(lb) + (size_t)B * 4, hipMemcpyHostToDevice, cc);
        if (e == hipSuccess && sparse)  // (only the dense repeat of a sparse refinement goes back to them)
            e = hipMemcpyAsync(d_pts0, d_pts, fb_align(pb) + lb, hipMemcpyDeviceToDevice, cc);
        if (e == hipSuccess) {
            const RefineIO io = refine_io_of(ctx, job.set, (double*)d_pts, (signed char*)d_lv, (const int32_t*)d_np, N, nullptr);
            const SparseRestore src{nullptr, 0, 0, (const double*)d_pts0, (const signed char*)(d_pts0 + fb_align(pb))};
            rc = queue_sparse_levels(ctx, fr, top, io, src, !sparse);
            job.top = top;
            e = hipMemcpyAsync(pin.pts, d_pts, job.h_levels ? fb_align(pb) + lb : pb, hipMemcpyDeviceToHost, cc);
            for (int L = 0; L < top && e == hipSuccess; ++L)  // (a frame whose tables overflowed at a level was not refined there)
                e = hipMemcpyAsync(pin.st + (size_t)L * B, status_of(ctx, L), (size_t)B * 4, hipMemcpyDeviceToHost, cc);
            if (e == hipSuccess) e = hipEventRecord(job.ev_b, cc);
            end_op(ctx);
            job.refine_queued = true;
        }
        ctx->cur = saved;
        if (e != hipSuccess) return fail_hip(ctx, e, "find_boards refinement", __FILE__, __LINE__);
        if (rc) return rc;
    }
    FB_LAP(4);
    return 0;
}

// the rest of a job: wait for part B, boards into the caller's array, then the frames still open (level_arg < 0 only)
static int fb_finish(mrgingham_amd_ctx* ctx, mrgingham_amd_ctx::BoardsJob& job) {
    const int B = job.fr.nframes, N = job.gridn * job.gridn;
    int rc = 0;
    FB_T0;
    if (job.refine_queued) {
        MRG_HIP_CHECK(hipEventSynchronize(job.ev_b));
        FB_LAP(5);
        add_elapsed_ms(ctx->fb_dev_ms[1], job.ev_b0, job.ev_b);
        const FbPinned pin = fb_layout(job.pin.p, job.nlev, B, job.cap, N);
        bool overflowed = false;
        for (int k = 0; k < B && !rc; ++k) {
            const int Lf = job.h_found[k];
            if (Lf < 1) continue;
            int bad = 0;
            for (int L = 0; L < Lf; ++L) bad |= pin.st[(size_t)L * B + k] & (kStatusHotOverflow | kStatusCandOverflow);
            if (!bad) {
                memcpy(job.h_boards + (size_t)k * N * 2, pin.pts + (size_t)k * N * 2, sizeof(double) * 2 * N);
                if (job.h_levels) memcpy(job.h_levels + (size_t)k * N, pin.lv + (size_t)k * N, (size_t)N);
                continue;
            }
            // The component tables of a level overflowed for this frame (dense texture): it was not refined there.  Its
            // board -- still the grid finder's in h_boards -- is refined on the single-frame context, which retries with
            // a table entry per pixel; the tables of this context grow for the batches to come.
            overflowed = true;
            rc = refine_frame_alone(ctx, job.fr, k, job.h_boards + (size_t)k * N * 2, job.h_levels, k, N, Lf);
        }
        if (overflowed)
            for (int L = 0; L < job.top; ++L) {
                int grew = 0;
                harvest_status(ctx, job.set, L, &grew, true);
            }
        job.refine_queued = false;
        FB_LAP(6);
    }
    const int lowest = job.levs[job.nlev - 1];
    std::vector<int> open;
    if (job.level_arg < 0 && lowest > 0)
        for (int k = 0; k < B; ++k)
            if (job.h_found[k] < 0) open.push_back(k);
    job.state = 0;  // the set is this job's no longer
    if (!open.empty()) {
        // what is left (no board in view, or one that only shows at full resolution): level by level, synchronously, on
        // the single-frame context of this device -- its own streams and scratch, so the jobs in flight here stay so
        mrgingham_amd_ctx* one = same_device_ctx(ctx);
        if (!one) return MRGINGHAM_AMD_ERR_DEVICE;
        rc = find_boards_sync_levels(one, &job.fr, job.gridn, lowest - 1, 0, job.h_boards, job.h_found, job.nthreads, open,
                                     job.do_refine, job.h_levels, job.grid_device);
        if (rc) ctx->err = one->err;
    }
    return rc;
}

static int fb_abandon(mrgingham_amd_ctx* ctx, mrgingham_amd_ctx::BoardsJob& job, int rc) {
    if (job.grid_running) ctx->pool.wait();
    job.grid_running = false;
    hipStreamSynchronize(ctx->ccs[job.set]);  // nothing of this job may stay queued behind an error
    job.state = 0;
    job.refine_queued = false;
    return rc;
}
static int fb_complete(mrgingham_amd_ctx* ctx, mrgingham_amd_ctx::BoardsJob& job) {
    int rc = 0;
    if (job.state == 1) {
        rc = fb_host_begin(ctx, job);
        if (!rc) rc = fb_host_end(ctx, job);
    }
    if (rc) return fb_abandon(ctx, job, rc);
    return fb_finish(ctx, job);
}

// find_boards_submit / _collect jobs in flight hold scratch sets between their device passes: every other call that
// rotates through the sets or resizes them completes those jobs first (their results stay collectable)
void fb_drain(mrgingham_amd_ctx* ctx) {
    for (auto& j : ctx->jobs)
        if (j.state != 0) {
            const int ticket = j.ticket;
            fb_remember(ctx, ticket, fb_complete(ctx, j));
        }
}

// (the public entry + what the single-image wrappers need on top of it: no refinement, the corners' refinement levels)
static int fb_submit(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int gridn, int image_pyramid_level,
                     double* h_boards, signed char* h_found_level, int nthreads, bool do_refine, signed char* h_levels) {
    int rc = validate_frames(ctx, fr);
    if (rc) return rc;
    if (gridn < 2 || image_pyramid_level > kMaxLevel || !h_boards || !h_found_level)
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad gridn / level / NULL outputs");
    const int B = fr->nframes, N = gridn * gridn;
    const int ticket = ctx->next_ticket++ & 0x3fffffff;
    FB_T0;
    for (int f = 0; f < B; ++f) h_found_level[f] = -1;
    if (B == 0) {
        fb_remember(ctx, ticket, 0);
        return ticket;
    }
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    if (!ctx->fb_pipeline) {  // option "find_boards_pipeline" 0: the synchronous dense schedule, at once
        fb_drain(ctx);
        const int first = image_pyramid_level >= 0 ? image_pyramid_level : 3;
        const int last = image_pyramid_level >= 0 ? image_pyramid_level : 0;
        std::vector<int> open(B);
        for (int f = 0; f < B; ++f) open[f] = f;
        fb_remember(ctx, ticket, find_boards_sync_levels(ctx, fr, gridn, first, last, h_boards, h_found_level, nthreads, open,
                                                               do_refine, h_levels,
                                                               ctx->fb_grid_device && !g_grid_debug && !g_grid_debug_sequence.on));
        return ticket;
    }
    // levels searched in the first pass: the one asked for, or 3, 2 and 1 (levels 2 and 1 speculatively: together they
    // cost the device a third of a level-0 pass, 12 MP boards are found at level 2, and the one frame in fifty that
    // needs level 1 would otherwise hold up its whole batch); level 0 only for what is still open after them
    const int top = image_pyramid_level >= 0 ? image_pyramid_level : 3;
    const int nlev = image_pyramid_level >= 0 ? 1 : 3;
    const int cap = 4 * N + 64;  // candidates kept per frame for the grid finder
    // option "find_boards_grid": the lists of this pass are ordered on the device, behind their detection (not while the
    // calling thread has the reference's debug dumps or its sequence trace on: those are the host finder's)
    const bool grid_device = ctx->fb_grid_device && gridn <= kGfMaxGridn && !g_grid_debug && !g_grid_debug_sequence.on;
    // the refinement takes the sparse schedule where it pays: such a context keeps three scratch sets (choose_sets)
    if (sparse_possible(ctx, top)) ctx->sparse_seen = true;
    {   // a change of the rotation (another batch shape) synchronises and may free a set: no job may be in flight then
        const double per_set = 5.0 * (double)B * fr->width * fr->height;
        const double mx = per_set > ctx->max_set_bytes ? per_set : ctx->max_set_bytes;
        const int want = ctx->nsets_fixed ? ctx->nsets : (3.0 * mx <= (ctx->sparse_seen ? 16e9 : 8e9) ? 3 : 2);
        if (want != ctx->nsets) fb_drain(ctx);
    }
    if ((rc = choose_sets(ctx, fr))) return rc;
    // the set this job is going to take may still belong to an earlier one: that one is completed first
    {
        auto& occupant = ctx->jobs[(ctx->cur + 1) % ctx->nsets];
        if (occupant.state != 0) fb_remember(ctx, occupant.ticket, fb_complete(ctx, occupant));
    }
    // Level scratch of THAT set alone (the other sets belong to jobs in flight, possibly of another frame size: a stream
    // of mixed resolutions keeps every job's level sizes with its own set).  Buffers only ever grow; a buffer that has
    // to grow synchronises the device first, which the jobs in flight survive.
    {
        const int target = (ctx->cur + 1) % ctx->nsets;
        for (int L = 0; L <= top; ++L)
            if ((rc = ensure_level_set(ctx, target, L, B, fr->width, fr->height, N))) return rc;
    }
    if ((rc = ensure_points(ctx, B, N))) return rc;
    if (!ctx->sparse_stat.p) {
        if ((rc = ensure(ctx, ctx->sparse_stat, 256))) return rc;
        MRG_HIP_CHECK(hipMemset(ctx->sparse_stat.p, 0, 256));
    }
    {   // everything the job allocates BEFORE the scratch rotation moves (begin_op): an allocation that fails returns with
        // the context as it was -- no set taken, nothing queued -- and the call can simply be made again
        auto& nj = ctx->jobs[(ctx->cur + 1) % ctx->nsets];
        if ((rc = ensure(ctx, nj.d_cnt, fb_align((size_t)nlev * B * 4) + (size_t)nlev * B * cap * 8)) ||
            (rc = ensure(ctx, nj.d_pts, fb_align((size_t)B * N * 16) + fb_align((size_t)B * N) + (size_t)B * 4)) ||
            (rc = ensure(ctx, nj.d_pts0, fb_align((size_t)B * N * 16) + (size_t)B * N)))
            return rc;
        if ((rc = ensure_pinned(ctx, nj.pin, fb_layout(nullptr, nlev, B, cap, N).bytes, 4, false))) return rc;
        if (grid_device) {  // statuses | indices of the device finder, one block on both sides
            const size_t gb = fb_align((size_t)nlev * B * 4) + (size_t)nlev * B * N * 4;
            if ((rc = ensure(ctx, nj.d_grid, gb)) || (rc = ensure_pinned(ctx, nj.pin_grid, gb, 4, false)) ||
                (rc = ensure_find_grids(ctx, (ctx->cur + 1) % ctx->nsets, nlev * B)))
                return rc;
        }
        for (Event* e : {&nj.ev_a, &nj.ev_b, &nj.ev_a0, &nj.ev_b0}) MRG_HIP_CHECK(e->create(hipEventDefault));
    }
    begin_op(ctx, top);
    auto& job = ctx->jobs[ctx->cur];
    job.set = ctx->cur;
    job.ticket = ticket;
    job.fr = *fr;
    job.gridn = gridn;
    job.level_arg = image_pyramid_level;
    job.nthreads = nthreads;
    job.nlev = nlev;
    for (int li = 0; li < 3; ++li) job.levs[li] = top - li;
    job.cap = cap;
    job.h_boards = h_boards;
    job.h_found = h_found_level;
    job.h_levels = h_levels;
    job.do_refine = do_refine;
    job.refine_queued = false;
    job.grid_device = grid_device;
    // The host part of the job before this one runs inside this call: its grid-finder threads are started first when
    // its candidates have already arrived (the steady state), so that they work while this thread queues the device
    // passes below; otherwise after them.
    mrgingham_amd_ctx::BoardsJob* prev = nullptr;
    for (auto& other : ctx->jobs)
        if (&other != &job && other.state == 1) prev = &other;
    bool prev_begun = false;
    FB_LAP(0);
    if (prev && hipEventQuery(prev->ev_a) == hipSuccess) {
        const int r = fb_host_begin(ctx, *prev);
        if (r) {
            fb_remember(ctx, prev->ticket, fb_abandon(ctx, *prev, r));
            prev = nullptr;
        }
        prev_begun = true;
    }
    FB_LAP(1);
    order_after_previous(ctx, {}, {});
    hipEventRecord(job.ev_a0, ctx->pix);
    // part A: level images of every level up to the top in one pass (the refinement's variance windows and cells read
    // them too), the responses of the levels searched, their candidates
    queue_level_images(ctx, fr, top, true);
    const int lowest = job.levs[job.nlev - 1];
    LevelBatch by_level[kMaxLevel + 1], lbs[3];
    hipEvent_t lev_ev[kMaxLevel + 1] = {};
    queue_chess_levels(ctx, fr, top, lowest, false, by_level, lev_ev, nullptr);  // (no kernel timing around these)
    for (int li = 0; li < job.nlev; ++li) lbs[li] = by_level[job.levs[li]];
    hipStream_t cc = cur_cc(ctx);
    hipError_t e = hipStreamWaitEvent(cc, lev_ev[lowest], 0);  // the last of them on the pixel stream
    {   // the candidates of every level searched in this pass: one grid per kernel, not one per level
        CompTables dts[3];
        DetectOut douts[3];
        for (int li = 0; li < job.nlev; ++li) {
            dts[li] = tables_of(ctx, job.levs[li]);
            douts[li] = DetectOut{(int32_t*)((char*)job.d_cnt.p + fb_align((size_t)job.nlev * B * 4)) + (size_t)li * B * cap * 2, cap,
                                  (int32_t*)job.d_cnt.p + (size_t)li * B};
        }
        launch_cc_detect_levels(lbs, dts, job.levs, douts, job.nlev, B, cc);
    }
    int grid_rc = 0;
    if (grid_device) {  // every list of the pass -- [level][frame], as the counts lie -- in one launch right behind it
        int32_t* const d_st = (int32_t*)job.d_grid.p;
        grid_rc = launch_find_grids(ctx, job.set, (const int32_t*)((char*)job.d_cnt.p + fb_align((size_t)job.nlev * B * 4)), (const int32_t*)job.d_cnt.p,
                                    job.nlev * B, cap, gridn, d_st + fb_align((size_t)job.nlev * B * 4) / 4, d_st, cc);
    }
    const FbPinned pin = fb_layout(job.pin.p, job.nlev, B, cap, N);
    if (e == hipSuccess)  // counts | candidates: one block on both sides
        e = hipMemcpyAsync(pin.cnt, job.d_cnt.p, fb_align((size_t)job.nlev * B * 4) + (size_t)job.nlev * B * cap * 8, hipMemcpyDeviceToHost, cc);
    if (e == hipSuccess && grid_device)
        e = hipMemcpyAsync(job.pin_grid.p, job.d_grid.p, fb_align((size_t)job.nlev * B * 4) + (size_t)job.nlev * B * N * 4, hipMemcpyDeviceToHost, cc);
    if (e == hipSuccess) e = hipEventRecord(job.ev_a, cc);
    end_op(ctx);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && !grid_rc) job.state = 1;
    FB_LAP(2);
    ++ctx->fb_prof_n;
    // ... and while the device works on that: the (rest of the) host part of the job before this one
    if (prev) {
        int r = prev_begun ? 0 : fb_host_begin(ctx, *prev);
        if (!r) r = fb_host_end(ctx, *prev);
        if (r) fb_remember(ctx, prev->ticket, fb_abandon(ctx, *prev, r));
    }
    if (e != hipSuccess) return fail_hip(ctx, e, "find_boards first pass", __FILE__, __LINE__);
    if (grid_rc) return grid_rc;
    return ticket;
}

// mrgingham::find_chessboard_from_image_array (mrgingham.cc:38-140) on ONE frame that already lives
// on the device (dense, stride == width): detector and refinement on the GPU, grid finder on the
// host.  Returns the level the grid was found at, or -1.  `lv` receives the per-corner refinement
// level; without do_refine nothing is refined and every entry is the found level.
// Every caller has rejected levels above kMaxLevel already, and its per-thread context keeps the pipeline on (no entry
// point exposes one): so the pipelined detector below serves every search but the reference's `debug` one, whose dumps
// (write_debug_dumps, the grid finder's vnlogs) need the level-by-level schedule after it.
int find_board_on_device(mrgingham_amd_ctx* ctx, const char* who, const mrgingham_amd_frames* fr, int gridn,
                         int image_pyramid_level, bool do_refine, std::vector<PointD>& board, std::vector<signed char>& lv,
                         bool debug, const char* debug_image_filename) {
    const int Nrows = fr->height, Ncols = fr->width;
    const int N = gridn * gridn;
    if (!debug) {
        // one frame through the pipelined batch detector (find_boards_submit / _collect above): the candidates of levels
        // 3, 2 and 1 in ONE device pass instead of a round trip per level, the refinement of every level in one more --
        // same boards (the pipelined detector equals the level-by-level schedule frame for frame, tests/test_gpu_board.py)
        board.assign((size_t)N, PointD{0., 0.});
        lv.assign((size_t)N, 0);
        signed char found_level = -1;
        const int ticket = fb_submit(ctx, fr, gridn, image_pyramid_level, &board[0].x, &found_level, 1, do_refine, lv.data());
        if (ticket < 0 || mrgingham_amd_find_boards_collect(ctx, ticket) != 0) return -1;
        return found_level;
    }
    std::vector<int32_t> xy;
    bool found = false;
    board.assign((size_t)N, PointD{0., 0.});
    // image_pyramid_level >= 0: that level only; < 0: 3, 2, 1, 0 until a grid is found (mrgingham.cc:116-139)
    const int first = image_pyramid_level >= 0 ? image_pyramid_level : 3;
    const int last = image_pyramid_level >= 0 ? image_pyramid_level : 0;
    int level = first;
    for (; level >= last && !found; --level) {
        if (!check_level_and_layout(who, Nrows, Ncols, fr->stride, level)) continue;
        int32_t count = 0;
        const bool ok = detect_one_frame_all(ctx, fr, level, xy, &count, debug, debug_image_filename);
        if (!ok || count < N) continue;
        g_grid_debug = debug;  // the reference hands its debug flag to the grid finder as well (mrgingham.cc:50-52)
        found = grid_of_candidates(xy.data(), count, gridn, &board[0].x);
        g_grid_debug = false;
        if (found) break;
    }
    if (!found) return -1;
    lv.assign((size_t)N, (signed char)level);
    if (do_refine) refine_board_alone(ctx, fr, &board[0].x, lv.data(), N, level, debug, debug_image_filename);
    return level;
}

}  // namespace mrg

using namespace mrg;

extern "C" {

int mrgingham_amd_find_boards_submit(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int gridn,
                                     int image_pyramid_level, double* h_boards, signed char* h_found_level, int nthreads) {
    return fb_submit(ctx, fr, gridn, image_pyramid_level, h_boards, h_found_level, nthreads, true, nullptr);
}

int mrgingham_amd_find_boards_submit_ex(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int gridn,
                                        int image_pyramid_level, int do_refine, double* h_boards, signed char* h_levels,
                                        signed char* h_found_level, int nthreads) {
    return fb_submit(ctx, fr, gridn, image_pyramid_level, h_boards, h_found_level, nthreads, do_refine != 0, h_levels);
}

int mrgingham_amd_find_boards_collect(mrgingham_amd_ctx* ctx, int ticket) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    for (auto& j : ctx->jobs)
        if (j.state != 0 && j.ticket == ticket) return fb_complete(ctx, j);
    for (size_t i = 0; i < ctx->done_tickets.size(); ++i)
        if (ctx->done_tickets[i].first == ticket) {
            const int rc = ctx->done_tickets[i].second;
            ctx->done_tickets.erase(ctx->done_tickets.begin() + (long)i);
            return rc;
        }
    return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "find_boards_collect: no such ticket (%d)", ticket);
}

int mrgingham_amd_find_boards_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int gridn,
                                    int image_pyramid_level, double* h_boards, signed char* h_found_level,
                                    int nthreads) {
    const int ticket = mrgingham_amd_find_boards_submit(ctx, fr, gridn, image_pyramid_level, h_boards, h_found_level, nthreads);
    if (ticket < 0) return ticket;
    return mrgingham_amd_find_boards_collect(ctx, ticket);
}


int mrgingham_amd_find_boards_stats(mrgingham_amd_ctx* ctx, double* out, int n, int reset) {
    if (!ctx || !out || n < 0) return MRGINGHAM_AMD_ERR_ARG;
    fb_drain(ctx);
    double v[MRGINGHAM_AMD_FB_STATS] = {};
    const double tick = grid_clock_tick_us();  // (may wait 0.2 ms when the process has only just started: not under the lock)
    {
        std::lock_guard<std::mutex> lk(ctx->fb_stat_mu);
        v[0] = (double)ctx->fb_prof_n;
        v[1] = (double)ctx->fb_threads_used;
        for (int i = 0; i < 7; ++i) v[2 + i] = ctx->fb_prof[i];
        v[9] = (double)ctx->fb_grid.calls; v[10] = (double)ctx->fb_grid.found;
        v[11] = ctx->fb_grid.graph_t * tick; v[12] = ctx->fb_grid.adjacency_t * tick; v[13] = ctx->fb_grid.sequences_t * tick;
        v[14] = ctx->fb_grid.cycles_t * tick;
        v[15] = ctx->fb_dev_ms[0]; v[16] = ctx->fb_dev_ms[1];
        if (reset) {
            for (double& x : ctx->fb_prof) x = 0;
            ctx->fb_prof_n = 0;
            ctx->fb_grid = GridPhaseClock{0, 0, 0, 0, 0, 0};
            ctx->fb_dev_ms[0] = ctx->fb_dev_ms[1] = 0;
        }
    }
    for (int i = 0; i < n && i < MRGINGHAM_AMD_FB_STATS; ++i) out[i] = v[i];
    return MRGINGHAM_AMD_FB_STATS;
}

int mrgingham_amd_grid_clock(double* out6, int reset) {
    if (!out6) return MRGINGHAM_AMD_ERR_ARG;
    GridPhaseClock& c = g_grid_clock;
    const double tick = grid_clock_tick_us();
    out6[0] = (double)c.calls; out6[1] = (double)c.found; out6[2] = c.graph_t * tick; out6[3] = c.adjacency_t * tick;
    out6[4] = c.sequences_t * tick; out6[5] = c.cycles_t * tick;
    if (reset) c = GridPhaseClock{0, 0, 0, 0, 0, 0};
    return 0;
}

}  // extern "C"
