// The context of libmrgingham_amd.so and the helpers that more than one of its host files calls.  Internal: not
// installed, not part of include/.  The host side is cut by concern: api.hip (context lifetime, options, scratch sets,
// status words, the pixel-only _batch entry points), chain.hip (the detector's stream scheduling: detect / refine /
// chain calls, kernel timing, the sparse schedule), multi.hip (several devices), reference.hip (the reference's own C
// symbols over one frame), boards.hip (find_boards: the level search, synchronous and pipelined), blobs_api.hip (the
// blob detector and the circle-grid finder over a batch), loader.hip (what the file-list loaders share).
#pragma once
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mrgingham_amd.h"
#include "common.h"
#include "grid.h"
#include "image_io.h"
#include "kernels.h"
#include "unpack_rows.h"

namespace mrg {

constexpr int kMaxLevel = 10;  // find_chessboard_corners.cc:433-436

// OWNERS.  What a context holds of the runtime -- device memory, page-locked memory, events, streams -- is a member of one
// of the four types below and is given back by that member's destructor: nothing lists the members a second time.  All
// four are move-only, and the raw handle stays readable (p and bytes; an Event or a Stream converts to its handle).
// device memory, grown on demand (ensure)
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    ~DevBuf() { if (p) (void)hipFree(p); }
};
// page-locked host memory, grown on demand like a DevBuf (ensure_pinned)
struct PinBuf {
    void* p = nullptr;
    size_t bytes = 0;
    PinBuf() = default;
    PinBuf(PinBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    PinBuf& operator=(PinBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    ~PinBuf() { if (p) (void)hipHostFree(p); }
};
struct Event {
    hipEvent_t h = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : h(o.h) { o.h = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Event() { if (h) (void)hipEventDestroy(h); }
    operator hipEvent_t() const { return h; }
    // created with `flags` on first use
    hipError_t create(unsigned flags) { return h ? hipSuccess : hipEventCreateWithFlags(&h, flags); }
};
// (created in place, by whichever of the runtime's calls the owner wants: hipStreamCreateWithPriority(&s.h, ...))
struct Stream {
    hipStream_t h = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : h(o.h) { o.h = nullptr; }
    Stream& operator=(Stream&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Stream() { if (h) (void)hipStreamDestroy(h); }
    operator hipStream_t() const { return h; }
};
static_assert(!std::is_copy_constructible_v<DevBuf> && !std::is_copy_assignable_v<DevBuf>, "DevBuf owns its memory");
static_assert(!std::is_copy_constructible_v<PinBuf> && !std::is_copy_assignable_v<PinBuf>, "PinBuf owns its memory");
static_assert(!std::is_copy_constructible_v<Event> && !std::is_copy_assignable_v<Event>, "Event owns its handle");
static_assert(!std::is_copy_constructible_v<Stream> && !std::is_copy_assignable_v<Stream>, "Stream owns its handle");

// Scratch of one pyramid level: level images, the dense response and the
// component tables.  Levels have their own scratch because the pixel kernels of
// level L-1 run while the component search of level L is still working.
struct LevelScratch {
    int w = 0, h = 0, nframes = 0, cap = 0, cand_cap = 0, sort_cap = 0, pitch = 0, shift = -1;
    long long arena_cap = 0;
    DevBuf img, resp, gidx, hot_xy, parent, comp_cnt, roots, comp_first, comp_box, arena, cand, sortkeys;
    // (for choose_sets, which hands the scratch of a set that leaves the rotation back)
    template <class F>
    void for_each_buffer(F&& f) {
        for (DevBuf* b : {&img, &resp, &gidx, &hot_xy, &parent, &comp_cnt, &roots, &comp_first, &comp_box, &arena, &cand, &sortkeys}) f(*b);
    }
};

// Kernel timing (chain.hip, KERNEL TIMING): every timing event the context has ever created, the pairs recorded since
// mrgingham_amd_chess_kernel_ms last read them, and the events that are in no pair.  The read-out puts every event back
// among the idle ones, so an event that was taken but never got into a pair (an error in between) is not lost.
struct TimingEvents {
    std::vector<Event> all;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pairs;
    std::vector<hipEvent_t> idle;
};

}  // namespace mrg

// Host worker threads of a context (the grid finder of mrgingham_amd_find_boards_batch): started
// once and parked on a condition variable, because spawning threads per call cost more than the
// grid finder itself.
struct HostPool {
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv_start, cv_done;
    std::function<void()> job;
    long generation = 0;
    int wanted = 0, running = 0;
    bool stop = false;

    void loop(int id) {
        long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(m);
            cv_start.wait(lk, [&] { return stop || (generation != seen && id < wanted); });
            if (stop) return;
            seen = generation;
            lk.unlock();
            job();
            lk.lock();
            if (--running == 0) cv_done.notify_all();
        }
    }
    // starts f on n pool threads (the caller is not one of them) and returns; wait() returns when they are done
    void start(int n, const std::function<void()>& f) {
        if (n <= 0) return;
        {
            std::unique_lock<std::mutex> lk(m);
            while ((int)threads.size() < n) {
                const int id = (int)threads.size();
                threads.emplace_back([this, id] { loop(id); });
            }
            job = f;
            wanted = n;
            running = n;
            ++generation;
        }
        cv_start.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return running == 0; });
        wanted = 0;
    }
    // runs f on n threads (the caller is one of them) and returns when all of them are done
    void run(int n, const std::function<void()>& f) {
        if (n <= 1) { f(); return; }
        start(n - 1, f);
        f();
        wait();
    }
    ~HostPool() {
        {
            std::unique_lock<std::mutex> lk(m);
            stop = true;
        }
        cv_start.notify_all();
        for (auto& t : threads) t.join();
    }
};

// body(i) for every i of 0 .. n-1, handed out one at a time to at most nthreads threads of the pool (the caller is one of
// them).  With a State, every thread owns one for the whole run and the body is body(i, state): buffers that are reused
// from file to file.
template <class State = char, class F>
void for_files(HostPool& pool, int nthreads, int n, F&& body) {
    std::atomic<int> next{0};
    pool.run(nthreads < n ? nthreads : n, [&] {
        State state{};
        for (int i; (i = next.fetch_add(1)) < n;) {
            if constexpr (std::is_invocable_v<F&, int>) body(i);
            else body(i, state);
        }
    });
}

constexpr int kMaxSets = 3;  // scratch sets a context can rotate through (option "scratch_sets": 2 or 3)

struct mrgingham_amd_ctx {
    int device = 0;
    int nsets = 2;
    bool nsets_fixed = false;  // option "scratch_sets" given: no automatic choice
    double max_set_bytes = 0;
    // HIP streams of a context: `pix` runs the pixel kernels (pyramid, ChESS) back to back, each
    // over the whole batch; `ccs[set]` run the latency-bound component kernels (a serial chain
    // detect -> refine -> refine ... per call) underneath them, one stream per scratch set so that
    // the chains of consecutive calls overlap each other as well.  Events order cc(L) after pix(L).
    mrg::Stream pix;
    mrg::Stream ccs[kMaxSets];
    // Device buffers the last call of each set wrote / read (caller-owned outputs and inputs):
    // consecutive calls run on different component streams, so a call that touches a buffer the
    // previous call wrote (or writes one it read) must wait for it explicitly.
    struct Span { const char* p; size_t n; };
    std::vector<Span> last_w[kMaxSets], last_r[kMaxSets];
    mrg::Event ev_pix[mrg::kMaxLevel + 1];
    // Level scratch exists `nsets` times (2, or 3 with option "scratch_sets"): call N+1 fills set (N+1) % nsets on
    // the pixel stream while the component streams still work through the calls before it in the other sets.
    // Two sets keep two component chains in flight, which hides them as long as a chain is shorter than two
    // steps of the pixel kernels; small frames (64 x 640x480: chain 430 us, pixel kernels 62 us) and dense boards
    // want three.
    mrg::Event ev_cc_done[kMaxSets];
    mrg::Event ev_ext;  // mrgingham_amd_after_stream
    bool cc_pending[kMaxSets] = {};
    int cur = 0;  // scratch set of the call being queued
    std::string err;
    // hot-pixel / component table capacity = level pixels >> shift entries per frame, shift = min(cap_shift,
    // grown_shift[level]).  The default (1/128: 98 304 hot pixels for a 4096x3072 frame, whose bench frames have
    // ~1.3e3 and whose textured ones ~7e4) keeps the tables at 0.35 B per pixel; a frame that needs more is
    // reported (MRGINGHAM_AMD_ERR_CAPACITY at the sync) and the tables of its level GROW to what it asked for, so
    // the same call succeeds when it is made again.
    int cap_shift = 7;
    int grown_shift[mrg::kMaxLevel + 1];
    bool use_v0 = false;  // reference-shaped ChESS kernel instead of the tuned one
    int sparse_subsets = 2;  // option "sparse_subsets": workgroups per frame of the sparse refinement (1 .. 4; 4 measures like 2)
    int chess_variant_hot = 0;  // the levels of a chain (clamp + hot list): 16 = chess_v16_hot_kernel / chess_v16_multi_kernel, 0 = chess_v1
    int pre_fused = 1;  // option "preprocess_fused": CLAHE blend + 3x3 blur in one kernel where the geometry allows (0: always two kernels, the A/B and test hook)
    int chess_seg = 0, chess16_seg = 0;  // options "chess_seg" / "chess16_seg": rows per workgroup of the response kernels, 0 = automatic
    int chess_variant = 0;  // the response without a hot list: 0 = chess_v16_kernel (chess16.hip) where it pays, 1 = chess_v1 always, 16 = chess_v16 wherever it can run
    // levels 3..1 of a chain in one launch (set_option "multi_level_launch"): +1.5 % chain rate, but the
    // component chains then start later and overlap the level-0 launch more (+5 % on that launch): off
    // chain_batch: 0 = one ChESS launch per level; 1 = levels 3..1 in one launch (default: two kernel
    // boundaries fewer per step, 1.129 -> 1.113 ms per 64 frames of 4096x3072); 2 = levels 0..3 in one
    // launch (measured slower: 1.171 ms)
    int multi_level = 1;
    int last_fused = 0, last_merged = 0;  // mrgingham_amd_chain_info
    // TEST HOOK mrgingham_amd_debug_pixel_stage: what it left for mrgingham_amd_debug_pixel_products.  The hot counters
    // are a host copy ([level][counters_nf]: end_op zeroes the device's); everything else is read out of scratch set
    // `set`, which the next op may overwrite -- begin_op says so (valid = false)
    struct PixelStage {
        bool valid = false;
        int set = 0, nframes = 0, cnf = 0;
        unsigned img_levels = 0, list_levels = 0;  // bit L: the level image / the response, list and map of level L are products
        std::vector<int32_t> hot_cnt;
    } pixel_stage;
    // option "sparse_refine": chain_batch computes the response of the levels BELOW the start level only in the cells
    // around the points it refines there (chain.hip: chain_pixels_sparse, queue_sparse_levels)
    int sparse_refine = 1;     // (default: where it pays)
    bool sparse_seen = false;  // a chain has taken the sparse schedule (choose_sets)
    mrg::DevBuf sparse_stat;   // [0]: frames the sparse schedule reported and the library repeated densely (mrgingham_amd_sparse_fallbacks); STATE: see scratch_fill
    int fuse_pyramid = 1;   // option "fuse_pyramid": chain calls take the level images 1..3 out of the level-0 response kernel
    // component-chain schedule of chain_batch: 0 = every level's component kernels start as soon as
    // that level's response is done; 1 (default) = levels 1 and 0 wait for the level-0 response (they then
    // run underneath the NEXT call's pyramid and small levels instead of underneath this call's level 0:
    // same step time, level-0 launch 668 -> 657 us); 2 = every level waits for the level-0 response
    int cc_schedule = 1;
    int cc_lds = 1;  // component search out of LDS for frames with few hot pixels (option "cc_lds"; bits 1-3: timing ablations)

    // device bytes of this context's scratch (mrgingham_amd_scratch_bytes), kept by ensure and release: atomic, because a
    // shard of mrgingham_amd_chain_multi grows its context's scratch on the submit thread
    std::atomic<long long> scratch_total{0};
    // TEST HOOK "scratch_fill" (DESIGN.md section 3.3): -1 = off; 0 .. 255: every new allocation of context memory -- ensure,
    // ensure_pinned, the ring slots of find_boards_files -- is filled with that byte over its whole allocated size before
    // anyone uses it, so that a kernel which reads scratch nobody has written reads something loud instead of the zero
    // of fresh memory.  From MRGINGHAM_AMD_SCRATCH_FILL when the context is created (so that it reaches the contexts no
    // caller holds), or set_option("scratch_fill").  set_option("scratch_fill_now", byte) fills, once and at rest, every
    // buffer in scratch_bufs / pinned_bufs: the buffers ensure and ensure_pinned have served, all of them members of this
    // context, its jobs or its slots (stable addresses; p == nullptr: given back).  Everything is scratch and is filled,
    // except the STATE listed here, which a call leaves for the next one by design:
    //   counters2[set], hot-count words [0, (kMaxLevel + 1) * counters_nf): zero between calls.  ensure_level_set zeroes
    //     them at allocation, the response kernels count them up, end_op zeroes them again behind the component kernels that
    //     consumed them (begin_op relies on it: no memset on the pixel stream).
    //   counters2[set], status words [(kMaxLevel + 1) * counters_nf, 2 * ...): zero unless a call reported.  Zeroed at
    //     allocation; the kernels only ever OR into them; inspect_status (mrgingham_amd_sync, harvest_status) clears what it
    //     has read.  The PATH words behind them are scratch (the classify kernel writes a frame's word before any kernel of
    //     that call reads it) and are filled.
    //   sparse_stat: word 0 counts the sparse fallbacks since mrgingham_amd_sparse_fallbacks last read it.  Zeroed where it
    //     is allocated (chain.hip, boards.hip), added to by the kernels, zeroed again by the read-out.
    //   clk: two counters that add up over the probed launches until mrgingham_amd_sclk_mhz reads and zeroes them; zeroed
    //     where they are allocated (mrgingham_amd_set_kernel_timing).
    //   grid_stat: eight counters of the device grid finder that add up until mrgingham_amd_find_grids_stats reads them;
    //     zeroed where they are allocated (grid_find.hip).
    // No page-locked buffer is state: status_pin is read only behind the copy end_op queues (status_copied), a job's pin
    // only while the job is in flight, and the fill completes every job first.
    int scratch_fill = -1;
    std::vector<mrg::DevBuf*> scratch_bufs;
    std::vector<mrg::PinBuf*> pinned_bufs;
    mrg::LevelScratch lvs[kMaxSets][mrg::kMaxLevel + 1];
    mrg::DevBuf counters2[kMaxSets];  // per scratch set: hot_cnt words [level][counters_nf], then status words, then path words (STATE but for the path words: see scratch_fill)
    int counters_nf = 0;
    struct PointScratch { mrg::DevBuf leader, need, nseeds, seeds, sroot, cand_xy, cand_counts, cell_list, cell_cnt, flag_list; } pts[kMaxSets];  // per scratch set
    mrg::DevBuf aux_img, io_frame, io_out, io_counts;
    mrg::PinBuf io_res_pin;  // page-locked: count + first candidates of the single-frame detector
    // page-locked copies of the sets' status words ([level][counters_nf], what mrgingham_amd_sync inspects): they follow every
    // op on its component stream (end_op), so that the sync behind it reads host memory instead of making a blocking copy;
    // allocated with counters2 (ensure_level_set): status_pin.bytes is what counters_nf implies, or 0 where that failed
    mrg::PinBuf status_pin[kMaxSets];
    bool status_copied[kMaxSets] = {};  // the LAST op on the set left its words in status_pin
    mrg::PinBuf io_pin;  // page-locked staging of mrgingham_ChESS_response_5's way back
    mrg::Event io_ev[4];
    mrg::DevBuf clk;  // two u64: shader cycles and constant-rate ticks of the probed workgroups (mrgingham_amd_sclk_mhz); STATE: see scratch_fill
    mrg::DevBuf pre_scratch, pre_tmp, pre_out, pre16_scratch, io_frame16, dbg_img, dbg_resp, blob_scratch, blob_nodes, blob_out;
    // blob detector (blobs.hip): a batch is worked through in chunks of frames whose plane scratch (blob_scratch) stays
    // within the budget; option "blob_chunk_frames" (test hook): at most that many frames per chunk, 0 = by budget
    size_t blob_plane_budget = (size_t)1 << 30;
    int blob_chunk_frames = 0;
    mrg::Event blob_ev[2];  // around a chunk's kernels while kernel timing is on
    double blob_stat[8] = {};    // mrgingham_amd_blobs_stats (+ [7]: frames)
    // The two chunk slots of the file loaders (loader.hip: loader_ring): two chunks of files in flight, one being decoded
    // into its page-locked staging while the other uploads into its device image and runs its kernels; `ev` follows the
    // chunk's last launch.  Every file-list loader uses them: mrgingham_amd_read_jpegs_batch (jpeg_idct.hip; staging:
    // coefficients | tables), _read_pngs_batch (png_recon.hip; scanlines), _read_pgms_batch (pgm_unpack.hip; payloads),
    // _read_tiffs_batch (tiff_decode.hip; files, strip tables), _read_bmps_batch (bmp_unpack.hip; grey tables | pixel
    // arrays) and _read_pnms_batch (pnm_unpack.hip; rasters).  Their calls never overlap, because all are synchronous,
    // and each call sizes and fills what it reads: nothing a call leaves in a slot matters to the next.  The staging is zero only until its first use (ensure_pinned zeroes it when it grows); that is enough,
    // because the IDCT kernel never reads a block outside width x height, and every decoded file covers those
    // (tests/test_gpu_scratch_fill.py runs every loader on staging filled with 0x7F and 0xFF).
    // Option "jpeg_chunk_frames" (test hook): at most that many frames per chunk, 0 = by jpeg_coef_budget
    struct LoaderSlot {
        mrg::DevBuf dev;
        mrg::PinBuf pin;
        mrg::Event ev;
    } loader_slot[2];
    size_t jpeg_coef_budget = (size_t)1 << 30;  // both device buffers together, for every loader
    int jpeg_chunk_frames = 0;
    // the device entropy path of the loader and mrgingham_amd_jpeg_entropy_batch (jpeg_huff.hip): per chunk slot one
    // staging image (jpeg_stage.h has the layout), page-locked on the host and mirrored on the device, both grown on demand.  Options "jpeg_entropy" (0: host threads
    // decode, 1: the device where the file has restart intervals), "jpeg_entropy_max_interval" (MCUs one lane may be
    // handed), "jpeg_entropy_memset" (0: lanes write whole blocks, 1: the area is zeroed in front and lanes store non-zeros)
    mrg::DevBuf jpeg_huff_dev[2];
    mrg::PinBuf jpeg_huff_pin[2];
    int jpeg_entropy = 0;
    int jpeg_entropy_max_interval = 1024;
    int jpeg_entropy_memset = 0;
    // files without restart intervals on the device (jpeg_huff_sync.hip): per chunk slot a staging image of their own
    // (jpeg_stage.h) and the device-only records of the subsequences.  Options "jpeg_sync" (0: such files keep the host decoder), "jpeg_sync_subsequence" (bytes per lane),
    // "jpeg_sync_max_rounds" (0: 8192 / jpeg_sync_subsequence), "jpeg_sync_time_phase" (tools: what kernel timing brackets)
    mrg::DevBuf jpeg_sync_dev[2], jpeg_sync_rec[2];
    mrg::PinBuf jpeg_sync_pin[2];
    int jpeg_sync = 0;
    int jpeg_sync_subsequence = 128;  // (measured: DESIGN.md section 4.10)
    int jpeg_sync_max_rounds = 0;
    int jpeg_sync_time_phase = 0;
    // mrgingham_amd_read_pngs_batch / _png_reconstruct_batch (png_recon.hip): the loader runs on loader_slot, within
    // jpeg_coef_budget; png_row: per frame of a launch the padded row that lane R - 1 hands to lane 0 of the next round;
    // option "png_chunk_frames" (test hook): at most that many files per chunk, 0 = by the budget
    mrg::DevBuf png_row;
    int png_chunk_frames = 0;
    // mrgingham_amd_read_pgms_batch (pgm_unpack.hip): on loader_slot within jpeg_coef_budget as well (staging: the files'
    // payloads); option "pgm_chunk_frames" (test hook): at most that many files per chunk, 0 = by the budget
    int pgm_chunk_frames = 0;
    // mrgingham_amd_read_bmps_batch (bmp_unpack.hip): on loader_slot within jpeg_coef_budget as well (staging: the files'
    // grey tables and pixel arrays); options "bmp_chunk_frames" (test hook, as above) and "bmp_unpack" (1: the device
    // unpacks the pixel arrays; 0: the host threads decode every file)
    int bmp_chunk_frames = 0;
    int bmp_unpack = 1;
    // mrgingham_amd_read_pnms_batch (pnm_unpack.hip): on loader_slot within jpeg_coef_budget as well (staging: the files'
    // rasters); options "pnm_chunk_frames" (test hook, as above) and "pnm_unpack" (1: the device unpacks the rasters; 0: the
    // host threads decode every file)
    int pnm_chunk_frames = 0;
    int pnm_unpack = 1;
    // mrgingham_amd_read_tiffs_batch / _tiff_decode_batch (tiff_decode.hip): the loader runs on loader_slot within
    // jpeg_coef_budget too (staging: the files as they lie on disk, their strip tables); tiff_raw: the decoded strips of an
    // LZW launch, rowbytes x height per frame; tiff_table: 4096 dwords per lane in flight, interleaved by lane;
    // tiff_broken: per frame, set by a lane whose strip broke a rule.  Options "tiff_chunk_frames" (test hook: at most
    // that many files per chunk, 0 = by the budget), "tiff_lzw_max_strip" (decoded bytes of an LZW strip above which a
    // file keeps the host decoder) and "tiff_lzw_lanes" (test hook: lanes in flight of the LZW launch, 0 = 16384)
    // Deflate strips: tiff_inflate_table: 1280 16-bit words per lane in flight (at most 131072), interleaved by lane.
    // Options "tiff_deflate" (1: mrgingham_amd_read_tiffs_batch sends Deflate files through the device; 0, the default:
    // they keep the host threads), "tiff_deflate_max_strip" (decoded bytes of a Deflate strip above which a file keeps the
    // host decoder) and "tiff_deflate_lanes" (test hook: lanes in flight of the Deflate launch, 0 = 131072)
    mrg::DevBuf tiff_raw, tiff_table, tiff_broken, tiff_inflate_table;
    int tiff_chunk_frames = 0;
    int tiff_lzw_max_strip = 64 << 10;  // (measured: DESIGN.md section 4.14)
    int tiff_lzw_lanes = 0;
    int tiff_deflate = 0;
    int tiff_deflate_max_strip = 8 << 10;  // (measured: DESIGN.md section 4.15)
    int tiff_deflate_lanes = 0;
    mrg::DevBuf fb_xy, fb_cnt, fb_pts, fb_lv, fb_np, fb_frames, fb_frames2;  // find_boards_batch: candidates, counts, boards, levels, point counts
    // find_boards_batch's frame-by-frame retries (full-capacity detect, 1-by-1 refine) run on a single-frame
    // context of THIS context's device, created on first use -- not on the calling thread's default context, which
    // lives on MRGINGHAM_AMD_DEVICE / device 0 and cannot touch another GPU's frames
    mrgingham_amd_ctx* one = nullptr;
    HostPool submit_pool;  // mrgingham_amd_chain_multi: the thread that queues this context's shard
    HostPool pool;  // preprocessing: extrema + tile histograms + LUTs, CLAHE output before the blur
    // mrgingham_amd_find_boards_submit / _collect: one job per scratch set (its level images stay in the set's scratch
    // between the first pass and the refinement)
    struct BoardsJob {
        int state = 0;  // 0 free, 1 first pass queued, 2 host part done (refinement queued, or nothing to refine)
        int ticket = -1, set = 0;
        mrgingham_amd_frames fr{};
        int gridn = 0, level_arg = 0, nthreads = 0, nlev = 0, levs[3] = {0, 0, 0}, cap = 0;
        double* h_boards = nullptr;
        signed char* h_found = nullptr;
        signed char* h_levels = nullptr;  // optional: the refinement level of every corner, [frame][gridn^2]
        bool do_refine = true;
        mrg::Event ev_a, ev_b;
        mrg::Event ev_a0, ev_b0;  // where the two device parts begin (mrgingham_amd_find_boards_stats)
        bool refine_queued = false;
        int top = 0;  // the highest level a board of the job was found at (levels below it are refined)
        // device images of the pinned staging, laid out like it (fb_layout) so that each direction is ONE copy:
        // d_cnt = counts | candidates (first pass), d_pts = boards | levels | point counts (refinement), d_pts0 = boards |
        // levels as they went in (what the dense repeat of a sparse refinement starts from)
        mrg::DevBuf d_cnt, d_pts, d_pts0;
        mrg::PinBuf pin;  // pinned host staging: counts, candidates | boards, levels, point counts
        // option "find_boards_grid" 1 (as the job was submitted): the device finder's statuses | indices of every list of the
        // first pass, [level][frame], on the device and in pinned host memory
        bool grid_device = false;
        mrg::DevBuf d_grid;
        mrg::PinBuf pin_grid;
        // the host part in progress (fb_host_begin .. fb_host_end): candidate lists of frames re-run at full capacity,
        // the frame counter of the grid-finder threads
        std::vector<std::vector<int32_t>> big;
        std::atomic<int> next{0};
        bool grid_running = false;
        int nworkers = 0;
        mrgingham_amd_ctx* owner = nullptr;
    } jobs[kMaxSets];
    // mrgingham_amd_chain_multi: this context's shard of the outputs before it travels to the first context's device
    mrg::DevBuf mg_pts, mg_lv, mg_np;
    mrg::Stream mg_stream;
    mrg::Event mg_done;
    bool mg_pending = false;
    int next_ticket = 0;
    std::vector<std::pair<int, int>> done_tickets;  // (ticket, status) of jobs completed before they were collected
    int fb_pipeline = 1;  // option "find_boards_pipeline"
    // mrgingham_amd_find_boards_stats: host milliseconds by phase of submit / collect, batches, and what the grid-finder
    // threads did (their thread-local clocks, grid.h, added up under the mutex when a worker leaves)
    double fb_prof[10] = {};
    long fb_prof_n = 0;
    int fb_threads_used = 0;
    double fb_dev_ms[2] = {0, 0};  // device milliseconds: first passes (submit .. candidates on the host), refinements
    std::mutex fb_stat_mu;
    mrg::GridPhaseClock fb_grid{0, 0, 0, 0, 0, 0};
    // The device grid finder (grid_find.hip).  grid_slots: per scratch set, one GfFar (rings,
    // adjacency lists) per workgroup of the launch -- scratch, written before it is read.  grid_stat: eight 64-bit counters
    // the kernel adds to (lists, found, none, declined -1 .. -5) until mrgingham_amd_find_grids_stats reads them; STATE: see
    // scratch_fill.  Options "find_grids_guard_bits" (the guard band is 2^-bits) and "find_boards_grid" (1: the pipelined
    // find_boards orders the candidates of levels 3..1 on the device and its host threads finish what the device declined;
    // every host finder call of such a job starts its rings at the canonical neighbour).  fb_grid_fallbacks: lists of such
    // jobs that the host finder answered because the device had declined them (under fb_stat_mu).
    mrg::DevBuf grid_slots[kMaxSets], grid_stat;
    int find_grids_guard_bits = 33;
    int fb_grid_device = 0;
    long long fb_grid_fallbacks = 0;
    int pts_nframes = 0, pts_pitch = 0;
    // levels (and frame counts) whose status words must be checked at the next sync
    int pending_frames[kMaxSets][mrg::kMaxLevel + 1] = {};

    // dominant-kernel timing
    bool timing = false;
    bool clk_on = false;  // the engine-clock probe of the level-0 response launches (mrgingham_amd_sclk_mhz)
    mrg::TimingEvents timing_events;
    std::vector<int32_t> host_status;
    std::vector<char> io_host_block;  // refine_on_device: the points block as it travels
};

namespace mrg {

// THE SPARSE SCHEDULE (option "sparse_refine"; chain_batch and the refinement of find_boards).  1 = where it pays: the
// dense response of a small call is cheaper than the longer chain -- measured crossover at 80-100 Mpx per call, e.g.
// 64 x 1280x960 or 8 x 4096x3072; 2 = always.
constexpr long long kSparsePaysPixels = 96ll << 20;  // option "sparse_refine" 1: calls with at least this many frame pixels
// this context can take it for points that start at level `top` (such a context keeps three scratch sets: choose_sets) ...
static inline bool sparse_possible(const mrgingham_amd_ctx* ctx, int top) {
    return ctx->sparse_refine && top >= 1 && ctx->cc_lds && !ctx->use_v0;
}
// ... and a call over `pixels` frame pixels in all does take it
static inline bool sparse_applies(const mrgingham_amd_ctx* ctx, int top, long long pixels) {
    return sparse_possible(ctx, top) && top <= kRefineLevelsMax && (ctx->sparse_refine == 2 || pixels >= kSparsePaysPixels);
}
constexpr int kCellsPerPoint = 9;  // sparse refinement: distinct cells the 3 x 3 seeds of one point can mark (2 x 2 each, one pixel apart)

// api.hip: errors, buffers, level scratch
int fail(mrgingham_amd_ctx* ctx, int code, const char* fmt, ...);
// at least `bytes` of device memory: the only place that allocates context scratch (and counts it, and notes the buffer
// in ctx->scratch_bufs, and fills what it allocates while ctx->scratch_fill is on)
int ensure(mrgingham_amd_ctx* ctx, DevBuf& b, size_t bytes);
void release(mrgingham_amd_ctx* ctx, DevBuf& b);  // gives it back now
// MRGINGHAM_AMD_SCRATCH_FILL as a fill byte (decimal or 0x..), -1 where it is unset, empty or no number in 0 .. 255
int scratch_fill_from_env();
// at least `bytes` of page-locked memory; growth allocates bytes + bytes / slack_divisor (0: no slack), zeroed if asked
// (while ctx->scratch_fill is on: filled with that byte, asked or not)
int ensure_pinned(mrgingham_amd_ctx* ctx, PinBuf& b, size_t bytes, int slack_divisor, bool zero_on_growth);
hipError_t copy_rows_async(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes, size_t rows,
                           hipMemcpyKind kind, hipStream_t s);
int level_dims(int W, int H, int level, int* w, int* h);
int validate_frames(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* f);
int ensure_level_set(mrgingham_amd_ctx* ctx, int set, int level, int nframes, int W, int H, int pitch);
int choose_sets(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr);
int ensure_level(mrgingham_amd_ctx* ctx, int level, int nframes, int W, int H, int pitch);
int ensure_points(mrgingham_amd_ctx* ctx, int nframes, int pitch);
int queue_preprocess16(mrgingham_amd_ctx* ctx, const uint16_t* d_frames, int64_t frame_pitch, int nframes, int width, int height,
                       int stride, int do_clahe, int blur_radius, uint8_t* d_out, hipStream_t s);
int harvest_status(mrgingham_amd_ctx* ctx, int set, int level, int* rc, bool quiet = false);
void launch_one_level_image(const mrgingham_amd_frames* fr, int level, uint8_t* out, int w, int h, hipStream_t s);

// chain.hip: the scratch-set rotation of a call, its pixel-stream and component-stream work
// an idle timing event, or a new one (NULL if it cannot be created); it stays the context's (TimingEvents)
hipEvent_t timing_event(mrgingham_amd_ctx* ctx);
// Kernel timing around the launches of the JPEG entropy decoders (jpeg_huff.hip): the caller numbers the boundaries
// between its launches and calls tick at each; with timing on, the pair of events opens at boundary `open` and closes --
// and is handed to mrgingham_amd_chess_kernel_ms -- at `close`.  An event that cannot be created is an error.
struct TimingBracket {
    hipEvent_t mark[2] = {nullptr, nullptr};
    int open = 0, close = 0;
    hipError_t begin(mrgingham_amd_ctx* ctx, int open_at, int close_at);
    hipError_t tick(mrgingham_amd_ctx* ctx, int boundary, hipStream_t s);
};
// launch(f0, n) over slabs of at most 65535 frames (a grid's y and z extents)
template <class F>
void for_frame_slabs(int nframes, F&& launch) {
    for (int f0 = 0; f0 < nframes; f0 += 65535) launch(f0, (unsigned)(nframes - f0 < 65535 ? nframes - f0 : 65535));
}
void begin_op(mrgingham_amd_ctx* ctx, int max_level);
void order_after_previous(mrgingham_amd_ctx* ctx, std::initializer_list<mrgingham_amd_ctx::Span> w,
                          std::initializer_list<mrgingham_amd_ctx::Span> r);
void end_op(mrgingham_amd_ctx* ctx);
void launch_chess_any(mrgingham_amd_ctx* ctx, const LevelBatch& lb, const CompTables& t, int n, bool clamp, bool hot,
                      hipStream_t s, bool time_it);
void queue_level_images(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int max_level, bool levels_1_to_3 = true,
                        bool gentle = false);
LevelBatch level_batch_of(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int level);
LevelBatch queue_level_chess(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int level);
int queue_chess_levels(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int hi, int lo, bool merge_l0, LevelBatch* lbs,
                       hipEvent_t* lev_ev, hipEvent_t* l0_mark);
int queue_sparse_levels(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int top, RefineIO io,
                        const SparseRestore& restore, bool dense_only = false);

// reference.hip: one frame that lives on the device
bool check_level_and_layout(const char* fn, int Nrows, int Ncols, int stride, int level);
bool detect_one_frame_all(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr1, int level, std::vector<int32_t>& xy,
                          int32_t* count_out, bool debug = false, const char* debug_image_filename = nullptr);
int refine_on_device(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, double* points_xy, signed char* level,
                     int Npoints, int image_pyramid_level, bool debug = false, const char* debug_image_filename = nullptr);

// blobs.hip: cv::SimpleBlobDetector as find_blobs.cc:14-46 configures it (device border following, host filters)
int blob_detect_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int nthreads, std::vector<std::vector<int32_t>>& xy,
                      std::vector<char>& bad);
int host_threads(int nthreads);

// jpeg_idct.hip
// a coefficient area of blocks_w x blocks_h blocks per frame for width x height pixels: 0, or MRGINGHAM_AMD_ERR_ARG
int check_coef_area(mrgingham_amd_ctx* ctx, const int16_t* d_coef, int64_t coef_pitch, int width, int height, int blocks_w, int blocks_h);
void launch_jpeg_idct(const int16_t* d_coef, int64_t coef_pitch, const uint16_t* d_quant, int nframes, int width, int height,
                      int blocks_w, uint8_t* d_out, int64_t frame_pitch, int stride, hipStream_t s);

// loader.hip: what the file-list loaders share -- read_jpegs_batch (jpeg_idct.hip) and its device-entropy route
// (jpeg_huff.hip), read_pngs_batch (png_recon.hip), read_pgms_batch (pgm_unpack.hip), read_tiffs_batch (tiff_decode.hip),
// read_bmps_batch (bmp_unpack.hip), read_pnms_batch (pnm_unpack.hip)
// the descriptor of a file list and its frames: 0, or MRGINGHAM_AMD_ERR_ARG with "bad <format> file batch descriptor"
// (elem: bytes per sample, 1 or 2; a NULL entry of filenames is refused)
int check_file_batch(mrgingham_amd_ctx* ctx, const char* format, const char* const* filenames, int nfiles, int width, int height,
                     size_t elem, const void* d_out, int64_t frame_pitch, int stride, const int32_t* h_status);
// zeroes width x height samples of `elem` bytes of frame `frame` (of a file that failed)
hipError_t zero_frame(void* d_out, int64_t frame, int64_t frame_pitch, int stride, int width, int height, size_t elem, hipStream_t s);
// the `after` of a loader: zeroes the frames (samples of `elem` bytes) of the chunk's files whose h_status is not 0
std::function<int(int k, int f0, int n)> zero_failed_frames(mrgingham_amd_ctx* ctx, void* d_out, int64_t frame_pitch, int stride, int width,
                                                            int height, size_t elem, const int32_t* h_status);
// the launch shape (unpack_rows.h) of an unpack kernel over nrows rows of row_bytes_out destination bytes on the context's
// device; the pitches in bytes
int unpack_launch_shape(mrgingham_amd_ctx* ctx, const void* d_out, long long frame_pitch_b, long long stride_b, long long row_bytes_out,
                        long long nrows, UnpackShape* shape);
// The two-slot chunk ring on ctx->pix: chunks of `chunk` files alternate between the slots (one slot if there is one
// chunk), whose device buffers are grown to dev_bytes and whose staging to pin_bytes (0: the stage grows it when it
// needs it).  Per chunk: wait for the event of the slot's previous chunk and, given `finish`, finish(k) behind it; then
// stage(k, f0, n) decodes files [f0, f0 + n) on the host and queues their uploads and launches; the slot's event is
// recorded; after(k, f0, n), if given, queues what goes behind the record (the zeroing of failed frames).  At the end
// the chunks still in flight are finished in slot order (only if there is a `finish`) and the stream is synchronised.
using LoaderStage = std::function<int(int k, int f0, int n)>;
int loader_ring(mrgingham_amd_ctx* ctx, int nfiles, int chunk, size_t dev_bytes, size_t pin_bytes, const LoaderStage& stage,
                const LoaderStage& after, const std::function<int(int k)>& finish);
// The loader of the formats whose raster goes to the device as it lies in the file (read_bmps_batch, read_pnms_batch), a
// stage of loader_ring: a header pass over all files, one staging area per file of a chunk sized by the largest raster,
// one upload per chunk, one launch per run of files with the same layout; a file the kernel does not take is decoded by
// its host thread (read_image) into its area and copied to its frame.  What a format brings (i: index into the list):
struct StagedThread {  // what a host thread keeps from file to file
    std::vector<uint8_t> head;
    Image im;
};
struct StagedFormat {
    size_t front;   // bytes per file in front of a chunk's areas, uploaded with them (BMP: the grey table), or 0
    int chunk_cap;  // the format's "<format>_chunk_frames" option
    // the header pass: the file's status (0, -1, -2); with 0, *route = 1 (its raster through the kernel, *raster_bytes of
    // it) or 2 (decoded by a host thread), and the format's own record of the layout
    std::function<int32_t(int i, StagedThread& t, int* route, size_t* raster_bytes)> header;
    // a route-1 file's raster to dst, its front bytes to `front`; false: unreadable
    std::function<bool(int i, StagedThread& t, uint8_t* dst, uint8_t* front)> stage_raster;
    std::function<bool(int i, int j)> same_launch;  // files i and j, both route 1, can share a launch
    // the launch over n files from file i on: rasters at d_payload, payload_pitch apart, front bytes at d_front, into `frame`
    std::function<int(int i, int n, const uint8_t* d_payload, int64_t payload_pitch, const uint8_t* d_front, uint8_t* frame)> launch;
};
// (arguments checked by the caller: check_file_batch; bits 8 or 16 of a frame's samples)
int read_staged_batch(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height, int bits, void* d_out,
                      int64_t frame_pitch, int stride, int nthreads, int32_t* h_status, const StagedFormat& fmt);
// jpeg_huff.hip: mrgingham_amd_read_jpegs_batch with option "jpeg_entropy" 1 (arguments checked, geometry chosen there)
int read_jpegs_device_entropy(mrgingham_amd_ctx* ctx, const char* const* filenames, int nfiles, int width, int height,
                              uint8_t* d_out, int64_t frame_pitch, int stride, int nthreads, int32_t* h_status, int bw, int bh,
                              int chunk);

// jpeg_huff_sync.hip: files without restart intervals (option "jpeg_sync"), for the chunk driver in jpeg_huff.hip; the
// files of a chunk and the layout of their staging image are jpeg_stage.h
struct JpegStageFile;
struct JpegSyncLayout;
// grows slot k's buffers to what the layout asks for (nothing for a chunk without sync files)
int jpeg_sync_grow(mrgingham_amd_ctx* ctx, int k, const JpegSyncLayout& l);
// queues the upload of slot k's filled image, the zeroing of the sync files' coefficient areas (file i of the chunk at
// d_coef + i * coef_pitch), round 0, the update rounds, the scan, the write pass and the download of the per-file words
int jpeg_sync_launch(mrgingham_amd_ctx* ctx, int k, const JpegSyncLayout& l, const JpegStageFile* files, int nfiles, int16_t* d_coef,
                     int64_t coef_pitch, size_t area_elems, hipStream_t s);
// after the stream has passed the download, sync file i: 0 decoded, -1 unreadable, -3 not converged within the cap
int32_t jpeg_sync_status(const mrgingham_amd_ctx* ctx, int k, const JpegSyncLayout& l, int i);

// boards.hip
struct GridScratch { std::vector<PointI> cand; std::vector<PointD> grid; };
bool grid_of_candidates(const int32_t* xy, int n, int gridn, double* out, GridScratch* scratch = nullptr);
int find_board_on_device(mrgingham_amd_ctx* ctx, const char* who, const mrgingham_amd_frames* fr, int gridn,
                         int image_pyramid_level, bool do_refine, std::vector<PointD>& board, std::vector<signed char>& lv,
                         bool debug = false, const char* debug_image_filename = nullptr);
void fb_drain(mrgingham_amd_ctx* ctx);

// grid_find.hip: the scratch of a launch over nlists lists on scratch set `set` (launch_find_grids grows it itself; a
// caller that must not allocate behind begin_op calls this in front of it); nlists candidate lists (capacity pairs apart, counts beside them) to board indices and statuses, one
// launch on s over the slots of scratch set `set`
int ensure_find_grids(mrgingham_amd_ctx* ctx, int set, int nlists);
int launch_find_grids(mrgingham_amd_ctx* ctx, int set, const int32_t* d_xy, const int32_t* d_counts, int nlists, int capacity, int gridn,
                      int32_t* d_index, int32_t* d_status, hipStream_t s);

// accessors the chain path calls per level: inline
static inline LevelScratch* cur_levels(mrgingham_amd_ctx* ctx) { return ctx->lvs[ctx->cur]; }
static inline hipStream_t cur_cc(mrgingham_amd_ctx* ctx) { return ctx->ccs[ctx->cur]; }
static inline int32_t* hot_cnt_of(mrgingham_amd_ctx* ctx, int level) {
    return (int32_t*)ctx->counters2[ctx->cur].p + (size_t)level * ctx->counters_nf;
}
static inline int32_t* status_of(mrgingham_amd_ctx* ctx, int level) {
    return (int32_t*)ctx->counters2[ctx->cur].p + (size_t)(kMaxLevel + 1 + level) * ctx->counters_nf;
}
static inline int32_t* path_of(mrgingham_amd_ctx* ctx, int level) {
    return (int32_t*)ctx->counters2[ctx->cur].p + (size_t)(2 * (kMaxLevel + 1) + level) * ctx->counters_nf;
}

// this call leaves status words of `nframes` frames at `level`: the next sync looks at them
static inline void note_pending(mrgingham_amd_ctx* ctx, int level, int nframes) {
    int& n = ctx->pending_frames[ctx->cur][level];
    if (nframes > n) n = nframes;
}
// a refinement of the caller's points over the point scratch of `set`
static inline RefineIO refine_io_of(mrgingham_amd_ctx* ctx, int set, double* points, signed char* levels, const int32_t* npoints,
                                    int pitch, int32_t* nrefined) {
    auto& ps = ctx->pts[set];
    return RefineIO{points, levels, npoints, pitch, nrefined, (int32_t*)ps.leader.p, (int32_t*)ps.need.p,
                    (int32_t*)ps.nseeds.p, (uint32_t*)ps.seeds.p, (int32_t*)ps.sroot.p};
}

static inline CompTables tables_of(mrgingham_amd_ctx* ctx, int level) {
    const LevelScratch& L = cur_levels(ctx)[level];
    CompTables t;
    t.cap = L.cap;
    t.hot_cnt = hot_cnt_of(ctx, level);
    t.hot_xy = (uint32_t*)L.hot_xy.p;
    t.parent = (int32_t*)L.parent.p;
    t.comp_cnt = (int32_t*)L.comp_cnt.p;
    t.comp_box = (int4*)L.comp_box.p;
    t.roots = (int32_t*)L.roots.p;
    t.comp_first = (int32_t*)L.comp_first.p;
    t.gidx = (uint2*)L.gidx.p;
    t.gw = (L.w + 7) / 8;
    t.gidx_pitch = (long long)t.gw * L.h;
    t.arena = (uint32_t*)L.arena.p;
    t.arena_cap = L.arena_cap;
    t.cand_cap = L.cand_cap;
    t.cand = (Cand*)L.cand.p;
    t.sortkeys = (unsigned long long*)L.sortkeys.p;
    t.sort_cap = L.sort_cap;
    t.status = status_of(ctx, level);
    t.path = path_of(ctx, level);
    t.lds_path = ctx->cc_lds;
    t.only = nullptr;
    return t;
}

// The reference-symbol wrappers (and the calls that span several devices: chain_multi, sync_multi, stream_wait_multi,
// gather_rccl) work on the calling thread's context, which may live on another device than the one the
// CALLER has current (the k-th thread's context is on device k % devices): they put the caller's device back when they
// return -- a worker thread of a multi-GPU host (PyTorch, ...) keeps the current device it had.
struct CallerDevice {
    int prev = -1;
    CallerDevice() {
        if (hipGetDevice(&prev) != hipSuccess) {
            prev = -1;
            (void)hipGetLastError();
        }
    }
    ~CallerDevice() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace mrg
