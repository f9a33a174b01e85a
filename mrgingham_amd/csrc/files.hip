// Host side of libmrgingham_amd.so, a list of image files to boards (mrgingham_amd_find_boards_files): the schedule that
// keeps the kernels of the loaders, of the preprocessing (preprocess.hip, preprocess16_batch.hip) and of the board
// detector (boards.hip) fed from a list of several sizes and formats.  No kernel of its own.
//
//   loader thread, LOADER context            calling thread, DETECTOR context
//   ------------------------------           ---------------------------------------------------------
//   wait: chunk c - 3 collected              wait: chunk c loaded            (or collect the oldest job meanwhile)
//   host files -> page-locked staging        pix stream waits for the slot's upload event
//     (host threads), upload, event          preprocess_batch on the pix stream, find_boards_submit_ex
//   runs of a batch route -> its loader      collect chunk c - k, scatter its results, advance the final prefix
//   chunk c loaded                           (one-image files are processed when the prefix reaches them)
//
// The route of a file (Route below); every run of consecutive files of a chunk with one batch route is one call of its
// loader, straight into the chunk's frames:
//
//   route   files                            loader (kernels)                              where the caller set
//   -----   ------------------------------   -------------------------------------------   ---------------------------------
//   host    whatever has no other route      read_image on the host threads
//   JPEG    JPEG                             read_jpegs_batch (jpeg_idct, jpeg_huff*.hip)   (always)
//   PNG     PNG without a palette            read_pngs_batch (png_recon.hip)                MRGINGHAM_AMD_FILES_PNG_DEVICE
//   PGM     16-bit PGM                       read_pgms_batch (pgm_unpack.hip)               MRGINGHAM_AMD_FILES_DEEP_CHUNKS
//   TIFF    TIFF                             read_tiffs_batch (tiff_decode.hip)             MRGINGHAM_AMD_FILES_TIFF_DEVICE
//   BMP     BMP                              read_bmps_batch (bmp_unpack.hip)               MRGINGHAM_AMD_FILES_BMP_DEVICE
//   PNM     PBM / PAM                        read_pnms_batch (pnm_unpack.hip)               MRGINGHAM_AMD_FILES_PNM_DEVICE
//
// 16-bit files are in chunks of their own, as uint16 frames, only with MRGINGHAM_AMD_FILES_DEEP_CHUNKS (the PNG, TIFF and
// PNM routes take them then); the detector side runs preprocess16_batch on such a chunk.
//
// The ring has three slots; slot c % 3 holds chunk c from its load to its collect.  What orders the two contexts:
// loader -> detector, the upload event of the slot (read_jpegs_batch is complete when it returns); detector -> loader,
// the collect of the chunk that held the slot (a collected job has no device work left that reads its frames).  Every
// wait on the condition variable also ends when the other side has failed.
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <deque>

#include "ctx.h"
#include "files_plan.h"
#include "image_io.h"

namespace {

using namespace mrg;

constexpr int kRing = 3;                            // chunks between their load and their collect
constexpr size_t kBufferBytes = (size_t)1 << 30;    // one ring buffer (a chunk's raw or preprocessed frames): the ring is 6 of them

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

enum class Route : int8_t { host, jpeg, png, pgm, tiff, bmp, pnm };  // (the table at the head of the file)

struct FileInfo {
    int w = 0, h = 0, bits = 0, kind = 0;  // kind 0: the probe rejected the file
    Route route = Route::host;
    bool batch_loader() const { return route != Route::host; }
};

// the batch loaders behind one signature (the JPEG and BMP loaders take no depth: their frames are bytes)
int read_run(mrgingham_amd_ctx* ctx, Route via, const char* const* names, int n, int w, int h, int bits, uint8_t* frames, int64_t pitch,
             int nthreads, int32_t* st) {
    switch (via) {
        case Route::jpeg: return mrgingham_amd_read_jpegs_batch(ctx, names, n, w, h, frames, pitch, w, nthreads, st);
        case Route::png: return mrgingham_amd_read_pngs_batch(ctx, names, n, w, h, bits, frames, pitch, w, nthreads, st);
        case Route::pgm: return mrgingham_amd_read_pgms_batch(ctx, names, n, w, h, bits, frames, pitch, w, nthreads, st);
        case Route::tiff: return mrgingham_amd_read_tiffs_batch(ctx, names, n, w, h, bits, frames, pitch, w, nthreads, st);
        case Route::bmp: return mrgingham_amd_read_bmps_batch(ctx, names, n, w, h, frames, pitch, w, nthreads, st);
        case Route::pnm: return mrgingham_amd_read_pnms_batch(ctx, names, n, w, h, bits, frames, pitch, w, nthreads, st);
        case Route::host: break;
    }
    return MRGINGHAM_AMD_ERR_ARG;
}

struct Chunk {
    std::vector<int> files;  // list indices, in slot order
    int w = 0, h = 0, bits = 8;  // one size and one depth
};

struct Slot {
    DevBuf d_raw, d_pre;            // (the slot's own, freed with it: in no context's scratch_bytes)
    PinBuf pin;                     // page-locked staging of the host-decoded files
    Event ev_up;                    // behind the uploads of the chunk in the slot (loader context's pix stream)
    bool uploaded = false;          // ... recorded for that chunk
    std::vector<int32_t> load_status;  // per slot of the chunk: 0 loaded, -1 the decoder rejected the file
    std::vector<double> boards;
    std::vector<signed char> levels, found;
};

struct Pipeline {
    std::mutex mu;
    std::condition_variable cv;
    int loaded = 0, collected = 0;  // chunks
    int failed = 0;                 // the error that stopped a side
    std::string err;
    double loader_wait_ms = 0;
    long n_device_loaded = 0, n_host_decoded = 0;

    void fail(int rc, const std::string& why) {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!failed) {
                failed = rc;
                err = why;
            }
        }
        cv.notify_all();
    }
};

struct Run {
    const char* const* names;
    const mrgingham_amd_files_options* o;
    int batch, nthreads;
    std::vector<FileInfo> info;
    std::vector<Chunk> chunks;
    Slot slots[kRing];
    Pipeline pipe;
    mrgingham_amd_ctx *loader = nullptr, *detector = nullptr;
};

// frames lie dense in a ring buffer, like the one frame of the one-image path (the pitch in samples)
size_t frame_pitch_of(int w, int h) { return (size_t)w * h; }

// One chunk into its slot (loader thread, loader context).  0, or the error that stops the pipeline.
int load_chunk(Run& R, int c) {
    const Chunk& ch = R.chunks[(size_t)c];
    Slot& S = R.slots[c % kRing];
    mrgingham_amd_ctx* ctx = R.loader;
    const int n = (int)ch.files.size();
    const size_t es = (size_t)ch.bits / 8, pitch = frame_pitch_of(ch.w, ch.h) * es, npx = (size_t)ch.w * ch.h * es;  // (bytes)
    hipStream_t s = ctx->pix;
    uint8_t *const d_raw = (uint8_t*)S.d_raw.p, *const pin = (uint8_t*)S.pin.p;
    S.load_status.assign((size_t)n, -1);
    if (S.uploaded) MRG_HIP_CHECK(hipEventSynchronize(S.ev_up));  // (long done: the chunk that recorded it has been collected)
    S.uploaded = false;
    // the host route: the host threads decode into the staging of the slot (a 16-bit chunk: native uint16 samples),
    // consecutive slots go up in one copy
    std::vector<int> host;
    for (int k = 0; k < n; ++k)
        if (!R.info[(size_t)ch.files[(size_t)k]].batch_loader()) host.push_back(k);
    if (!host.empty()) {
        for_files<Image>(ctx->pool, R.nthreads, (int)host.size(), [&](int i, Image& im) {
            const int k = host[(size_t)i];
            if (read_image(R.names[ch.files[(size_t)k]], im) && im.depth == ch.bits && im.w == ch.w && im.h == ch.h) {
                memcpy(pin + (size_t)k * pitch, ch.bits == 8 ? (const void*)im.px8.data() : (const void*)im.px16.data(), npx);
                S.load_status[(size_t)k] = 0;
            } else {
                memset(pin + (size_t)k * pitch, 0, npx);  // (the frame is detected on with its chunk; its result is dropped)
            }
        });
        for (size_t i = 0; i < host.size();) {
            size_t j = i + 1;
            while (j < host.size() && host[j] == host[j - 1] + 1) ++j;
            const size_t k0 = (size_t)host[i], bytes = (j - i) * pitch;
            MRG_HIP_CHECK(hipMemcpyAsync(d_raw + k0 * pitch, pin + k0 * pitch, bytes, hipMemcpyHostToDevice, s));
            i = j;
        }
        MRG_HIP_CHECK(hipEventRecord(S.ev_up, s));
        S.uploaded = true;
    }
    // the batch routes: every run of consecutive slots of one of them is one call of its loader, straight into the chunk's
    // frames
    long nbatch_ok = 0;
    auto route = [&](int k) { return R.info[(size_t)ch.files[(size_t)k]].route; };
    for (int k = 0; k < n;) {
        const Route via = route(k);
        if (via == Route::host) { ++k; continue; }
        int j = k + 1;
        while (j < n && route(j) == via) ++j;
        std::vector<const char*> run;
        for (int i = k; i < j; ++i) run.push_back(R.names[ch.files[(size_t)i]]);
        const int rc = read_run(ctx, via, run.data(), j - k, ch.w, ch.h, ch.bits, d_raw + (size_t)k * pitch, (int64_t)frame_pitch_of(ch.w, ch.h),
                                R.nthreads, S.load_status.data() + k);
        if (rc) return rc;
        for (int i = k; i < j; ++i) {
            if (S.load_status[(size_t)i] == 0) ++nbatch_ok;
            else S.load_status[(size_t)i] = -1;
        }
        k = j;
    }
    long nhost_ok = 0;
    for (int k : host) nhost_ok += S.load_status[(size_t)k] == 0;
    std::lock_guard<std::mutex> lk(R.pipe.mu);
    R.pipe.n_device_loaded += nbatch_ok;
    R.pipe.n_host_decoded += nhost_ok;
    return 0;
}

void loader_main(Run* Rp) {
    Run& R = *Rp;
    Pipeline& P = R.pipe;
    try {
        if (hipSetDevice(R.loader->device) != hipSuccess) {
            P.fail(MRGINGHAM_AMD_ERR_DEVICE, "loader: hipSetDevice failed");
            return;
        }
        for (int c = 0; c < (int)R.chunks.size(); ++c) {
            {
                std::unique_lock<std::mutex> lk(P.mu);
                const double t0 = now_ms();
                P.cv.wait(lk, [&] { return P.failed || c < P.collected + kRing; });
                P.loader_wait_ms += now_ms() - t0;
                if (P.failed) return;
            }
            const int rc = load_chunk(R, c);
            if (rc) {
                P.fail(rc, std::string("loader: ") + mrgingham_amd_last_error(R.loader));
                return;
            }
            {
                std::lock_guard<std::mutex> lk(P.mu);
                P.loaded = c + 1;
            }
            P.cv.notify_all();
        }
    } catch (...) {  // std::bad_alloc
        P.fail(MRGINGHAM_AMD_ERR_DEVICE, "loader: out of host memory");
    }
}

}  // namespace

extern "C" {

int mrgingham_amd_probe_image(const char* filename, int* width, int* height, int* bits, int* kind) {
    return probe_image(filename, width, height, bits, kind) ? 0 : -1;
}

int mrgingham_amd_files_plan(const int32_t* key, int nfiles, int batch_frames, int32_t* chunk_of_file, int32_t* slot_in_chunk,
                             int32_t* nchunks) {
    try {
        return files_plan(key, nfiles, batch_frames, chunk_of_file, slot_in_chunk, nchunks) ? MRGINGHAM_AMD_ERR_ARG : MRGINGHAM_AMD_OK;
    } catch (...) {
        return MRGINGHAM_AMD_ERR_ARG;
    }
}

}  // extern "C"

namespace {

constexpr int kFlagsEx = MRGINGHAM_AMD_FILES_PNG_DEVICE | MRGINGHAM_AMD_FILES_DEEP_CHUNKS, kFlagsEx2 = kFlagsEx | MRGINGHAM_AMD_FILES_TIFF_DEVICE,
              kFlagsEx3 = kFlagsEx2 | MRGINGHAM_AMD_FILES_TIFF_DEFLATE_DEVICE, kFlagsEx4 = kFlagsEx3 | MRGINGHAM_AMD_FILES_BMP_DEVICE,
              kFlagsEx5 = kFlagsEx4 | MRGINGHAM_AMD_FILES_PNM_DEVICE;

// every mrgingham_amd_find_boards_files* entry point: `accepted` is the mask of loader flags that the entry point takes
int find_boards_files(int accepted, const char* const* filenames, int nfiles, const mrgingham_amd_files_options* o, double* h_boards,
                      signed char* h_levels, signed char* h_found_level, int32_t* h_status, void (*progress)(int nfinal, void* cookie),
                      void* cookie, double* stats, int nstats, int loader_flags) {
    // (Deflate strips on the device are a part of the TIFF device route, not a route of their own)
    if ((loader_flags & MRGINGHAM_AMD_FILES_TIFF_DEFLATE_DEVICE) && !(loader_flags & MRGINGHAM_AMD_FILES_TIFF_DEVICE)) return MRGINGHAM_AMD_ERR_ARG;
    if (nfiles < 0 || (loader_flags & ~accepted) || !o || o->gridn < 2 || o->gridn > 1024 || o->image_pyramid_level > kMaxLevel || o->blur_radius < 0 ||
        o->blur_radius > 64 || o->device < -1 || nstats < 0 || (nstats > 0 && !stats) ||
        (nfiles > 0 && (!filenames || !h_boards || !h_levels || !h_found_level || !h_status)))
        return MRGINGHAM_AMD_ERR_ARG;
    for (int i = 0; i < nfiles; ++i)
        if (!filenames[i]) return MRGINGHAM_AMD_ERR_ARG;
    double st[MRGINGHAM_AMD_FILES_STATS] = {};
    auto leave = [&](int rc) {
        for (int i = 0; i < nstats && i < MRGINGHAM_AMD_FILES_STATS; ++i) stats[i] = st[i];
        return rc;
    };
    if (nfiles == 0) {
        if (progress) progress(0, cookie);
        return leave(MRGINGHAM_AMD_OK);
    }
    const CallerDevice caller_device_;
    int device = o->device;
    if (device < 0) device = mrgingham_amd_thread_device();
    if (device < 0) return MRGINGHAM_AMD_ERR_DEVICE;
    if (device >= mrgingham_amd_device_count()) return MRGINGHAM_AMD_ERR_ARG;

    const int N = o->gridn * o->gridn;
    Run R;
    R.names = filenames;
    R.o = o;
    R.nthreads = host_threads(o->nthreads);
    // ---- routing: what every file is, which size bucket it belongs to
    R.info.resize((size_t)nfiles);
    const bool deep_chunks = (loader_flags & MRGINGHAM_AMD_FILES_DEEP_CHUNKS) != 0;
    bool any_deep = false;
    std::vector<int32_t> key((size_t)nfiles, -1);
    {
        HostPool probe_pool;
        for_files(probe_pool, R.nthreads, nfiles, [&](int i) {
            FileInfo& f = R.info[(size_t)i];
            if (!probe_image(filenames[i], &f.w, &f.h, &f.bits, &f.kind)) f = FileInfo{};
            const bool depth_ok = f.bits == 8 || deep_chunks;
            auto asked = [&](int flag) { return (loader_flags & flag) != 0; };
            // (palette PNGs keep the host decoder: read_pngs_batch would hand them to it anyway, one by one)
            f.route = f.kind == 3                                                                    ? Route::jpeg
                      : f.kind == 2 && asked(MRGINGHAM_AMD_FILES_PNG_DEVICE) && depth_ok &&
                              png_header(filenames[i], nullptr, nullptr, nullptr) != 3               ? Route::png
                      : f.kind == 1 && deep_chunks && f.bits == 16                                   ? Route::pgm
                      : f.kind == 4 && asked(MRGINGHAM_AMD_FILES_TIFF_DEVICE) && depth_ok            ? Route::tiff
                      : f.kind == 5 && asked(MRGINGHAM_AMD_FILES_BMP_DEVICE)                         ? Route::bmp
                      : f.kind == 6 && asked(MRGINGHAM_AMD_FILES_PNM_DEVICE) && depth_ok             ? Route::pnm
                                                                                                     : Route::host;
        });
    }
    size_t max_frame = 0, max_host_frame = 0;
    for (int i = 0; i < nfiles; ++i) {
        const FileInfo& f = R.info[(size_t)i];
        h_status[i] = f.kind ? 0 : -1;
        h_found_level[i] = -1;
        // the batch preprocessing refuses CLAHE below 8 x 8 pixels, 16-bit files are in chunks only where the caller asked
        // for it: such files take the one-image path (key -1), like the ones the probe rejected take none
        const bool deep = f.bits == 16;
        if (!f.kind || (deep ? !deep_chunks : f.bits != 8) || (o->do_clahe && (f.w < 8 || f.h < 8))) continue;
        // (sides are at most 32767: 30 bits; bit 30 is the depth, so a chunk holds one size and one depth)
        key[(size_t)i] = (int32_t)(((uint32_t)deep << 30) | ((uint32_t)f.h << 15) | (uint32_t)f.w);
        any_deep = any_deep || deep;
        const size_t fp = frame_pitch_of(f.w, f.h) * (size_t)(f.bits / 8);  // bytes
        if (fp > max_frame) max_frame = fp;
        if (!f.batch_loader() && fp > max_host_frame) max_host_frame = fp;
    }
    R.batch = o->batch_frames > 0 ? o->batch_frames : 64;
    if (max_frame && (size_t)R.batch > kBufferBytes / max_frame) R.batch = (int)(kBufferBytes / max_frame);
    if (R.batch < 1) R.batch = 1;
    std::vector<int32_t> chunk_of((size_t)nfiles), slot_of((size_t)nfiles);
    int32_t nchunks = 0;
    if (files_plan(key.data(), nfiles, R.batch, chunk_of.data(), slot_of.data(), &nchunks)) return MRGINGHAM_AMD_ERR_ARG;
    R.chunks.resize((size_t)nchunks);
    for (int i = 0; i < nfiles; ++i)
        if (chunk_of[(size_t)i] >= 0) {
            Chunk& ch = R.chunks[(size_t)chunk_of[(size_t)i]];
            ch.files.push_back(i);  // (ascending i = ascending slot: files keep list order inside a key)
            ch.w = R.info[(size_t)i].w;
            ch.h = R.info[(size_t)i].h;
            ch.bits = R.info[(size_t)i].bits;
        }

    // ---- the two contexts, the ring
    Pipeline& P = R.pipe;
    const bool preprocess = o->do_clahe || o->blur_radius > 0;
    std::thread loader_thread;
    int rc = 0;
    auto cleanup = [&]() {
        if (loader_thread.joinable()) loader_thread.join();
        if (R.detector) mrgingham_amd_destroy(R.detector);  // (abandons what is in flight, synchronises the device)
        if (R.loader) mrgingham_amd_destroy(R.loader);
    };  // (the slots free themselves when R goes, after the contexts)
    auto setup = [&]() -> int {
        if (nchunks == 0) return 0;
        R.detector = mrgingham_amd_create(device);
        R.loader = mrgingham_amd_create(device);
        if (!R.detector || !R.loader) return MRGINGHAM_AMD_ERR_DEVICE;
        if (o->jpeg_entropy) {
            if (mrgingham_amd_set_option(R.loader, "jpeg_entropy", 1) || mrgingham_amd_set_option(R.loader, "jpeg_sync", 1))
                return MRGINGHAM_AMD_ERR_DEVICE;
        }
        if ((loader_flags & MRGINGHAM_AMD_FILES_TIFF_DEFLATE_DEVICE) && mrgingham_amd_set_option(R.loader, "tiff_deflate", 1))
            return MRGINGHAM_AMD_ERR_DEVICE;
        const int nslots = nchunks < kRing ? nchunks : kRing;
        const size_t bytes = (size_t)R.batch * max_frame;
        for (int k = 0; k < nslots; ++k) {
            Slot& S = R.slots[k];
            if (hipMalloc(&S.d_raw.p, bytes) != hipSuccess) return MRGINGHAM_AMD_ERR_DEVICE;
            // (a 16-bit chunk always has preprocessed frames: the conversion to 8 bit is part of its preprocessing)
            if ((preprocess || any_deep) && hipMalloc(&S.d_pre.p, bytes) != hipSuccess) return MRGINGHAM_AMD_ERR_DEVICE;
            if (max_host_frame && hipHostMalloc(&S.pin.p, (size_t)R.batch * max_host_frame, hipHostMallocDefault) != hipSuccess)
                return MRGINGHAM_AMD_ERR_DEVICE;
            if (const int fill = R.loader->scratch_fill; fill >= 0) {  // test hook (ctx.h, scratch_fill): the slots are scratch like a context's
                if (hipMemset(S.d_raw.p, fill, bytes) != hipSuccess || (S.d_pre.p && hipMemset(S.d_pre.p, fill, bytes) != hipSuccess) ||
                    hipDeviceSynchronize() != hipSuccess)
                    return MRGINGHAM_AMD_ERR_DEVICE;
                if (S.pin.p) memset(S.pin.p, fill, (size_t)R.batch * max_host_frame);
            }
            if (S.ev_up.create(hipEventDisableTiming) != hipSuccess) return MRGINGHAM_AMD_ERR_DEVICE;
            S.boards.resize((size_t)R.batch * N * 2);
            S.levels.resize((size_t)R.batch * N);
            S.found.resize((size_t)R.batch);
        }
        return 0;
    };
    try {
        rc = setup();
    } catch (...) {
        rc = MRGINGHAM_AMD_ERR_DEVICE;
    }
    if (rc) {
        (void)hipGetLastError();
        cleanup();
        return rc;
    }

    // ---- the calling thread: detector context, one-image path, the prefix of final files
    int nfinal = 0, last_reported = -1;
    std::vector<char> chunk_done((size_t)nchunks, 0);
    long n_one = 0, rerouted_device = 0, rerouted_host = 0;
    Image one_im;
    std::vector<double> one_xy((size_t)N * 2);
    std::vector<signed char> one_lv((size_t)N);
    auto one_image = [&](int i) {
        if (!read_image(filenames[i], one_im)) {
            h_status[i] = -1;
            return;
        }
        ++n_one;
        mrgingham_amd_cli_options co{};
        co.do_clahe = o->do_clahe;
        co.blur_radius = o->blur_radius;
        co.gridn = o->gridn;
        co.image_pyramid_level = o->image_pyramid_level;
        co.do_refine = o->do_refine;
        co.debug_sequence_x = co.debug_sequence_y = -1;
        co.filename = filenames[i];
        const bool deep = one_im.depth == 16;
        const int level = mrgingham_amd_process_image_ex(deep ? (const void*)one_im.px16.data() : (const void*)one_im.px8.data(), deep ? 16 : 8,
                                                         one_im.w, one_im.h, one_im.w, &co, one_xy.data(), one_lv.data());
        if (level < 0) return;  // no board (or an image the one-image path refuses: -2)
        h_found_level[i] = (signed char)level;
        memcpy(h_boards + (size_t)i * N * 2, one_xy.data(), sizeof(double) * 2 * N);
        memcpy(h_levels + (size_t)i * N, one_lv.data(), (size_t)N);
    };
    // files [0, nfinal) are final: moves over rejected files, files of collected chunks and one-image files (processed here)
    auto advance = [&]() {
        for (; nfinal < nfiles; ++nfinal) {
            const int i = nfinal;
            if (h_status[i] != 0) continue;
            if (chunk_of[(size_t)i] >= 0) {
                if (!chunk_done[(size_t)chunk_of[(size_t)i]]) break;
            } else {
                one_image(i);
            }
        }
        if (progress && nfinal != last_reported) progress(nfinal, cookie);
        last_reported = nfinal;
    };
    struct Flight { int chunk, ticket; };
    std::deque<Flight> flight;
    double detector_wait_ms = 0;
    // a chunk the batch entry points refuse (MRGINGHAM_AMD_ERR_ARG) goes through the one-image path, file by file
    auto collect_oldest = [&]() -> int {
        const Flight f = flight.front();
        flight.pop_front();
        const Chunk& ch = R.chunks[(size_t)f.chunk];
        Slot& S = R.slots[f.chunk % kRing];
        if (f.ticket >= 0) {
            const int r = mrgingham_amd_find_boards_collect(R.detector, f.ticket);
            if (r) return r;
        }
        for (size_t k = 0; k < ch.files.size(); ++k) {
            const int i = ch.files[k];
            if (S.load_status[k] != 0) {
                h_status[i] = -1;
                continue;
            }
            if (f.ticket < 0) {  // counted as loaded by the loader: as a one-image file from here on
                --(R.info[(size_t)i].batch_loader() ? rerouted_device : rerouted_host);
                one_image(i);
                continue;
            }
            if (S.found[k] < 0) continue;
            h_found_level[i] = S.found[k];
            memcpy(h_boards + (size_t)i * N * 2, S.boards.data() + k * N * 2, sizeof(double) * 2 * N);
            memcpy(h_levels + (size_t)i * N, S.levels.data() + k * N, (size_t)N);
        }
        chunk_done[(size_t)f.chunk] = 1;
        {
            std::lock_guard<std::mutex> lk(P.mu);
            P.collected = f.chunk + 1;
        }
        P.cv.notify_all();
        advance();
        return 0;
    };
    auto submit = [&](int c) -> int {
        const Chunk& ch = R.chunks[(size_t)c];
        Slot& S = R.slots[c % kRing];
        const int n = (int)ch.files.size();
        const size_t pitch = frame_pitch_of(ch.w, ch.h);
        mrgingham_amd_ctx* ctx = R.detector;
        MRG_HIP_CHECK(hipSetDevice(device));
        if (S.uploaded) MRG_HIP_CHECK(hipStreamWaitEvent(ctx->pix, S.ev_up, 0));
        mrgingham_amd_frames fr{(uint8_t*)S.d_raw.p, (int64_t)pitch, n, ch.w, ch.h, ch.w};
        int r = 0;
        if (ch.bits == 16) {
            // what the one-image path does with a 16-bit image: normalize + CLAHE at 16 bit, convertTo 8 bit, the blur
            r = mrgingham_amd_preprocess16_batch(ctx, (const uint16_t*)S.d_raw.p, (int64_t)pitch, n, ch.w, ch.h, ch.w, o->do_clahe,
                                                 o->blur_radius, (uint8_t*)S.d_pre.p, ctx->pix);
            fr.frames = (uint8_t*)S.d_pre.p;
        } else if (preprocess) {
            // on the pixel stream, like the one-image path: the detector's pixel kernels follow it there
            r = mrgingham_amd_preprocess_batch(ctx, &fr, o->do_clahe, o->blur_radius, (uint8_t*)S.d_pre.p, ctx->pix);
            fr.frames = (uint8_t*)S.d_pre.p;
        }
        int ticket = -1;
        if (!r) {
            ticket = mrgingham_amd_find_boards_submit_ex(ctx, &fr, o->gridn, o->image_pyramid_level, o->do_refine, S.boards.data(),
                                                         S.levels.data(), S.found.data(), R.nthreads);
            if (ticket < 0) r = ticket;
        }
        if (r == MRGINGHAM_AMD_ERR_ARG) {
            r = 0;
            ticket = -1;
        }
        if (r) return r;
        flight.push_back(Flight{c, ticket});
        return 0;
    };
    try {
        if (nchunks > 0) loader_thread = std::thread(loader_main, &R);
        advance();
        for (int c = 0; c < nchunks && !rc; ++c) {
            for (;;) {  // chunk c loaded -- or, while it is not, the oldest job collected
                std::unique_lock<std::mutex> lk(P.mu);
                if (P.failed || P.loaded > c) break;
                if (!flight.empty()) {
                    lk.unlock();
                    if ((rc = collect_oldest())) break;
                    continue;
                }
                const double t0 = now_ms();
                P.cv.wait(lk, [&] { return P.failed || P.loaded > c; });
                detector_wait_ms += now_ms() - t0;
                break;
            }
            if (rc) break;
            {
                std::lock_guard<std::mutex> lk(P.mu);
                if (P.failed) break;
            }
            // as many chunks in flight as the detector context has scratch sets: a further submit would complete the oldest
            // inside the library.  (With three in flight the ring is full and chunk c + 1 cannot load: the loop above then
            // collects instead of waiting, so the two sides never wait for each other.)
            while (!rc && !flight.empty() && (int)flight.size() >= (R.detector->nsets < kRing ? R.detector->nsets : kRing))
                rc = collect_oldest();
            if (!rc) rc = submit(c);
        }
        while (!rc && !flight.empty()) rc = collect_oldest();
    } catch (...) {
        rc = MRGINGHAM_AMD_ERR_DEVICE;
    }
    if (rc) P.fail(rc, R.detector ? mrgingham_amd_last_error(R.detector) : "");
    {
        std::lock_guard<std::mutex> lk(P.mu);
        if (!rc && P.failed) rc = P.failed;
        if (rc && !P.err.empty()) fprintf(stderr, "mrgingham_amd_find_boards_files: %s\n", P.err.c_str());
    }
    st[MRGINGHAM_AMD_FILES_CHUNKS] = (double)nchunks;
    cleanup();  // (joins the loader first: its counters are final below)
    if (rc) return leave(rc);
    long unreadable = 0;
    for (int i = 0; i < nfiles; ++i) unreadable += h_status[i] != 0;
    st[MRGINGHAM_AMD_FILES_DEVICE_LOADED] = (double)(P.n_device_loaded + rerouted_device);
    st[MRGINGHAM_AMD_FILES_HOST_DECODED] = (double)(P.n_host_decoded + rerouted_host);
    st[MRGINGHAM_AMD_FILES_ONE_IMAGE] = (double)n_one;
    st[MRGINGHAM_AMD_FILES_UNREADABLE] = (double)unreadable;
    st[MRGINGHAM_AMD_FILES_DETECTOR_WAIT_MS] = detector_wait_ms;
    st[MRGINGHAM_AMD_FILES_LOADER_WAIT_MS] = P.loader_wait_ms;
    return leave(MRGINGHAM_AMD_OK);
}

}  // namespace

extern "C" {

int mrgingham_amd_find_boards_files(const char* const* filenames, int nfiles, const mrgingham_amd_files_options* o, double* h_boards,
                                    signed char* h_levels, signed char* h_found_level, int32_t* h_status,
                                    void (*progress)(int nfinal, void* cookie), void* cookie, double* stats, int nstats) {
    return find_boards_files(0, filenames, nfiles, o, h_boards, h_levels, h_found_level, h_status, progress, cookie, stats, nstats, 0);
}

// the later entry points differ in the loader flags they accept: each takes the flags that existed when it was added
#define MRG_FILES_ENTRY(name, accepted)                                                                                                \
    int name(const char* const* filenames, int nfiles, const mrgingham_amd_files_options* o, double* h_boards, signed char* h_levels,  \
             signed char* h_found_level, int32_t* h_status, void (*progress)(int nfinal, void* cookie), void* cookie, double* stats,   \
             int nstats, int loader_flags) {                                                                                           \
        return find_boards_files(accepted, filenames, nfiles, o, h_boards, h_levels, h_found_level, h_status, progress, cookie, stats, \
                                 nstats, loader_flags);                                                                                \
    }
MRG_FILES_ENTRY(mrgingham_amd_find_boards_files_ex, kFlagsEx)
MRG_FILES_ENTRY(mrgingham_amd_find_boards_files_ex2, kFlagsEx2)
MRG_FILES_ENTRY(mrgingham_amd_find_boards_files_ex3, kFlagsEx3)
MRG_FILES_ENTRY(mrgingham_amd_find_boards_files_ex4, kFlagsEx4)
MRG_FILES_ENTRY(mrgingham_amd_find_boards_files_ex5, kFlagsEx5)
#undef MRG_FILES_ENTRY

}  // extern "C"
