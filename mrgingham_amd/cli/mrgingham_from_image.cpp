// mrgingham-amd-from-image: the reference's command-line tool (mrgingham-from-image.cc) over
// libmrgingham_amd.so.  Same options, same vnlog output ("# filename x y level", one record per
// corner, "filename - - -" when no board is found), same worker model (--jobs N threads, image i
// goes to worker i % N, mrgingham-from-image.cc:50), same failure behaviour (an unreadable image is
// reported and ends that worker, :58-68).  Row (f)-3 of the scope table: I/O around the hot path.
// --batch N leaves that worker model: the whole list goes through mrgingham_amd_find_boards_files (a loader thread and
// the detector pipelined over chunks of N equally-sized frames, JPEG decoded on the device), records come out in list
// order, and an unreadable image is reported without ending anything.
//
// Image decoding: the reference uses cv::imread; OpenCV is not available to this build, so this
// file reads binary PGM (P5, 8 or 16 bit), non-interlaced PNG (8 or 16 bit; grey, grey+alpha,
// RGB, RGBA, 8-bit palette) with zlib, baseline JPEG (the luma plane), TIFF, Windows Bitmap and binary PBM and PAM (csrc/image_io.h).  Colour is reduced to grey with the fixed-point BT.601
// weights (4899 R + 9617 G + 1868 B + 8192) >> 14 -- OpenCV's own conversion depends on its
// codec build, so byte-identity with cv::imread on colour files is not claimed.
//
// Preprocessing (normalize + CLAHE(8), box blur) and detection run on the GPU through
// mrgingham_amd_process_image_ex, for 8- and 16-bit images alike (16 bit: normalize to 0..65535, CLAHE on
// 16 bits, convertTo(CV_8U, 255/65535), :85-92).
#include <getopt.h>
#include <glob.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "mrgingham_amd.h"
#include "../csrc/image_io.h"

namespace {

using mrg::Image;
using mrg::read_image;

struct Options {
    glob_t globbed;
    int jobs = 1, blur_radius = 1, gridn = 10, level = -1;
    int gpus = 0;  // --gpus: 0 = not given (the library's default: worker k on device k % devices, or MRGINGHAM_AMD_DEVICE)
    bool doclahe = true, do_refine = true, debug = false, doblobs = false;
    int debug_sequence_x = -1, debug_sequence_y = -1;
    int batch = 0;                // --batch N: frames per chunk of mrgingham_amd_find_boards_files; 0 = not given
    bool entropy_device = false;  // --jpeg-entropy device
    bool png_device = false;      // --png-reconstruct device
    bool deep_chunks = false;     // --deep-batch chunks
    bool tiff_device = false;     // --tiff-lzw device
    bool tiff_deflate_device = false;  // --tiff-deflate device
    bool bmp_device = false;      // --bmp-unpack device
    bool pnm_device = false;      // --pnm-unpack device
} opt;

const char* kUsage =
    "Usage: %s [--gridn N] [--noclahe] [--blur radius] [--level l] [--no-refine] [--jobs N]\n"
    "          [--gpus N|all] [--batch N [--jpeg-entropy host|device] [--png-reconstruct host|device]\n"
    "          [--deep-batch one|chunks] [--tiff-lzw host|device [--tiff-deflate host|device]]\n"
    "          [--bmp-unpack host|device] [--pnm-unpack host|device]]\n"
    "          [--debug] [--debug-sequence x,y]\n"
    "          imageglobs...\n"
    "\n"
    "Finds the chessboard in every image (binary PGM, PBM, PAM, PNG, baseline JPEG, strip or tiled TIFF, BMP) and writes a vnlog table\n"
    "\n"
    "  # filename x y level\n"
    "\n"
    "with one record per corner, or 'filename - - -' when no board was found.  The corner\n"
    "candidates, the contrast preprocessing and the refinement run on an AMD GPU\n"
    "(libmrgingham_amd); the options mean what they mean in mrgingham-from-image:\n"
    "\n"
    "  --gridn N       corners per side of the board (default 10)\n"
    "  --noclahe       skip the normalize + CLAHE(8) step\n"
    "  --blur R        box blur radius applied before detection (default 1, 0 = none)\n"
    "  --level L       pyramid level to search at; default -1 = try 3, 2, 1, 0 in turn\n"
    "  --no-refine     keep the corners of the level the board was found at\n"
    "  --jobs N, -j N  worker threads (image i is handled by worker i mod N)\n"
    "  --gpus N|all    GPUs to use: worker k works on device k mod N (default: every GPU of the node,\n"
    "                  or the one named by MRGINGHAM_AMD_DEVICE); --jobs several times the GPU count keeps\n"
    "                  each GPU busy while other workers read and decode\n"
    "  --batch N       the whole list through the batch pipeline, N >= 1 frames per chunk: files of one size are\n"
    "                  loaded in chunks (JPEG decoded on the GPU) while the chunks before them are searched, on one\n"
    "                  GPU; --jobs is the number of host threads.  Records are written in list order.  An unreadable\n"
    "                  image is reported like without --batch, and processing goes on: in this mode no worker stops.\n"
    "                  Not with --debug, --blobs or --gpus above 1\n"
    "  --jpeg-entropy host|device   with --batch: where JPEG files are Huffman-decoded (default host: --jobs threads)\n"
    "  --png-reconstruct host|device   with --batch: where the row filters of PNG files are undone and colour is reduced\n"
    "                  to grey (default host; device: the --jobs threads only inflate)\n"
    "  --deep-batch one|chunks   with --batch: how 16-bit PGM / PNG files are processed (default one: one at a time; chunks:\n"
    "                  in chunks of their own, the byte swap and the 16-bit preprocessing a chunk at a time on the device)\n"
    "  --tiff-lzw host|device   with --batch: where the strips of TIFF files are decoded and their rows reduced to grey\n"
    "                  (default host; device: the --jobs threads only read the files, LZW strips are decoded one lane each)\n"
    "  --tiff-deflate host|device   with --batch and --tiff-lzw device: where the Deflate strips of TIFF files are inflated\n"
    "                  (default host: the --jobs threads; device: one lane per strip)\n"
    "  --bmp-unpack host|device   with --batch: where the rows of BMP files are flipped and unpadded, their indices unpacked,\n"
    "                  the palette looked up and colour reduced to grey (default host; device: the --jobs threads only read\n"
    "                  the files)\n"
    "  --pnm-unpack host|device   with --batch: where the rasters of binary PBM and PAM files are unpacked and colour\n"
    "                  reduced to grey (default host; device: the --jobs threads only read the files)\n"
    "  --blobs         find a grid of dark circles instead of a chessboard (no --level, no refinement)\n"
    "  --debug         one image only: write the preprocessed image, the level images, the ChESS\n"
    "                  responses and the corner vnlogs to /tmp like the reference does\n"
    "  --debug-sequence x,y   accepted (the grid finder's own dumps are not produced)\n";

// At most kDeviceSlots threads per GPU call into the library.  With --jobs up to that many per GPU the workers call it
// themselves; with more, the workers only read, decode and print, and hand their images to kDeviceSlots DEVICE THREADS
// per GPU, asleep on a condition variable while they wait.  More callers per GPU add no throughput (the device is one),
// every caller costs a context (streams, scratch: ~20 ms of start-up each), and every waiting caller spins for the device:
// once they outnumber the cores the spinners burn the time slices of the threads that feed the device (4096 small images
// on 16 cores: 1.4 s with 4 workers, 2-4 s with 16, 10-13 s with 32 before this; decoding PNGs is what more workers are
// for).
constexpr int kDeviceSlots = 8;
struct Request {
    const void* px;
    int depth, w, h;
    const mrgingham_amd_cli_options* o;
    double* xy;
    signed char* lv;
    int level;
    bool done;
    pthread_cond_t cv;
};
struct DeviceQueue {
    pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
    pthread_cond_t work = PTHREAD_COND_INITIALIZER;
    std::vector<Request*> q;  // (a handful of entries: at most one per worker)
    bool stop = false;
    int device = -1;  // -1: wherever the library puts the thread (MRGINGHAM_AMD_DEVICE)
};
std::vector<DeviceQueue> device_queues;  // one per GPU in use (main)
bool hand_off = false;                   // more workers than device slots

int process(const void* px, int depth, int w, int h, const mrgingham_amd_cli_options* o, double* xy, signed char* lv) {
    return mrgingham_amd_process_image_ex(px, depth, w, h, w, o, xy, lv);
}
void* device_thread(void* arg) {
    DeviceQueue& Q = *(DeviceQueue*)arg;
    if (Q.device >= 0) mrgingham_amd_set_thread_device(Q.device);
    pthread_mutex_lock(&Q.mu);
    while (true) {
        while (Q.q.empty() && !Q.stop) pthread_cond_wait(&Q.work, &Q.mu);
        if (Q.q.empty()) break;
        Request* r = Q.q.front();
        Q.q.erase(Q.q.begin());
        pthread_mutex_unlock(&Q.mu);
        const int level = process(r->px, r->depth, r->w, r->h, r->o, r->xy, r->lv);
        pthread_mutex_lock(&Q.mu);
        r->level = level;
        r->done = true;
        pthread_cond_signal(&r->cv);
    }
    pthread_mutex_unlock(&Q.mu);
    return nullptr;
}

void* worker(void* arg) {
    const int ijob = (int)(intptr_t)arg;
    const int N = opt.gridn * opt.gridn;
    std::vector<double> xy((size_t)N * 2);
    std::vector<signed char> lv((size_t)N);
    Image im;  // reused: its buffers keep their pages from image to image
    // worker k works on device k mod N (N = --gpus, or every GPU of the node; MRGINGHAM_AMD_DEVICE pins all to one)
    DeviceQueue& Q = device_queues[(size_t)ijob % device_queues.size()];
    if (!hand_off && Q.device >= 0) mrgingham_amd_set_thread_device(Q.device);
    Request req{};
    if (hand_off) pthread_cond_init(&req.cv, nullptr);
    // the decoded pixels are page-locked where they lie, so that the upload runs at the speed of the link (re-done
    // when an image of another size moves the buffer)
    void* locked = nullptr;
    auto lock_pixels = [&](void* p, size_t bytes) {
        if (p == locked) return;
        if (locked) mrgingham_amd_host_unregister(locked);
        locked = mrgingham_amd_host_register(p, bytes) == 0 ? p : nullptr;
    };
    // a larger image is about to move the pixel buffer: the registration goes first (registered memory must stay allocated
    // until it is unregistered, include/mrgingham_amd.h), then the buffer grows with nothing locked in it
    im.before_grow = [&](size_t n8, size_t n16) {
        if (locked) mrgingham_amd_host_unregister(locked);
        locked = nullptr;
        if (n8 > im.px8.capacity()) im.px8.reserve(n8 + n8 / 8);
        if (n16 > im.px16.capacity()) im.px16.reserve(n16 + n16 / 8);
    };
    // MRGINGHAM_AMD_CLI_TIMING=1: where a worker's time goes (stderr, at its end)
    static const bool timing = getenv("MRGINGHAM_AMD_CLI_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_read = 0, t_proc = 0, t_out = 0;
    int nimg = 0;
    for (int i = ijob; i < (int)opt.globbed.gl_pathc; i += opt.jobs) {
        const char* filename = opt.globbed.gl_pathv[i];
        const double t0 = now();
        if (!read_image(filename, im)) {  // mrgingham-from-image.cc:58-68
            fprintf(stderr, "Couldn't open image '%s'\n", filename);
            flockfile(stdout);
            printf("## Couldn't open image '%s'\n", filename);
            printf("%s - - -\n", filename);
            funlockfile(stdout);
            break;
        }
        mrgingham_amd_cli_options o{};
        o.do_clahe = opt.doclahe;
        o.blur_radius = opt.blur_radius;
        o.gridn = opt.gridn;
        o.image_pyramid_level = opt.level;
        o.do_refine = opt.do_refine;
        o.do_blobs = opt.doblobs;
        o.debug = opt.debug;
        o.debug_sequence_x = opt.debug_sequence_x;
        o.debug_sequence_y = opt.debug_sequence_y;
        o.filename = filename;
        if (im.depth == 16) lock_pixels(im.px16.data(), im.px16.capacity() * 2);
        else lock_pixels(im.px8.data(), im.px8.capacity());
        const double t1 = now();
        // 8- and 16-bit images go to the device as they are (mrgingham-from-image.cc:71-92)
        const void* px = im.depth == 16 ? (const void*)im.px16.data() : (const void*)im.px8.data();
        int level;
        if (!hand_off) {
            level = process(px, im.depth == 16 ? 16 : 8, im.w, im.h, &o, xy.data(), lv.data());
        } else {
            req.px = px; req.depth = im.depth == 16 ? 16 : 8; req.w = im.w; req.h = im.h;
            req.o = &o; req.xy = xy.data(); req.lv = lv.data(); req.done = false;
            pthread_mutex_lock(&Q.mu);
            Q.q.push_back(&req);
            pthread_cond_signal(&Q.work);
            while (!req.done) pthread_cond_wait(&req.cv, &Q.mu);
            pthread_mutex_unlock(&Q.mu);
            level = req.level;
        }
        const double t2 = now();
        flockfile(stdout);
        if (level >= 0)  // mrgingham-from-image.cc:174-183
            for (int k = 0; k < N; ++k)
                printf("%s %f %f %d\n", filename, xy[2 * k], xy[2 * k + 1], (opt.do_refine && !opt.doblobs) ? (int)lv[k] : level);
        else
            printf("%s - - -\n", filename);
        funlockfile(stdout);
        t_read += t1 - t0; t_proc += t2 - t1; t_out += now() - t2; ++nimg;
    }
    if (timing && nimg)
        fprintf(stderr, "worker %d: %d images; per image: read + decode %.3f ms, upload + device + grid finder %.3f ms, output %.3f ms\n",
                ijob, nimg, t_read / nimg, t_proc / nimg, t_out / nimg);
    if (locked) mrgingham_amd_host_unregister(locked);
    if (hand_off) pthread_cond_destroy(&req.cv);
    return nullptr;
}

// --batch: records of the files [printed, nfinal), in list order, as the prefix of final files grows
struct BatchOut {
    std::vector<double> xy;
    std::vector<signed char> lv, found;
    std::vector<int32_t> status;
    int printed = 0;
};
void batch_progress(int nfinal, void* cookie) {
    BatchOut& B = *(BatchOut*)cookie;
    const int N = opt.gridn * opt.gridn;
    flockfile(stdout);
    for (; B.printed < nfinal; ++B.printed) {
        const int i = B.printed;
        const char* filename = opt.globbed.gl_pathv[i];
        if (B.status[(size_t)i] != 0) {  // mrgingham-from-image.cc:58-68
            fprintf(stderr, "Couldn't open image '%s'\n", filename);
            printf("## Couldn't open image '%s'\n", filename);
            printf("%s - - -\n", filename);
            continue;
        }
        const int level = B.found[(size_t)i];
        if (level >= 0)
            for (int k = 0; k < N; ++k)
                printf("%s %f %f %d\n", filename, B.xy[((size_t)i * N + k) * 2], B.xy[((size_t)i * N + k) * 2 + 1],
                       opt.do_refine ? (int)B.lv[(size_t)i * N + k] : level);
        else
            printf("%s - - -\n", filename);
    }
    funlockfile(stdout);
}
int run_batch() {
    const size_t n = opt.globbed.gl_pathc, N = (size_t)opt.gridn * opt.gridn;
    BatchOut B;
    B.xy.resize(n * N * 2);
    B.lv.resize(n * N);
    B.found.resize(n);
    B.status.resize(n);
    mrgingham_amd_files_options o{};
    o.do_clahe = opt.doclahe;
    o.blur_radius = opt.blur_radius;
    o.gridn = opt.gridn;
    o.image_pyramid_level = opt.level;
    o.do_refine = opt.do_refine;
    o.batch_frames = opt.batch;
    o.nthreads = opt.jobs;
    o.jpeg_entropy = opt.entropy_device;
    o.device = -1;
    double stats[MRGINGHAM_AMD_FILES_STATS] = {};
    const int rc = mrgingham_amd_find_boards_files_ex5(opt.globbed.gl_pathv, (int)n, &o, B.xy.data(), B.lv.data(), B.found.data(),
                                                       B.status.data(), batch_progress, &B, stats, MRGINGHAM_AMD_FILES_STATS,
                                                       (opt.png_device ? MRGINGHAM_AMD_FILES_PNG_DEVICE : 0) |
                                                           (opt.deep_chunks ? MRGINGHAM_AMD_FILES_DEEP_CHUNKS : 0) |
                                                           (opt.tiff_device ? MRGINGHAM_AMD_FILES_TIFF_DEVICE : 0) |
                                                           (opt.tiff_deflate_device ? MRGINGHAM_AMD_FILES_TIFF_DEFLATE_DEVICE : 0) |
                                                           (opt.bmp_device ? MRGINGHAM_AMD_FILES_BMP_DEVICE : 0) |
                                                           (opt.pnm_device ? MRGINGHAM_AMD_FILES_PNM_DEVICE : 0));
    fflush(stdout);
    if (getenv("MRGINGHAM_AMD_CLI_TIMING"))
        fprintf(stderr, "batch: %.0f chunks; files: %.0f device loader, %.0f host-decoded, %.0f one at a time, %.0f unreadable; "
                        "detector waited %.1f ms for chunks, loader waited %.1f ms for ring slots\n",
                stats[0], stats[1], stats[2], stats[3], stats[4], stats[5], stats[6]);
    if (rc != 0) {
        fprintf(stderr, "mrgingham-amd-from-image: the batch pipeline failed (%d)\n", rc);
        return 2;
    }
    return 0;
}

}  // namespace

int main(int argc, char* argv[]) {
    static const struct option longopts[] = {
        {"blobs", no_argument, nullptr, 'B'},          {"blur", required_argument, nullptr, 'b'},
        {"noclahe", no_argument, nullptr, 'C'},        {"level", required_argument, nullptr, 'l'},
        {"no-refine", no_argument, nullptr, 'R'},      {"jobs", required_argument, nullptr, 'j'},
        {"gridn", required_argument, nullptr, 'N'},    {"debug", no_argument, nullptr, 'd'},
        {"debug-sequence", required_argument, nullptr, 'D'}, {"help", no_argument, nullptr, 'h'},
        {"gpus", required_argument, nullptr, 'G'},     {"batch", required_argument, nullptr, 'T'},
        {"jpeg-entropy", required_argument, nullptr, 'E'},
        {"png-reconstruct", required_argument, nullptr, 'P'},
        {"deep-batch", required_argument, nullptr, 'Q'},
        {"tiff-lzw", required_argument, nullptr, 'Z'},
        {"tiff-deflate", required_argument, nullptr, 'Y'},
        {"bmp-unpack", required_argument, nullptr, 'M'},
        {"pnm-unpack", required_argument, nullptr, 'U'},
        {nullptr, 0, nullptr, 0}};
    bool doblobs = false, entropy_given = false, png_given = false, deep_given = false, tiff_given = false, deflate_given = false, bmp_given = false, pnm_given = false;
    int c;
    while ((c = getopt_long(argc, argv, "hj:b:l:", longopts, nullptr)) != -1) {
        switch (c) {
            case 'h': printf(kUsage, argv[0]); return 0;
            case 'B': doblobs = true; break;
            case 'C': opt.doclahe = false; break;
            case 'R': opt.do_refine = false; break;
            case 'd': opt.debug = true; break;
            case 'D': {
                int x, y;
                if (sscanf(optarg, "%d,%d", &x, &y) != 2) {
                    fprintf(stderr, "I could not parse 'x,y' from --debug-sequence '%s'. Giving up\n", optarg);
                    fprintf(stderr, kUsage, argv[0]);
                    return -1;
                }
                opt.debug_sequence_x = x;
                opt.debug_sequence_y = y;
                break;
            }
            case 'N': opt.gridn = atoi(optarg); break;
            case 'b': opt.blur_radius = atoi(optarg); break;
            case 'l': opt.level = atoi(optarg); break;
            case 'j': opt.jobs = atoi(optarg); break;
            case 'G': opt.gpus = !strcmp(optarg, "all") ? -1 : atoi(optarg); if (opt.gpus == 0) opt.gpus = -2; break;
            case 'T': {
                char* end = nullptr;
                const long v = strtol(optarg, &end, 10);
                if (end == optarg || *end || v < 1 || v > 1 << 20) {
                    fprintf(stderr, "--batch takes a positive frame count, got '%s'\n", optarg);
                    fprintf(stderr, kUsage, argv[0]);
                    return 1;
                }
                opt.batch = (int)v;
                break;
            }
            case 'E':
                if (strcmp(optarg, "host") && strcmp(optarg, "device")) {
                    fprintf(stderr, "--jpeg-entropy takes 'host' or 'device', got '%s'\n", optarg);
                    fprintf(stderr, kUsage, argv[0]);
                    return 1;
                }
                entropy_given = true;
                opt.entropy_device = !strcmp(optarg, "device");
                break;
            case 'P':
                if (strcmp(optarg, "host") && strcmp(optarg, "device")) {
                    fprintf(stderr, "--png-reconstruct takes 'host' or 'device', got '%s'\n", optarg);
                    fprintf(stderr, kUsage, argv[0]);
                    return 1;
                }
                png_given = true;
                opt.png_device = !strcmp(optarg, "device");
                break;
            case 'Q':
                if (strcmp(optarg, "one") && strcmp(optarg, "chunks")) {
                    fprintf(stderr, "--deep-batch takes 'one' or 'chunks', got '%s'\n", optarg);
                    fprintf(stderr, kUsage, argv[0]);
                    return 1;
                }
                deep_given = true;
                opt.deep_chunks = !strcmp(optarg, "chunks");
                break;
            case 'Z':
                if (strcmp(optarg, "host") && strcmp(optarg, "device")) {
                    fprintf(stderr, "--tiff-lzw takes 'host' or 'device', got '%s'\n", optarg);
                    fprintf(stderr, kUsage, argv[0]);
                    return 1;
                }
                tiff_given = true;
                opt.tiff_device = !strcmp(optarg, "device");
                break;
            case 'Y':
                if (strcmp(optarg, "host") && strcmp(optarg, "device")) {
                    fprintf(stderr, "--tiff-deflate takes 'host' or 'device', got '%s'\n", optarg);
                    fprintf(stderr, kUsage, argv[0]);
                    return 1;
                }
                deflate_given = true;
                opt.tiff_deflate_device = !strcmp(optarg, "device");
                break;
            case 'M':
                if (strcmp(optarg, "host") && strcmp(optarg, "device")) {
                    fprintf(stderr, "--bmp-unpack takes 'host' or 'device', got '%s'\n", optarg);
                    fprintf(stderr, kUsage, argv[0]);
                    return 1;
                }
                bmp_given = true;
                opt.bmp_device = !strcmp(optarg, "device");
                break;
            case 'U':
                if (strcmp(optarg, "host") && strcmp(optarg, "device")) {
                    fprintf(stderr, "--pnm-unpack takes 'host' or 'device', got '%s'\n", optarg);
                    fprintf(stderr, kUsage, argv[0]);
                    return 1;
                }
                pnm_given = true;
                opt.pnm_device = !strcmp(optarg, "device");
                break;
            default:
                fprintf(stderr, "Unknown option\n");
                fprintf(stderr, kUsage, argv[0]);
                return 1;
        }
    }
    if (entropy_given && !opt.batch) {
        fprintf(stderr, "--jpeg-entropy is only accepted with --batch\n");
        return 1;
    }
    if (png_given && !opt.batch) {
        fprintf(stderr, "--png-reconstruct is only accepted with --batch\n");
        return 1;
    }
    if (deep_given && !opt.batch) {
        fprintf(stderr, "--deep-batch is only accepted with --batch\n");
        return 1;
    }
    if (tiff_given && !opt.batch) {
        fprintf(stderr, "--tiff-lzw is only accepted with --batch\n");
        return 1;
    }
    if (deflate_given && !opt.batch) {
        fprintf(stderr, "--tiff-deflate is only accepted with --batch\n");
        return 1;
    }
    if (bmp_given && !opt.batch) {
        fprintf(stderr, "--bmp-unpack is only accepted with --batch\n");
        return 1;
    }
    if (pnm_given && !opt.batch) {
        fprintf(stderr, "--pnm-unpack is only accepted with --batch\n");
        return 1;
    }
    if (opt.tiff_deflate_device && !opt.tiff_device) {
        fprintf(stderr, "--tiff-deflate device is only accepted with --tiff-lzw device\n");
        return 1;
    }
    if (opt.batch && (opt.debug || doblobs || opt.gpus > 1 || opt.gpus == -1)) {
        fprintf(stderr, "--batch works on one GPU (no --gpus above 1, no --gpus all) and has neither --debug nor --blobs\n");
        return 1;
    }
    if (optind > argc - 1) {
        fprintf(stderr, "Not enough arguments: need image globs\n");
        fprintf(stderr, kUsage, argv[0]);
        return 1;
    }
    if (opt.jobs <= 0) {
        fprintf(stderr, "The job count must be a positive integer\n");
        fprintf(stderr, kUsage, argv[0]);
        return 1;
    }
    if (doblobs && opt.level >= 0) {  // mrgingham-from-image.cc:305-309
        fprintf(stderr, "ERROR: 'image_pyramid_level' only implemented for chessboards.\n");
        return 1;
    }
    opt.doblobs = doblobs;
    if (doblobs) opt.level = 0;
    if (opt.gridn < 2) {
        fprintf(stderr, "--gridn value must be >= 2\n");
        return 1;
    }
    if (opt.blur_radius < 0) {
        fprintf(stderr, "--blur value must be >= 0\n");
        return 1;
    }
    int append = 0;
    for (int i = optind; i < argc; ++i) {
        const int r = glob(argv[i], append | GLOB_ERR | GLOB_MARK | GLOB_NOSORT | GLOB_TILDE_CHECK, nullptr, &opt.globbed);
        if (r == GLOB_NOMATCH) { fprintf(stderr, "'%s' matched no files!\n", argv[i]); return 1; }
        if (r != 0) { fprintf(stderr, "globbing '%s' failed!\n", argv[i]); return 1; }
        append = GLOB_APPEND;
    }
    if (opt.debug && opt.globbed.gl_pathc != 1) {
        fprintf(stderr, "When debugging, pass one image at a time. Got %d instead\n", (int)opt.globbed.gl_pathc);
        return 1;
    }
    const int ndev = mrgingham_amd_device_count();
    if (ndev <= 0) {
        fprintf(stderr, "mrgingham-amd-from-image: no HIP device: this tool has no CPU path\n");
        return 2;
    }
    if (opt.gpus == -2 || opt.gpus < -2) {
        fprintf(stderr, "--gpus takes a positive count or 'all'\n");
        return 1;
    }
    if (opt.gpus == -1) opt.gpus = ndev;
    if (opt.gpus > ndev) {
        fprintf(stderr, "mrgingham-amd-from-image: --gpus %d, but this node has %d: using %d\n", opt.gpus, ndev, ndev);
        opt.gpus = ndev;
    }
    printf("## generated with");
    for (int i = 0; i < argc; ++i) printf(" %s", argv[i]);
    printf("\n# filename x y level\n");
    fflush(stdout);
    if (opt.batch) {
        const int rc = run_batch();
        globfree(&opt.globbed);
        return rc;
    }
    const bool pinned_by_env = getenv("MRGINGHAM_AMD_DEVICE") != nullptr && opt.gpus <= 0;
    const int ng = opt.gpus > 0 ? opt.gpus : (pinned_by_env ? 1 : ndev);
    device_queues = std::vector<DeviceQueue>((size_t)ng);
    for (int d = 0; d < ng; ++d) device_queues[(size_t)d].device = pinned_by_env ? -1 : d;
    hand_off = opt.jobs > kDeviceSlots * ng;
    std::vector<pthread_t> dth;
    if (hand_off) {
        dth.resize((size_t)kDeviceSlots * ng);
        for (size_t i = 0; i < dth.size(); ++i) pthread_create(&dth[i], nullptr, device_thread, &device_queues[i % (size_t)ng]);
    }
    std::vector<pthread_t> th((size_t)opt.jobs);
    for (int i = 0; i < opt.jobs; ++i) pthread_create(&th[i], nullptr, worker, (void*)(intptr_t)i);
    for (int i = 0; i < opt.jobs; ++i) pthread_join(th[i], nullptr);
    for (DeviceQueue& Q : device_queues) {
        pthread_mutex_lock(&Q.mu);
        Q.stop = true;
        pthread_cond_broadcast(&Q.work);
        pthread_mutex_unlock(&Q.mu);
    }
    for (pthread_t& t : dth) pthread_join(t, nullptr);
    globfree(&opt.globbed);
    return 0;
}
