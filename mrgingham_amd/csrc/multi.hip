// Host side of libmrgingham_amd.so over several devices: the shards of a batch (shard_range), chain_batch over one
// context per shard with the corner lists gathered on the first context's device (chain_multi), the packed layout and the
// ncclGather of a process-per-GPU host (gather_rccl), and the waits for all of it (sync_multi, stream_wait_multi).
#include <dlfcn.h>

#include "ctx.h"

using namespace mrg;

extern "C" {

int mrgingham_amd_shard_range(int total, int k, int n, int* first, int* count) {
    if (total < 0 || n <= 0 || k < 0 || k >= n || !first || !count) return MRGINGHAM_AMD_ERR_ARG;
    const int q = total / n, r = total % n;  // the first r shards take one frame more
    *first = k * q + (k < r ? k : r);
    *count = q + (k < r ? 1 : 0);
    return MRGINGHAM_AMD_OK;
}

// One shard of mrgingham_amd_chain_multi: the chain on its context and, for a shard that is not on the root device, the
// copy of its block to the root behind it.  Runs on the context's submit thread (or on the caller for a single shard).
static int chain_multi_shard(mrgingham_amd_ctx* ctx, int root_device, const mrgingham_amd_frames* shard, int start_level,
                             double* dst_p, signed char* dst_l, int32_t* dst_n, int points_pitch) {
    const int B = shard->nframes;
    const size_t np = (size_t)B * points_pitch;
    int rc;
    if (ctx->device == root_device) {
        if ((rc = mrgingham_amd_chain_batch(ctx, shard, start_level, dst_p, dst_l, dst_n, points_pitch))) return rc;
        ctx->mg_pending = false;
        return MRGINGHAM_AMD_OK;
    }
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    if (!ctx->mg_stream) {
        MRG_HIP_CHECK(hipStreamCreateWithFlags(&ctx->mg_stream.h, hipStreamNonBlocking));
        MRG_HIP_CHECK(ctx->mg_done.create(hipEventDisableTiming));
        int can = 0;  // direct peer copies where the link allows them (otherwise HIP stages through the host)
        if (hipDeviceCanAccessPeer(&can, ctx->device, root_device) == hipSuccess && can) {
            hipError_t e = hipDeviceEnablePeerAccess(root_device, 0);
            if (e != hipSuccess) (void)hipGetLastError();  // (already enabled, or refused: the copy still works)
        }
    }
    if ((rc = ensure(ctx, ctx->mg_pts, np * 16)) || (rc = ensure(ctx, ctx->mg_lv, np)) || (rc = ensure(ctx, ctx->mg_np, (size_t)B * 4)))
        return rc;
    if (ctx->mg_pending) MRG_HIP_CHECK(hipStreamWaitEvent(ctx->pix, ctx->mg_done, 0));  // the gather before this one has read the buffers
    if ((rc = mrgingham_amd_chain_batch(ctx, shard, start_level, (double*)ctx->mg_pts.p, (signed char*)ctx->mg_lv.p,
                                        (int32_t*)ctx->mg_np.p, points_pitch)))
        return rc;
    if ((rc = mrgingham_amd_stream_wait(ctx, ctx->mg_stream))) return rc;
    MRG_HIP_CHECK(hipMemcpyPeerAsync(dst_p, root_device, ctx->mg_pts.p, ctx->device, np * 16, ctx->mg_stream));
    MRG_HIP_CHECK(hipMemcpyPeerAsync(dst_l, root_device, ctx->mg_lv.p, ctx->device, np, ctx->mg_stream));
    MRG_HIP_CHECK(hipMemcpyPeerAsync(dst_n, root_device, ctx->mg_np.p, ctx->device, (size_t)B * 4, ctx->mg_stream));
    MRG_HIP_CHECK(hipEventRecord(ctx->mg_done, ctx->mg_stream));
    ctx->mg_pending = true;
    return MRGINGHAM_AMD_OK;
}

/* chain_batch over several contexts -- one per device of a node, or several on one -- in ONE call: context k takes
 * shards[k] (frames in the memory of ITS device), and the corner lists of every shard arrive in d_points / d_levels /
 * d_npoints, buffers on the device of ctxs[0] laid out for the sum of the shards' frames in shard order (frame-major):
 * a shard on that device writes its block in place, a shard elsewhere writes into its own context's buffers and the
 * block travels device to device behind its chain (hipMemcpyPeerAsync: xGMI between the GPUs of a node) -- the ONE
 * exchange of the path.  Asynchronous; mrgingham_amd_sync_multi waits for everything.
 * Every shard is queued by a submit thread of its own context, all at once (queueing one chain costs the host ~70 us:
 * eight of them from one thread would be 0.56 ms per call, more than a sparse step takes on the device); the call returns
 * when all of them are queued. */
int mrgingham_amd_chain_multi(mrgingham_amd_ctx* const* ctxs, int nctx, const mrgingham_amd_frames* shards, int start_level,
                              double* d_points, signed char* d_levels, int32_t* d_npoints, int points_pitch) {
    if (!ctxs || nctx <= 0 || !shards || !ctxs[0]) return MRGINGHAM_AMD_ERR_ARG;
    const CallerDevice keep;  // (the shards' contexts live on several devices: the caller's current one is put back)
    mrgingham_amd_ctx* root = ctxs[0];
    if (!d_points || !d_levels || !d_npoints || points_pitch <= 0)
        return fail(root, MRGINGHAM_AMD_ERR_ARG, "NULL point buffers");
    for (int k = 0; k < nctx; ++k) {
        if (!ctxs[k]) return fail(root, MRGINGHAM_AMD_ERR_ARG, "NULL context %d", k);
        for (int j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return fail(root, MRGINGHAM_AMD_ERR_ARG, "context %d is context %d again: one context per shard", k, j);
    }
    int nwork = 0;
    for (int k = 0; k < nctx; ++k) {
        const int rc = validate_frames(ctxs[k], &shards[k]);
        if (rc) return rc;
        nwork += shards[k].nframes > 0;
    }
    std::vector<int> rcs((size_t)nctx, MRGINGHAM_AMD_OK);
    std::vector<char> started((size_t)nctx, 0);
    const int root_device = root->device;
    size_t off = 0;  // frames in front of shard k
    for (int k = 0; k < nctx; ++k) {
        mrgingham_amd_ctx* ctx = ctxs[k];
        const int B = shards[k].nframes;
        if (B == 0) continue;
        double* dst_p = d_points + off * points_pitch * 2;
        signed char* dst_l = d_levels + off * points_pitch;
        int32_t* dst_n = d_npoints + off;
        off += (size_t)B;
        const mrgingham_amd_frames* sh = &shards[k];
        int* out = &rcs[(size_t)k];
        if (nwork == 1) {
            *out = chain_multi_shard(ctx, root_device, sh, start_level, dst_p, dst_l, dst_n, points_pitch);
        } else {
            ctx->submit_pool.start(1, [=] { *out = chain_multi_shard(ctx, root_device, sh, start_level, dst_p, dst_l, dst_n, points_pitch); });
            started[(size_t)k] = 1;
        }
    }
    int rc = MRGINGHAM_AMD_OK;
    for (int k = 0; k < nctx; ++k) {
        if (started[(size_t)k]) ctxs[k]->submit_pool.wait();
        if (rcs[(size_t)k] && !rc) rc = rcs[(size_t)k];
    }
    (void)hipSetDevice(root_device);
    return rc;
}

int mrgingham_amd_packed_layout(int nframes, int points_pitch, size_t* off_levels, size_t* off_npoints, size_t* bytes) {
    if (nframes < 0 || points_pitch <= 0) return MRGINGHAM_AMD_ERR_ARG;
    const size_t np = (size_t)nframes * points_pitch;
    const size_t o_lv = np * 16, o_np = (o_lv + np + 7) / 8 * 8;
    if (off_levels) *off_levels = o_lv;
    if (off_npoints) *off_npoints = o_np;
    if (bytes) *bytes = (o_np + (size_t)nframes * 4 + 7) / 8 * 8;  // (a multiple of 8: rank blocks of the gathered buffer stay aligned)
    return MRGINGHAM_AMD_OK;
}

/* The one exchange of the path for a host that runs ONE PROCESS PER GPU (rccl.h:745): ncclGather of this
 * rank's packed corner lists to `root`, on `stream`, behind the context's most recent call.  RCCL is not linked: the
 * communicator was made by the RCCL the host process runs on, and its ncclGather is the one that has to be called -- looked
 * up in the process (dlsym), then in librccl.so.1 / librccl.so. */
int mrgingham_amd_gather_rccl(mrgingham_amd_ctx* ctx, void* nccl_comm, int root, const void* d_packed, size_t bytes,
                              void* d_gathered, void* stream) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    if (!nccl_comm || !d_packed || bytes == 0 || root < 0) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "gather_rccl: NULL communicator / buffer, or nothing to send");
    // RCCL's ncclGather, looked up in the copy of RCCL the HOST has loaded (the one that made `nccl_comm`): no header and no
    // link dependency, and never a second copy -- a communicator handed to another instance of the library is undefined
    // behaviour.  First among the global symbols (a C host linked with -lrccl), then in an already-loaded librccl that was
    // opened RTLD_LOCAL (Python / PyTorch's bundled copy): dlopen(RTLD_NOLOAD) finds it without loading anything.  A
    // failed lookup is not remembered (the host may load RCCL later).
    using gather_fn = int (*)(const void*, void*, size_t, int /* ncclDataType_t */, int, void* /* ncclComm_t */, hipStream_t);
    using errstr_fn = const char* (*)(int);
    constexpr int kNcclSuccess = 0, kNcclUint8 = 1;  // nccl.h: ncclSuccess, ncclUint8 (stable since NCCL 2.0)
    static std::atomic<gather_fn> gather_cached{nullptr};
    static std::atomic<errstr_fn> errstr_cached{nullptr};
    gather_fn gather = gather_cached.load(std::memory_order_acquire);
    if (!gather) {
        void* f = dlsym(RTLD_DEFAULT, "ncclGather");
        void* e = dlsym(RTLD_DEFAULT, "ncclGetErrorString");
        if (!f)
            for (const char* name : {"librccl.so.1", "librccl.so"}) {
                void* h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
                if (h && (f = dlsym(h, "ncclGather"))) {
                    e = dlsym(h, "ncclGetErrorString");
                    break;  // (the handle is kept: the library stays mapped as long as this one uses its function)
                }
                if (h) dlclose(h);
            }
        if (!f)
            return fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "gather_rccl: RCCL is not loaded in this process (no ncclGather among the global symbols, "
                                                       "no librccl.so mapped): the host that made the communicator must have it loaded");
        gather = (gather_fn)f;
        errstr_cached.store((errstr_fn)e, std::memory_order_release);
        gather_cached.store(gather, std::memory_order_release);
    }
    const errstr_fn errstr = errstr_cached.load(std::memory_order_acquire);
    const CallerDevice keep;  // (the caller's current device is put back)
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    const int rc = mrgingham_amd_stream_wait(ctx, stream);  // the gather starts behind the chain that fills d_packed, on the device
    if (rc) return rc;
    const int r = gather(d_packed, d_gathered, bytes, kNcclUint8, root, nccl_comm, (hipStream_t)stream);
    if (r != kNcclSuccess)
        return fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "ncclGather failed: %s", errstr ? errstr(r) : "(no error text)");
    return MRGINGHAM_AMD_OK;
}

int mrgingham_amd_sync_multi(mrgingham_amd_ctx* const* ctxs, int nctx) {
    if (!ctxs || nctx <= 0) return MRGINGHAM_AMD_ERR_ARG;
    const CallerDevice keep;  // (the contexts live on several devices: the caller's current one is put back)
    int rc = MRGINGHAM_AMD_OK;
    for (int k = 0; k < nctx; ++k) {
        mrgingham_amd_ctx* ctx = ctxs[k];
        if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
        const int r = mrgingham_amd_sync(ctx);
        if (r && !rc) rc = r;
        if (ctx->mg_stream) {
            MRG_HIP_CHECK(hipSetDevice(ctx->device));
            MRG_HIP_CHECK(hipStreamSynchronize(ctx->mg_stream));
        }
        ctx->mg_pending = false;
    }
    return rc;
}

/* Device-side alternative to mrgingham_amd_sync_multi: `stream` (a hipStream_t of any device, normally the first
 * context's) waits for the chains and the gathers of the most recent mrgingham_amd_chain_multi. */
int mrgingham_amd_stream_wait_multi(mrgingham_amd_ctx* const* ctxs, int nctx, void* stream) {
    if (!ctxs || nctx <= 0) return MRGINGHAM_AMD_ERR_ARG;
    const CallerDevice keep;
    for (int k = 0; k < nctx; ++k) {
        mrgingham_amd_ctx* ctx = ctxs[k];
        if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
        if (ctx->mg_pending) {
            MRG_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, ctx->mg_done, 0));
        } else {
            const int r = mrgingham_amd_stream_wait(ctx, stream);
            if (r) return r;
        }
    }
    return MRGINGHAM_AMD_OK;
}
}  // extern "C"
