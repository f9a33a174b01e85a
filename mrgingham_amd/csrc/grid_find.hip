// The grid finder on the device: candidate lists that lie in device memory to board indices, one workgroup of 256 lanes
// per list, one launch per call.  The phases are grid_phases.h, the text the host model (grid_model.cpp:
// mrgingham_amd_find_grids_host) runs serially; this file is the executor, the launch and the entry points.  See
// include/mrgingham_amd.h for the contract, DESIGN.md section 4.25 for the phases, the decline rule, the guard band
// and the kernel's footprint.
#include "ctx.h"

#include "grid_phases.h"

using namespace mrg;

namespace mrg {

constexpr int kGfMaxSlots = 256;  // workgroups of a launch, each with a slot of scratch: one per CU; more lists take turns
constexpr int kGfStatWords = 8;   // lists, found, none, declined -1 .. -5

struct DeviceLanes {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int lanes() const { return kGfLanes; }
    __device__ __forceinline__ void barrier() const { __syncthreads(); }
    __device__ __forceinline__ void lower(int32_t* word, int value) const { atomicMin(word, value); }
};

// blockIdx.x = slot; the slot's lists are slot, slot + gridDim.x, ...
__global__ __launch_bounds__(kGfLanes) void find_grids_kernel(const int32_t* __restrict__ xy, const int32_t* __restrict__ counts, int nlists,
                                                              int capacity, int gridn, int guard_bits, GfFar* __restrict__ slots,
                                                              int32_t* __restrict__ index, int32_t* __restrict__ status,
                                                              unsigned long long* __restrict__ stats) {
    __shared__ GfNear s;
    DeviceLanes x;
    GfFar& g = slots[blockIdx.x];
    for (int l = (int)blockIdx.x; l < nlists; l += (int)gridDim.x) {
        const int st = gf_find_grid(x, s, g, xy + (size_t)l * capacity * 2, counts[l], capacity, gridn, guard_bits,
                                    index + (size_t)l * gridn * gridn);
        if (threadIdx.x == 0) {
            status[l] = st;
            atomicAdd(&stats[0], 1ull);
            if (st <= kGfFound && st >= kGfDeclineCoord) atomicAdd(&stats[2 - st], 1ull);  // 1 found, 2 none, 3 .. 7 declined -1 .. -5
        }  // (gf_find_grid ends behind a barrier: the next list's first phase writes nothing a lane of this one still reads)
    }
}

// the launch of find_grids_batch and of the pipelined find_boards, on stream s; scratch: the slots of scratch set `set`
int ensure_find_grids(mrgingham_amd_ctx* ctx, int set, int nlists) {
    int rc;
    const int slots = nlists < kGfMaxSlots ? nlists : kGfMaxSlots;
    if ((rc = ensure(ctx, ctx->grid_slots[set], (size_t)slots * sizeof(GfFar)))) return rc;
    if (!ctx->grid_stat.p) {  // STATE (ctx.h, scratch_fill): counters that add up until mrgingham_amd_find_grids_stats reads them
        if ((rc = ensure(ctx, ctx->grid_stat, kGfStatWords * sizeof(unsigned long long)))) return rc;
        MRG_HIP_CHECK(hipMemset(ctx->grid_stat.p, 0, ctx->grid_stat.bytes));
    }
    return 0;
}

int launch_find_grids(mrgingham_amd_ctx* ctx, int set, const int32_t* d_xy, const int32_t* d_counts, int nlists, int capacity, int gridn,
                      int32_t* d_index, int32_t* d_status, hipStream_t s) {
    const int slots = nlists < kGfMaxSlots ? nlists : kGfMaxSlots;
    if (int rc = ensure_find_grids(ctx, set, nlists)) return rc;
    hipLaunchKernelGGL(find_grids_kernel, dim3((unsigned)slots), dim3(kGfLanes), 0, s, d_xy, d_counts, nlists, capacity, gridn,
                       ctx->find_grids_guard_bits, (GfFar*)ctx->grid_slots[set].p, d_index, d_status, (unsigned long long*)ctx->grid_stat.p);
    MRG_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace mrg

extern "C" {

void mrgingham_amd_find_grids_geometry(int* lanes_per_workgroup, int* max_candidates, int* min_gridn, int* max_gridn, int* max_workgroups,
                                       int64_t* scratch_bytes_per_workgroup) {
    if (lanes_per_workgroup) *lanes_per_workgroup = kGfLanes;
    if (max_candidates) *max_candidates = kGfMaxSites;
    if (min_gridn) *min_gridn = kGfMinGridn;
    if (max_gridn) *max_gridn = kGfMaxGridn;
    if (max_workgroups) *max_workgroups = kGfMaxSlots;
    if (scratch_bytes_per_workgroup) *scratch_bytes_per_workgroup = (int64_t)sizeof(GfFar);
}

int mrgingham_amd_find_grids_batch(mrgingham_amd_ctx* ctx, const int32_t* d_xy, const int32_t* d_counts, int nlists, int capacity, int gridn,
                                   int32_t* d_index, int32_t* d_status) {
    if (!ctx) return MRGINGHAM_AMD_ERR_ARG;
    fb_drain(ctx);
    if (gridn < kGfMinGridn || gridn > kGfMaxGridn) return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "find_grids: gridn %d .. %d", kGfMinGridn, kGfMaxGridn);
    if (nlists < 0 || capacity < 0 || capacity > (1 << 24) || (nlists > 0 && (!d_counts || !d_index || !d_status || (capacity > 0 && !d_xy))))
        return fail(ctx, MRGINGHAM_AMD_ERR_ARG, "bad candidate list batch descriptor");
    if (nlists == 0) return 0;
    MRG_HIP_CHECK(hipSetDevice(ctx->device));
    if (int rc = ensure_find_grids(ctx, (ctx->cur + 1) % ctx->nsets, nlists)) return rc;  // (in front of the rotation: a failure leaves the context as it was)
    // an op of its own: the next scratch set, behind whatever the pixel stream has been told to wait for
    // (mrgingham_amd_after_stream) and behind the earlier calls that touch these buffers, on the set's component stream
    begin_op(ctx, 0);
    const size_t nl = (size_t)nlists, g2 = (size_t)gridn * gridn;
    order_after_previous(ctx, {{(const char*)d_index, nl * g2 * 4}, {(const char*)d_status, nl * 4}},
                         {{(const char*)d_xy, nl * (size_t)capacity * 8}, {(const char*)d_counts, nl * 4}});
    hipError_t e = hipEventRecord(ctx->ev_pix[0], ctx->pix);
    if (e == hipSuccess) e = hipStreamWaitEvent(cur_cc(ctx), ctx->ev_pix[0], 0);
    const int rc = e == hipSuccess ? launch_find_grids(ctx, ctx->cur, d_xy, d_counts, nlists, capacity, gridn, d_index, d_status, cur_cc(ctx)) : 0;
    // the op ends on every path, like the others (it leaves no status words and has counted no hot pixel: of end_op, the
    // event alone)
    const hipError_t e_done = hipEventRecord(ctx->ev_cc_done[ctx->cur], cur_cc(ctx));
    ctx->cc_pending[ctx->cur] = true;
    MRG_HIP_CHECK(e);
    MRG_HIP_CHECK(e_done);
    return rc;
}

int mrgingham_amd_find_grids_stats(mrgingham_amd_ctx* ctx, double* out, int n, int reset) {
    if (!ctx || !out || n < 0) return MRGINGHAM_AMD_ERR_ARG;
    fb_drain(ctx);
    unsigned long long words[kGfStatWords] = {};
    if (ctx->grid_stat.p) {
        MRG_HIP_CHECK(hipSetDevice(ctx->device));
        MRG_HIP_CHECK(hipDeviceSynchronize());
        MRG_HIP_CHECK(hipMemcpy(words, ctx->grid_stat.p, sizeof(words), hipMemcpyDeviceToHost));
        if (reset) MRG_HIP_CHECK(hipMemset(ctx->grid_stat.p, 0, sizeof(words)));
    }
    for (int i = 0; i < n && i < MRGINGHAM_AMD_FIND_GRIDS_STATS; ++i)
        out[i] = i < kGfStatWords ? (double)words[i] : (double)ctx->fb_grid_fallbacks;
    if (reset) ctx->fb_grid_fallbacks = 0;
    return MRGINGHAM_AMD_FIND_GRIDS_STATS;
}

}  // extern "C"
