// The host model of the device grid finder: grid_phases.h, the text grid_find.hip runs with one workgroup per list, run
// serially -- one lane, phase loop by phase loop -- over lists in host memory.  No device, no context.  It answers what
// the kernel answers, list for list, every status and decline reason included, because both sides make the same IEEE
// operations in the same order; it is what a debugger steps through when a device test disagrees.  See
// include/mrgingham_amd.h (mrgingham_amd_find_grids_host) and DESIGN.md section 4.25.
#include <memory>

#include "../../include/mrgingham_amd.h"
#include "grid_phases.h"

namespace {

struct HostLane {
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void barrier() const {}
    void lower(int32_t* word, int value) const {
        if (value < *word) *word = value;
    }
};

}  // namespace

extern "C" int mrgingham_amd_find_grids_host(const int32_t* xy, const int32_t* counts, int nlists, int capacity, int gridn,
                                             int guard_bits, int32_t* index, int32_t* status) {
    using namespace mrg;
    if (nlists < 0 || capacity < 0 || gridn < kGfMinGridn || gridn > kGfMaxGridn || guard_bits < kGfGuardBitsMin ||
        guard_bits > kGfGuardBitsMax || (nlists > 0 && (!counts || !index || !status || (capacity > 0 && !xy))))
        return MRGINGHAM_AMD_ERR_ARG;
    if (nlists == 0) return MRGINGHAM_AMD_OK;
    const std::unique_ptr<GfNear> near_(new GfNear);
    const std::unique_ptr<GfFar> far_(new GfFar);
    HostLane x;
    for (int l = 0; l < nlists; ++l)
        status[l] = gf_find_grid(x, *near_, *far_, xy + (size_t)l * capacity * 2, counts[l], capacity, gridn, guard_bits,
                                 index + (size_t)l * gridn * gridn);
    return MRGINGHAM_AMD_OK;
}
