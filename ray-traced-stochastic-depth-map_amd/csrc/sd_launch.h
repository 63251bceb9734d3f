// sd_launch.h -- the launchers of the SD trace's kernels, one per translation unit that defines kernels, and the
// K x N dispatch they share.  sd_trace.hip calls them in the order the plan (sd_plan.h) decided; a launcher decides
// nothing, it branches on SdPlan fields to name the instantiation the plan chose.  Each returns the first launch error.
#pragma once
#include <type_traits>

#include "sd_common.h"

namespace rsd {

// sd_setup.hip.  sd_setup_build_key: the kPlanBuildKey its kernels were compiled with (SdPlan.buildKey must match).
uint32_t sd_setup_build_key();
hipError_t launch_ray_table(float* tab, int sdW, int sdH, int guard, uint32_t jitter, const rsd_camera& cam,
                            hipStream_t s);
hipError_t launch_sd_setup(const SDArgs& a, const SdPlan& pl, uint32_t N, float4* queue, uint32_t* qctl, hipStream_t s);

// the walks: SdPlan.walk 0 and 3 (sd_walk_quad.hip), 1 and 2 (sd_walk_row.hip), 6, 5, 4
hipError_t launch_sd_walk_quad(const SDArgs& a, const SdPlan& pl, uint32_t N, const float4* queue, uint32_t* qctl,
                               hipStream_t s);
hipError_t launch_sd_walk_row(const SDArgs& a, const SdPlan& pl, uint32_t N, const float4* queue, uint32_t* qctl,
                              uint2* keys, hipStream_t s);
hipError_t launch_sd_walk_hybrid(const SDArgs& a, const SdPlan& pl, uint32_t N, const float4* queue, uint32_t* qctl,
                                 uint2* keys, hipStream_t s);
hipError_t launch_sd_walk_wavefront(const SDArgs& a, const SdPlan& pl, uint32_t N, const float4* queue, uint32_t* qctl,
                                    hipStream_t s);
hipError_t launch_sd_walk_raster(const SDArgs& a, const SdPlan& pl, uint32_t N, const float4* queue, uint32_t* qctl,
                                 uint2* keys, hipStream_t s);

// f(std::integral_constant<int, N>) for the sample count N of the call, f(K, N) with the plan's K (4, 8 or 16) too
template <int V>
using sd_int = std::integral_constant<int, V>;
template <class F>
hipError_t sd_dispatch_n(uint32_t N, F&& f) {
    switch (N) {
        case 1: return f(sd_int<1>{});
        case 2: return f(sd_int<2>{});
        case 4: return f(sd_int<4>{});
        case 8: return f(sd_int<8>{});
        case 16: return f(sd_int<16>{});
        default: return hipErrorInvalidValue;
    }
}
template <class F>
hipError_t sd_dispatch_kn(uint32_t K, uint32_t N, F&& f) {
    return sd_dispatch_n(N, [&](auto n) {
        return K == 4 ? f(sd_int<4>{}, n) : K == 8 ? f(sd_int<8>{}, n) : f(sd_int<16>{}, n);
    });
}

}  // namespace rsd
