// sd_walk_hybrid.hip -- walk 6 of the SD trace: sd_row.h's body and sd_quad.h's in one kernel.  (Overview: sd_common.h)
#include "sd_launch.h"
#include "sd_quad.h"
#include "sd_row.h"

namespace rsd {

// The hybrid walk (walk 6): one launch whose first a.hybridRowBlocks blocks walk the longest-first rays with the
// specialised row walk and whose other blocks walk the remaining rays with the specialised quad walk, so the long
// rays' chains (which set a quad-walk launch) take 8 items per step while the bulk keeps the quad walk's lane use.
// One dynamic LDS allocation serves either role (max of the two).
template <int K, int N, int ROW, int POOL>
__global__ void __launch_bounds__(kBlock) sd_trace_hybrid_kernel(SDArgs a, const float4* __restrict__ queue,
                                                                 uint32_t* __restrict__ qctl, uint2* __restrict__ keys) {
    extern __shared__ uint32_t sDyn[];
    const uint32_t rb = a.hybridRowBlocks;
    if ((blockIdx.x < rb && a.rowPrio) || a.prio) __builtin_amdgcn_s_setprio(2);  // (rowPrio: neutral, trace_ab/prio_*)
    if (blockIdx.x < rb)
        sd_trace_row_body<K, N, ROW, false, false, POOL, true>(
            a, queue, qctl, keys, sDyn, reinterpret_cast<float*>(sDyn + (kBlock / ROW) * POOL), blockIdx.x, rb, 1u);
    else
        sd_trace_queue_body<K, N, true>(a, queue, qctl, sDyn, blockIdx.x - rb, gridDim.x - rb, 2u);
}

hipError_t launch_sd_walk_hybrid(const SDArgs& a, const SdPlan& pl, uint32_t N, const float4* queue, uint32_t* qctl,
                                 uint2* keys, hipStream_t s) {
    const dim3 pg(pl.persistentBlocks), wb(kBlock);
    const size_t lds = pl.ldsBytes;
    return sd_dispatch_kn(pl.K, N, [&](auto k, auto n) {
        constexpr int K = decltype(k)::value, N_ = decltype(n)::value;
        if (pl.pool == 128) hipLaunchKernelGGL((sd_trace_hybrid_kernel<K, N_, 8, 128>), pg, wb, lds, s, a, queue, qctl, keys);
        else hipLaunchKernelGGL((sd_trace_hybrid_kernel<K, N_, 8, kPoolCap>), pg, wb, lds, s, a, queue, qctl, keys);
        return hipGetLastError();
    });
}

}  // namespace rsd
