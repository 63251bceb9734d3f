// sd_walk_row.hip -- the row walks of the SD trace (sd_row.h's body): walk 1, fused (the any-hit algorithm runs in the
// walk), and walk 2, split (the walk writes each ray's K nearest keys, sd_resolve_row_kernel runs the algorithm).
// (Overview: sd_common.h)
#include "sd_launch.h"
#include "sd_row.h"

namespace rsd {

template <int K, int N, int ROW, bool SPLIT, bool CNT, int POOL = kPoolCap, bool SPEC = false>
__global__ void __launch_bounds__(kBlock) sd_trace_row_kernel(SDArgs a, const float4* __restrict__ queue,
                                                              uint32_t* __restrict__ qctl, uint2* __restrict__ keys) {
    constexpr int kRowRays = kBlock / ROW;
    __shared__ uint32_t sItem[kRowRays * POOL];
    __shared__ float sT[kRowRays * POOL];
    sd_trace_row_body<K, N, ROW, SPLIT, CNT, POOL, SPEC>(a, queue, qctl, keys, sItem, sT, blockIdx.x, gridDim.x, a.qrange);
}

// Walk 2 (split: the walk, then the resolve), else walk 1 (fused)
hipError_t launch_sd_walk_row(const SDArgs& a, const SdPlan& pl, uint32_t N, const float4* queue, uint32_t* qctl,
                              uint2* keys, hipStream_t s) {
    const dim3 pg(pl.persistentBlocks), wb(kBlock);
    const bool cnt = pl.counters, small = pl.pool == 128;
    return sd_dispatch_kn(pl.K, N, [&](auto k, auto n) {
        constexpr int K = decltype(k)::value, N_ = decltype(n)::value, ROW = K <= 8 ? 8 : 16;
        if (pl.walk == 2) {
            if (cnt) hipLaunchKernelGGL((sd_trace_row_kernel<K, N_, ROW, true, true>), pg, wb, 0, s, a, queue, qctl, keys);
            else if (small) hipLaunchKernelGGL((sd_trace_row_kernel<K, N_, ROW, true, false, 128>), pg, wb, 0, s, a, queue, qctl, keys);
            else hipLaunchKernelGGL((sd_trace_row_kernel<K, N_, ROW, true, false>), pg, wb, 0, s, a, queue, qctl, keys);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL((sd_resolve_row_kernel<K, N_, ROW>), pg, wb, 0, s, a, queue, qctl, keys);
        } else {
            if (cnt) hipLaunchKernelGGL((sd_trace_row_kernel<K, N_, ROW, false, true>), pg, wb, 0, s, a, queue, qctl, keys);
            else if (pl.spec && small) hipLaunchKernelGGL((sd_trace_row_kernel<K, N_, ROW, false, false, 128, true>), pg, wb, 0, s, a, queue, qctl, keys);
            else if (pl.spec) hipLaunchKernelGGL((sd_trace_row_kernel<K, N_, ROW, false, false, kPoolCap, true>), pg, wb, 0, s, a, queue, qctl, keys);
            else hipLaunchKernelGGL((sd_trace_row_kernel<K, N_, ROW, false, false>), pg, wb, 0, s, a, queue, qctl, keys);
        }
        return hipGetLastError();
    });
}

}  // namespace rsd
