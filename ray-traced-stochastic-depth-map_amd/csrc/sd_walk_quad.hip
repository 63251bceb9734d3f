// sd_walk_quad.hip -- the quad walks of the SD trace: walk 0, the depth-first canonical walk (sd_quad.h's body), and
// walk 3, the depth-first traversal-order any-hit stream.  (Overview: sd_common.h)
#include "sd_launch.h"
#include "sd_quad.h"

namespace rsd {

template <int K, int N, bool SPEC = false, bool CNT = false>
__global__ void __launch_bounds__(kBlock) sd_trace_queue_kernel(SDArgs a, const float4* __restrict__ queue,
                                                                uint32_t* __restrict__ qctl) {
    extern __shared__ uint32_t sQuadStack[];
    sd_trace_queue_body<K, N, SPEC, CNT>(a, queue, qctl, sQuadStack, blockIdx.x, gridDim.x, a.qrange);
}

// ------------------------------------------------------------------------------------
// Traversal-order any-hit stream (rsd_sd_params.hit_order = RSD_HIT_ORDER_TRAVERSAL, rsd.h).
// The DXR-like order: a depth-first walk of the 4-wide BVH, children nearest entry distance
// first (the quad sorting network below; ties keep child-slot order), leaf triangles in record
// order, each triangle delivered once to anyHit -> algorithm as it is found.  A committed hit
// (Common.slangh: algorithm() == true, the any-hit shader does not IgnoreHit) shrinks the ray's
// TMax to its t, and later candidates must be nearer (t < TMax), so the reservoir's random slot
// replacement (Common.slangh:137-151) really samples: the texel depends on the BVH (the oracle
// walks the same tree, rsd_scene_export_bvh).  A quad (4 lanes) walks one ray: lane q tests
// child q / triangle q, the leaf's candidates are delivered one by one in record order with the
// TMax test repeated against the current TMax.  All 4 lanes keep identical algorithm state.
// ------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void sd_trace_ordered_ray(const SDArgs& a, f3 d, float TMin, float TMax, float cosT,
                                                     float (&depths)[N], uint32_t* __restrict__ sItem,
                                                     float* __restrict__ sT, int q, int quadBase, TraceStats& st,
                                                     uint32_t& delivered) {
    const rsd_camera& c = a.cam;
    RayCtx r;
    ray_setup(r, mk(c.posW[0], c.posW[1], c.posW[2]), d);
    uint32_t cnt = 0;
    float tCur = TMax;       // RayTCurrent(): TMax, then the t of the last committed hit
    bool committed = false;  // after a commit only nearer hits (t < tCur) are candidates
    int sp = 0;
    uint32_t item = 0;       // the root node
    const float* bf = reinterpret_cast<const float*>(a.nodes);
    while (true) {
        const uint32_t off = item & kOffMask;
        uint32_t next = kNoItem;
        if (item & kLeafBit) {
            st.leaves++;
            const uint32_t n = ((item >> 29) & 3u) + 1u;
            bool cand = false, af = false;
            float t = 0.0f, rng = 0.0f, z = 0.0f;
            if ((uint32_t)q < n) {
                const float4* tp = a.nodes + off + 3u * (uint32_t)q;
                const float4 va = tp[0], vb = tp[1], vc = tp[2];
                st.tris++;
                float bu, bv, det;
                if (intersect_tri(r, va, vb, vc, t, bu, bv, det) && t >= TMin && t <= tCur &&
                    !culled(det, __float_as_uint(vb.w), a.cull)) {
                    cand = true;
                    rng = sd_hash(bu, bv);
                    z = t * cosT;  // RayToViewDepth
                    if (a.normalize) z = saturate((z - c.nearZ) / (c.farZ - c.nearZ));
                    af = a.alphaTest && (__float_as_uint(vb.w) & 4u) &&
                         alpha_test_fails(a.alphaData, __float_as_uint(va.w), va, vb, vc, bu, bv, true, t, r.d);
                }
            }
            const uint32_t afBits = (uint32_t)(__ballot(af) >> quadBase) & 0xfu;
            for (uint32_t m = (uint32_t)(__ballot(cand) >> quadBase) & 0xfu; m; m &= m - 1u) {
                const int j = __ffs(m) - 1;
                const float tj = qself(t, j), rj = qself(rng, j), zj = qself(z, j);
                if (committed ? !(tj < tCur) : !(tj <= tCur)) continue;  // behind the committed hit
                delivered++;
                if (sd_any_hit<N>(a, rj, zj, ((afBits >> j) & 1u) != 0u, depths, cnt)) {
                    tCur = tj;  // AcceptHit: TMax = t
                    committed = true;
                }
            }
        } else {
            st.nodes++;
            const float* nb = bf + 4u * off;
            const float lox = nb[q], hix = nb[4 + q], loy = nb[8 + q], hiy = nb[12 + q], loz = nb[16 + q],
                        hiz = nb[20 + q];
            const uint32_t ref = __float_as_uint(nb[24 + q]), ccnt = __float_as_uint(nb[28 + q]);
            float tn;
            const bool hit = ref != kNoItem && box_hit(r, lox, hix, loy, hiy, loz, hiz, TMin, tCur, tn);
            float k = hit ? tn : INFINITY;
            uint32_t it = hit ? make_item(ref, ccnt, a.triOff) : kNoItem;
            const int m = __popc((uint32_t)(__ballot(hit) >> quadBase) & 0xfu);
            // sorting network (0,1)(2,3) (0,2)(1,3) (1,2): a pair swaps only if strictly out of order
            quad_cx<kDppXor1>(k, it, (q & 1) == 0);
            quad_cx<kDppXor2>(k, it, (q & 2) == 0);
            {
                const float ok = dppf<kDppXor3>(k);
                const uint32_t oi = dppu<kDppXor3>(it);
                const bool mid = q == 1 || q == 2;
                const bool takeOther = mid && ((q == 1) ? (ok < k) : (k < ok));
                k = takeOther ? ok : k;
                it = takeOther ? oi : it;
            }
            next = qbcu<0>(it);
            if (q >= 1 && q < m) {
                const int slot = sp + (m - 1 - q);  // the nearest of the rest on top
                sItem[slot * kQuadRays] = it;
                sT[slot * kQuadRays] = k;
            }
            sp += m > 0 ? m - 1 : 0;
        }
        if (next == kNoItem) {
            while (sp > 0) {
                --sp;
                if (sT[sp * kQuadRays] <= tCur) { next = sItem[sp * kQuadRays]; break; }
            }
            if (next == kNoItem) break;
        }
        item = next;
    }
}

// Persistent waves over the live-ray queue (as sd_trace_queue_kernel), 16 rays per wave.
template <int N>
__global__ void __launch_bounds__(kBlock) sd_trace_ordered_kernel(SDArgs a, const float4* __restrict__ queue,
                                                                  uint32_t* __restrict__ qctl) {
    extern __shared__ uint32_t sQuadStack[];  // a.quadStack entries per ray: items, then their entry distances
    uint32_t* sItem = sQuadStack;
    float* sT = reinterpret_cast<float*>(sQuadStack + a.quadStack * kQuadRays);
    const int lane = threadIdx.x;
    const int q = lane & 3, quad = lane >> 2, quadBase = lane & ~3;
    const uint32_t part = blockIdx.x % kQueueParts, wavesPerPart = gridDim.x / kQueueParts;
    const uint32_t nLong = __hip_atomic_load(&qctl[part], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t count = nLong + (a.lpt ? __hip_atomic_load(&qctl[kQctlShort + part], __ATOMIC_RELAXED,
                                                               __HIP_MEMORY_SCOPE_AGENT) : 0u);
    const float DEFAULT = a.normalize ? 1.0f : 3.40282347e+37f;  // Common.slangh:16
    TraceStats st{0u, 0u, 0u};
    uint32_t active = 0, delivered = 0, maxNodes = 0, maxSteps = 0;
    uint32_t base = (blockIdx.x / kQueueParts) * (uint32_t)kQuadRays;
    bool firstChunk = true;
    while (base < count || (firstChunk && a.spread)) {
        // the static first chunk (spread: quad q of the partition's wave w takes index q * waves + w)
        const uint32_t qi = firstChunk && a.spread ? (uint32_t)quad * wavesPerPart + blockIdx.x / kQueueParts
                                                   : base + (uint32_t)quad;
        firstChunk = false;
        if (qi < count) {
            f3 d;
            float TMin, TMax, cosT;
            uint32_t idx;
            ray_rec_load(queue, queue_slot(a, part, qi, nLong), d, TMin, TMax, cosT, idx);
            float depths[N];
#pragma unroll
            for (int i = 0; i < N; ++i) depths[i] = DEFAULT;
            const uint32_t n0 = st.nodes, l0 = st.leaves;
            sd_trace_ordered_ray<N>(a, d, TMin, TMax, cosT, depths, &sItem[quad], &sT[quad], q, quadBase, st,
                                    delivered);
            if (q == 0) {
                maxNodes = max(maxNodes, st.nodes - n0);
                maxSteps = max(maxSteps, st.nodes - n0 + st.leaves - l0);
                active++;
                sd_store<N>(a, (int)(idx % (uint32_t)a.sdW), (int)(idx / (uint32_t)a.sdW), depths);
            }
        }
        if (lane == 0)
            base = wavesPerPart * (uint32_t)kQuadRays + atomicAdd(&qctl[kQueueParts + part], (uint32_t)kQuadRays);
        base = __shfl(base, 0);
    }
    if (a.counters) {
        atomicAdd(&a.counters[1], (unsigned long long)active);
        atomicAdd(&a.counters[2], (unsigned long long)(q == 0 ? st.nodes : 0u));
        atomicAdd(&a.counters[3], (unsigned long long)st.tris);
        atomicAdd(&a.counters[4], (unsigned long long)(q == 0 ? delivered : 0u));
        atomicMax(&a.counters[5], (unsigned long long)maxNodes);
        atomicMax(&a.counters[6], (unsigned long long)maxSteps);
        atomicAdd(&a.counters[9], (unsigned long long)(q == 0 ? st.leaves : 0u));
    }
}

// Walk 3 (the traversal-order stream), else walk 0
hipError_t launch_sd_walk_quad(const SDArgs& a, const SdPlan& pl, uint32_t N, const float4* queue, uint32_t* qctl,
                               hipStream_t s) {
    const dim3 pg(pl.persistentBlocks), wb(kBlock);
    const size_t lds = pl.ldsBytes;
    if (pl.walk == 3)
        return sd_dispatch_n(N, [&](auto n) {
            hipLaunchKernelGGL((sd_trace_ordered_kernel<decltype(n)::value>), pg, wb, lds, s, a, queue, qctl);
            return hipGetLastError();
        });
    return sd_dispatch_kn(pl.K, N, [&](auto k, auto n) {
        constexpr int K = decltype(k)::value, N_ = decltype(n)::value;
        if (pl.counters) hipLaunchKernelGGL((sd_trace_queue_kernel<K, N_, false, true>), pg, wb, lds, s, a, queue, qctl);
        else if (pl.spec) hipLaunchKernelGGL((sd_trace_queue_kernel<K, N_, true>), pg, wb, lds, s, a, queue, qctl);
        else hipLaunchKernelGGL((sd_trace_queue_kernel<K, N_>), pg, wb, lds, s, a, queue, qctl);
        return hipGetLastError();
    });
}

}  // namespace rsd
