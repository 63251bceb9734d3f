// sd_quad.h -- the quad walk of the SD trace: the DPP quad exchanges, the distributed k-list and the body that
// sd_walk_quad.hip (walk 0) and sd_walk_hybrid.hip (the quad blocks of walk 6) wrap in kernels.  sd_row.h builds
// its row exchanges on dppu.
#pragma once
#include "sd_common.h"

namespace rsd {

// ------------------------------------------------------------------------------------
// Quad-cooperative traversal (the SD trace).  A live SD ray is latency-bound: few rays,
// long dependent chains (MI355X: one wave alone issues a VALU op every ~4 cycles).  So
// each ray is walked by a QUAD of 4 lanes: in a node step lane q fetches and tests child
// q (the node is SoA, so the quad's 8 loads of 4 B are 16-B coalesced rows); in a leaf
// step lane q tests triangle q.  The 4 child keys are sorted across the quad with
// __shfl_xor compare-exchanges, the nearest is taken and the rest go to the ray's LDS
// stack.  Every lane keeps an identical copy of the ray's k-list; accepted hits are
// broadcast one by one and inserted by all 4 lanes.  A wave walks 16 rays (kQuadRays), each with an LDS
// stack of SDArgs.quadStack entries (quad_stack_entries, sd_plan.h).
// ------------------------------------------------------------------------------------

// Quad-local exchange through DPP quad_perm (a VALU modifier: no LDS round trip, unlike
// __shfl / ds_bpermute).  CTRL = quad_perm(p0,p1,p2,p3) = p0 | p1<<2 | p2<<4 | p3<<6.
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppXor3 = 0x1B;
template <int CTRL>
__device__ __forceinline__ uint32_t dppu(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int L>  // value of quad lane L, in every lane of the quad
__device__ __forceinline__ float qbcf(float v) { return dppf<L * 0x55>(v); }
template <int L>
__device__ __forceinline__ uint32_t qbcu(uint32_t v) { return dppu<L * 0x55>(v); }
__device__ __forceinline__ float qself(float v, int j) {
    const float b0 = qbcf<0>(v), b1 = qbcf<1>(v), b2 = qbcf<2>(v), b3 = qbcf<3>(v);
    return j == 0 ? b0 : (j == 1 ? b1 : (j == 2 ? b2 : b3));
}
__device__ __forceinline__ uint32_t qselu(uint32_t v, int j) {
    const uint32_t b0 = qbcu<0>(v), b1 = qbcu<1>(v), b2 = qbcu<2>(v), b3 = qbcu<3>(v);
    return j == 0 ? b0 : (j == 1 ? b1 : (j == 2 ? b2 : b3));
}

template <int CTRL>
__device__ __forceinline__ void quad_cx(float& k, uint32_t& it, bool low) {
    const float ok = dppf<CTRL>(k);
    const uint32_t oi = dppu<CTRL>(it);
    const bool takeOther = low ? (ok < k) : (k < ok);
    k = takeOther ? ok : k;
    it = takeOther ? oi : it;
}

// Step clocks of the instrumented quad walk (rsd_counters.step_*; the latency floor of bench.py): per
// step of a ray -- one iteration of its quad's loop -- the wait for the step's own fetch (the
// instrumented build waits right after issuing it), its own box / triangle tests and merge, the stack
// push / pop from the point where the quad's branches reconverge, and the whole iteration from loop top
// to loop top (the remainder is the other branch of the wave: divergence).  s_memtime is wave-uniform;
// every quad's lane 0 accumulates its own ray's steps.
struct QuadClk {
    unsigned long long fetch = 0, tests = 0, stack = 0, total = 0, steps = 0;
};

// The quad walk's K nearest keys, distributed over the quad (round 5): lane q holds keys j = 4 s + q (slot s
// of S = K / 4), so each lane keeps K / 4 keys instead of a copy of all K (at K = 16: 8 instead of 32 VGPRs,
// and the record index is not kept at all -- the epilogue finds a key's triangle record through the scene's
// primitive -> record map).  Lane q's slots are exactly the keys whose terms lane q prepares in the epilogue.
// Every lane of the quad inserts the same key: its position is the quad-wide count of keys before it, and
// each slot at or after it takes the key before it -- lane q - 1's same slot, or (lane 0) lane 3's previous
// slot -- through one quad rotation per slot.  The K-th key is kept replicated for the pruning tests.
constexpr int kDppQuadRotR = 0x93;  // quad_perm [3, 0, 1, 2]: lane q reads lane q - 1 (lane 0: lane 3)
template <int K>
struct QuadKeys {
    static constexpr int S = K / 4;
    float t[S];
    uint32_t p[S];
    float kthT;  // key K - 1 (every lane)
    uint32_t kthP;
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < S; ++i) { t[i] = INFINITY; p[i] = 0xffffffffu; }
        kthT = INFINITY;
        kthP = 0xffffffffu;
    }
    __device__ __forceinline__ void insert(float nt, uint32_t np, int q) {
        uint32_t c = 0u;
#pragma unroll
        for (int i = 0; i < S; ++i) c += key_less(t[i], p[i], nt, np) ? 1u : 0u;
        c += dppu<kDppXor1>(c);
        c += dppu<kDppXor2>(c);  // every lane: the keys before the new one
        float rt[S];
        uint32_t rp[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            rt[i] = dppf<kDppQuadRotR>(t[i]);
            rp[i] = dppu<kDppQuadRotR>(p[i]);
        }
#pragma unroll
        for (int i = 0; i < S; ++i) {
            const uint32_t j = 4u * (uint32_t)i + (uint32_t)q;
            const float prevT = q > 0 ? rt[i] : (i > 0 ? rt[i > 0 ? i - 1 : 0] : INFINITY);
            const uint32_t prevP = q > 0 ? rp[i] : (i > 0 ? rp[i > 0 ? i - 1 : 0] : 0xffffffffu);
            const bool put = j == c, shift = j > c;
            t[i] = put ? nt : (shift ? prevT : t[i]);
            p[i] = put ? np : (shift ? prevP : p[i]);
        }
        kthT = qbcf<3>(t[S - 1]);
        kthP = qbcu<3>(p[S - 1]);
    }
};

template <int K>
__device__ __forceinline__ int trace_knearest_quad(const float4* __restrict__ bvh, uint32_t triOff, const RayCtx& r,
                                                   float tmin, float tmax, uint32_t cull, bool useLB, float lbT,
                                                   uint32_t lbP, QuadKeys<K>& kl, uint32_t* __restrict__ sItem,
                                                   float* __restrict__ sT, int q, int quadBase, TraceStats& st,
                                                   const uint32_t* __restrict__ ent, uint32_t nEnt,
                                                   QuadClk* clk = nullptr) {
    kl.clear();
    int sp = 0, found = 0;
    unsigned long long tTop = clk ? __builtin_amdgcn_s_memtime() : 0ull, tA = 0ull, tF = 0ull;
    uint32_t item = 0;
    if (nEnt) {
        // the segment's entry-grid frontier (entry_grid.h): item 0 first, the rest on the stack
        // (entry distance -inf: always popped; the result does not depend on the order)
        item = ent[0];
        if (q == 0)
            for (uint32_t e = 1; e < nEnt; ++e) {
                sItem[(e - 1) * kQuadRays] = ent[e];
                sT[(e - 1) * kQuadRays] = -INFINITY;
            }
        sp = (int)nEnt - 1;
    }
    const float tlo = useLB ? fmaxf(tmin, lbT) : tmin;
    const float* bf = reinterpret_cast<const float*>(bvh);
    while (true) {
        const uint32_t off = item & kOffMask;
        uint32_t next = kNoItem;
        if (clk) tA = __builtin_amdgcn_s_memtime();
        if (item & kLeafBit) {
            st.leaves++;
            const uint32_t cnt = ((item >> 29) & 3u) + 1u;
            bool acc = false;
            float t = 0.0f;
            uint32_t prim = 0u;
            float4 va = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vb = va, vc = va;
            if ((uint32_t)q < cnt) {
                const float4* tp = bvh + off + 3u * (uint32_t)q;
                va = tp[0];
                vb = tp[1];
                vc = tp[2];
            }
            if (clk) {  // the step's fetch (the instrumented build waits here)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                tF = __builtin_amdgcn_s_memtime();
                if (q == 0) clk->fetch += tF - tA;
            }
            if ((uint32_t)q < cnt) {
                st.tris++;
                float bu, bv, det;
                if (intersect_tri(r, va, vb, vc, t, bu, bv, det) && t >= tmin && t <= tmax) {
                    prim = __float_as_uint(va.w);
                    acc = !culled(det, __float_as_uint(vb.w), cull) && (!useLB || key_less(lbT, lbP, t, prim)) &&
                          key_less(t, prim, kl.kthT, kl.kthP);
                }
            }
            uint32_t m = (uint32_t)(__ballot(acc) >> quadBase) & 0xfu;
            while (m) {
                const int j = __ffs(m) - 1;
                m &= m - 1u;
                const float tj = qself(t, j);
                const uint32_t pj = qselu(prim, j);
                if (key_less(tj, pj, kl.kthT, kl.kthP)) {
                    kl.insert(tj, pj, q);
                    found = found < K ? found + 1 : K;
                }
            }
            if (clk && q == 0) clk->tests += __builtin_amdgcn_s_memtime() - tF;
        } else {
            st.nodes++;
            const float thi = fminf(tmax, kl.kthT);
            const float* nb = bf + 4u * off;
            const float lox = nb[q], hix = nb[4 + q], loy = nb[8 + q], hiy = nb[12 + q], loz = nb[16 + q],
                        hiz = nb[20 + q];
            const uint32_t ref = __float_as_uint(nb[24 + q]), cnt = __float_as_uint(nb[28 + q]);
            if (clk) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                tF = __builtin_amdgcn_s_memtime();
                if (q == 0) clk->fetch += tF - tA;
            }
            float tn;
            const bool hit = ref != kNoItem && box_hit(r, lox, hix, loy, hiy, loz, hiz, tlo, thi, tn);
            float k = hit ? tn : INFINITY;
            uint32_t it = hit ? make_item(ref, cnt, triOff) : kNoItem;
            const int m = __popc((uint32_t)(__ballot(hit) >> quadBase) & 0xfu);
            // sorting network (0,1)(2,3) (0,2)(1,3) (1,2) across the quad
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
            if (clk && q == 0) clk->tests += __builtin_amdgcn_s_memtime() - tF;
            if (q >= 1 && q < m) {
                const int slot = sp + (m - 1 - q);  // farthest deepest
                sItem[slot * kQuadRays] = it;
                sT[slot * kQuadRays] = k;
            }
            sp += m > 0 ? m - 1 : 0;
        }
        if (clk) tA = __builtin_amdgcn_s_memtime();  // the branches reconverged
        if (next == kNoItem) {
            const float thi = fminf(tmax, kl.kthT);
            while (sp > 0) {
                --sp;
                const float tt = sT[sp * kQuadRays];
                if (tt <= thi) { next = sItem[sp * kQuadRays]; break; }
            }
        }
        if (clk) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            if (q == 0) {
                clk->stack += t - tA;
                clk->total += t - tTop;
                clk->steps++;
            }
            tTop = t;
        }
        if (next == kNoItem) break;
        item = next;
    }
    return found;
}

// TraceRay + anyHit -> algorithm (Common.slangh:102-254) over the canonical hit stream,
// for the ray of this quad.  All 4 lanes end with identical depths.
template <int K, int N, bool SPEC = false>
__device__ __forceinline__ void sd_resolve(const SDArgs& a, f3 d, float TMin, float TMax, float cosT, float (&depths)[N],
                                           uint32_t* sItem, float* sT, int q, int quadBase, TraceStats& st,
                                           uint32_t& hitsDelivered, const uint32_t* ent = nullptr,
                                           uint32_t nEnt = 0u, QuadClk* clk = nullptr) {
    const rsd_camera& c = a.cam;
    RayCtx r;
    ray_setup(r, mk(c.posW[0], c.posW[1], c.posW[2]), d);
    QuadKeys<K> kl;
    uint32_t count = 0;
    bool commit = false, useLB = false;
    float lbT = 0.0f;
    uint32_t lbP = 0u;
    constexpr int J = (K + 3) / 4;  // hits per lane in the epilogue
    while (!commit) {
        // SPEC (as the row walk's): one chunk of K keys decides the texel -- no lower bound, no alpha test
        const int found = trace_knearest_quad<K>(a.nodes, a.triOff, r, TMin, TMax, a.cull, SPEC ? false : useLB, lbT, lbP, kl, sItem,
                                                 sT, q, quadBase, st, ent, nEnt, SPEC ? nullptr : clk);
        // barycentrics + hash of hit j are computed by lane j % 4 (re-running the identical
        // triangle test on the hit's record), then shared with the quad
        float rngL[J], zL[J];
        uint32_t afL = 0u;  // bit i: hit 4 i + q fails the alpha test
#pragma unroll
        for (int i = 0; i < J; ++i) {
            const int j = 4 * i + q;
            rngL[i] = 0.0f;
            zL[i] = 0.0f;
            uint32_t ti = 0u;
            if (j < found) ti = a.primRec[kl.p[i]];  // key j = 4 i + q is this lane's slot i
            if (j < found) {
                float t, bu, bv, det;
                const float4 v0 = a.tris[3 * ti], v1 = a.tris[3 * ti + 1], v2 = a.tris[3 * ti + 2];
                intersect_tri(r, v0, v1, v2, t, bu, bv, det);
                rngL[i] = sd_hash(bu, bv);
                float z = t * cosT;  // RayToViewDepth
                if (a.normalize) z = saturate((z - c.nearZ) / (c.farZ - c.nearZ));
                zL[i] = z;
                if (!SPEC && a.alphaTest && (__float_as_uint(v1.w) & 4u) &&
                    alpha_test_fails(a.alphaData, __float_as_uint(v0.w), v0, v1, v2, bu, bv, true, t, r.d))
                    afL |= 1u << i;
            }
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const float rng = qself(rngL[j / 4], j % 4);
            float z = qself(zL[j / 4], j % 4);
            const bool af = (qselu(afL, j % 4) >> (j / 4)) & 1u;
            if (commit || j >= found) continue;
            hitsDelivered++;
            commit = sd_any_hit_impl<N, SPEC ? 0 : -1>(a, rng, z, af, depths, count);
        }
        if (SPEC || found < K) break;  // stream exhausted (SPEC: a commit by the K-th key)
        useLB = true;
        lbT = kl.kthT;
        lbP = kl.kthP;
    }
}

// Phase 2: persistent waves pull 16 live rays (one per quad) at a time from the queue
// until it drains (every wave reaches the exit: the head only grows, the count is fixed).
// The first chunk of each wave is static (blockIdx); later ones come from one atomic head
// that starts after the static range, so a wave with no static chunk exits without an
// atomic (one head word serialises ~90 dequeues/us, MI355X_MICROARCH.md "dequeue").
template <int K, int N, bool SPEC = false, bool CNT = false>
__device__ __forceinline__ void sd_trace_queue_body(const SDArgs& a, const float4* __restrict__ queue,
                                                    uint32_t* __restrict__ qctl, uint32_t* sQuadStack, uint32_t bid,
                                                    uint32_t nb, uint32_t qr) {
    // sQuadStack: a.quadStack entries per ray, items then their entry distances; (bid, nb): this wave's block
    // among the walk's blocks (the hybrid kernel's quad blocks follow its row blocks); qr: the queue range
    uint32_t* sItem = sQuadStack;
    float* sT = reinterpret_cast<float*>(sQuadStack + a.quadStack * kQuadRays);
    const int lane = threadIdx.x;
    const int q = lane & 3, quad = lane >> 2, quadBase = lane & ~3;
    // wave w serves partition w % kQueueParts (nb is a multiple of kQueueParts)
    const uint32_t part = bid % kQueueParts, wavesPerPart = nb / kQueueParts;
    const uint32_t nLong = __hip_atomic_load(&qctl[part], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // (RSD_TRACE_QRANGE, diagnostics: only the longest-first rays, or only the others)
    const uint32_t q0 = qr == 2u ? nLong : 0u;
    const uint32_t count = (qr == 1u ? nLong : nLong + (a.lpt ? __hip_atomic_load(&qctl[kQctlShort + part],
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u)) - q0;
    TraceStats st{0u, 0u, 0u};
    uint32_t active = 0, hitsDelivered = 0, maxNodes = 0, maxSteps = 0;
    unsigned long long sumCycles = 0, maxCycles = 0;
    // instrumented traces (counters): the step clocks of every ray (QuadClk) and the clock calibration of
    // the first wave (s_memtime ticks against the 100 MHz s_memrealtime), as the row walk's
    QuadClk clk;
    unsigned long long cal0 = 0, calR0 = 0;
    if (CNT && bid == 0) {
        cal0 = __builtin_amdgcn_s_memtime();
        calR0 = __builtin_amdgcn_s_memrealtime();
    }
    uint32_t base = (bid / kQueueParts) * (uint32_t)kQuadRays;
    bool firstChunk = true;
    while (base < count || (firstChunk && a.spread)) {
        // the static first chunk (spread: quad q of the partition's wave w takes index q * waves + w)
        const uint32_t qi = firstChunk && a.spread ? (uint32_t)quad * wavesPerPart + bid / kQueueParts
                                                   : base + (uint32_t)quad;
        firstChunk = false;
        if (qi < count) {
            f3 d;
            float TMin, TMax, cosT;
            uint32_t idx, nEnt;
            const uint32_t slot = queue_slot(a, part, qi + q0, nLong);
            ray_rec_load(queue, slot, d, TMin, TMax, cosT, idx, nEnt);
            const int x = (int)(idx % (uint32_t)a.sdW), y = (int)(idx / (uint32_t)a.sdW);
            float depths[N];
            const float DEFAULT = a.normalize ? 1.0f : 3.40282347e+37f;
#pragma unroll
            for (int i = 0; i < N; ++i) depths[i] = DEFAULT;
            const uint32_t n0 = st.nodes, l0 = st.leaves;
            const unsigned long long c0 = a.counters ? __builtin_amdgcn_s_memtime() : 0ull;
            sd_resolve<K, N, SPEC>(a, d, TMin, TMax, cosT, depths, &sItem[quad], &sT[quad], q, quadBase, st,
                             hitsDelivered, a.entOn ? a.entQ + (size_t)slot * kEntryCap : nullptr, nEnt,
                             CNT ? &clk : nullptr);
            if (q == 0) {
                if (a.counters) {
                    const unsigned long long dc = __builtin_amdgcn_s_memtime() - c0;
                    sumCycles += dc;
                    maxCycles = dc > maxCycles ? dc : maxCycles;
                }
                maxNodes = max(maxNodes, st.nodes - n0);
                maxSteps = max(maxSteps, st.nodes - n0 + st.leaves - l0);
                active++;
                sd_store<N>(a, x, y, depths);
            }
        }
        if (lane == 0)
            base = wavesPerPart * (uint32_t)kQuadRays + atomicAdd(&qctl[kQueueParts + part], (uint32_t)kQuadRays);
        base = __shfl(base, 0);
    }
    if (a.counters) {
        if (q != 0) hitsDelivered = 0;
        atomicAdd(&a.counters[1], (unsigned long long)active);
        atomicAdd(&a.counters[2], (unsigned long long)(q == 0 ? st.nodes : 0u));
        atomicAdd(&a.counters[3], (unsigned long long)st.tris);
        atomicAdd(&a.counters[4], (unsigned long long)hitsDelivered);
        atomicMax(&a.counters[5], (unsigned long long)maxNodes);
        atomicMax(&a.counters[6], (unsigned long long)maxSteps);
        atomicAdd(&a.counters[7], sumCycles);
        atomicMax(&a.counters[8], maxCycles);
        atomicAdd(&a.counters[9], (unsigned long long)(q == 0 ? st.leaves : 0u));
        if (CNT && q == 0) {  // step clocks (rsd_counters.step_*): compute = own tests + the other branch
            atomicAdd(&a.counters[14], clk.steps);
            atomicAdd(&a.counters[16], clk.fetch);
            atomicAdd(&a.counters[17], clk.total - clk.fetch - clk.stack);
            atomicAdd(&a.counters[18], clk.stack);
            atomicAdd(&a.counters[24], clk.tests);
        }
        if (CNT && bid == 0 && lane == 0) {
            const unsigned long long cal1 = __builtin_amdgcn_s_memtime(), calR1 = __builtin_amdgcn_s_memrealtime();
            atomicMax(&a.counters[21], cal1 - cal0);
            atomicMax(&a.counters[22], calR1 - calR0);
        }
    }
}

}  // namespace rsd
