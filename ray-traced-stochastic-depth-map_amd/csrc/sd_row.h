// sd_row.h -- the row walk of the SD trace: the row exchanges, the any-hit algorithm over a row's sorted keys, the
// body that sd_walk_row.hip (walks 1 and 2) and sd_walk_hybrid.hip (the row blocks of walk 6) wrap in kernels, and
// sd_resolve_row_kernel, which sd_walk_row.hip (the split walk's keys) and sd_walk_raster.hip (the raster walk's)
// each instantiate.  sd_walk_wavefront.hip uses the row exchanges alone.
#pragma once
#include "sd_common.h"
#include "sd_quad.h"  // dppu

namespace rsd {

// ------------------------------------------------------------------------------------
// Row-parallel traversal (the default SD trace).  The quad walk (sd_quad.h) is depth-first: its
// critical path is every node and leaf the ray visits, one dependent fetch after the other
// (the slowest live ray of a 1080p/4 frame visits ~130 items, and the launch lasts as long
// as that ray).  Here a ray is walked by a ROW of 16 lanes (a quarter wave): each step, up
// to 16 work items (4-wide nodes or leaves) taken from the top of the ray's LDS pool are
// processed at once, one per lane, and their surviving children are pushed back, nearest on
// top.  The critical path becomes ~ the tree depth plus (visited items / 16).
// The ray's k-list is sorted ACROSS the row (lane j holds key j, up to 16 keys): inserting a
// hit is one ballot and three shuffles.  Pruning is the depth-first walk's: an item is
// dropped once the K-th key is nearer than its box, which only depends on keys found, so the
// K nearest keys -- and the SD texel -- do not depend on the visiting order.
// Pool bound: a row pops 16 items per step while the pool holds <= poolSoft items and one
// item (a depth-first step, +3 items per level at most) above, so the pool never exceeds
// poolSoft + 48 + 3 * (wide tree depth) <= kPoolCap (poolSoft is derived from the depth: sd_plan.cpp).
// A wave walks 4 rays; every row refills from the live-ray queue on its own.
// ------------------------------------------------------------------------------------

template <int ROW>
__device__ __forceinline__ uint32_t row_bits(bool p, int base) {
    return (uint32_t)(__ballot(p) >> base) & ((1u << ROW) - 1u);
}

// Row-local moves without the LDS crossbar (8-lane rows: two per 16-lane DPP row; 16-lane
// rows fall back to __shfl).  DPP row_shr:n -> lane i reads lane i - n, row_shl:n -> i + n.
constexpr int kDppRowShr1 = 0x111, kDppRowShr4 = 0x114, kDppRowShl4 = 0x104;
// value of row lane L (3 or 7 for 8-lane rows) in every lane of the row
template <int ROW, int L>
__device__ __forceinline__ uint32_t row_bcast(uint32_t v, int l, int base) {
    if constexpr (ROW == 8) {
        const uint32_t q = dppu<(L & 3) * 0x55>(v);  // lanes 0-3 <- lane L % 4, lanes 4-7 <- lane 4 + L % 4
        if constexpr (L >= 4) {
            const uint32_t w = dppu<kDppRowShl4>(q);  // lanes 0-3 <- lane L
            return l < 4 ? w : q;
        } else {
            const uint32_t w = dppu<kDppRowShr4>(q);  // lanes 4-7 <- lane L
            return l < 4 ? q : w;
        }
    } else {
        return (uint32_t)__shfl((int)v, base + L);
    }
}
template <int ROW, int L>
__device__ __forceinline__ float row_bcastf(float v, int l, int base) {
    return __uint_as_float(row_bcast<ROW, L>(__float_as_uint(v), l, base));
}
// value of row lane l - 1 (lane 0's result is unspecified)
template <int ROW>
__device__ __forceinline__ uint32_t row_prev(uint32_t v, int l, int base) {
    if constexpr (ROW == 8) return dppu<kDppRowShr1>(v);
    else return (uint32_t)__shfl((int)v, base + (l > 0 ? l - 1 : 0));
}

// insert key (nt, np) into the row-distributed sorted list (lane j holds key j); the largest key
// falls off the last lane.  Keys are (t, prim): the resolve pass finds a key's triangle record by
// its primitive id (rsd_scene.d_prim_rec), so the list carries no record index.
template <int ROW>
__device__ __forceinline__ void row_insert(float& kt, uint32_t& kp, float nt, uint32_t np, int l, int base) {
    const int pos = __popc(row_bits<ROW>(key_less(kt, kp, nt, np), base));
    const float st = __uint_as_float(row_prev<ROW>(__float_as_uint(kt), l, base));
    const uint32_t sp = row_prev<ROW>(kp, l, base);
    if (l == pos) {
        kt = nt; kp = np;
    } else if (l > pos) {
        kt = st; kp = sp;
    }
}
// the same with the key's barycentrics (the fused walk's hit terms)
template <int ROW>
__device__ __forceinline__ void row_insert(float& kt, uint32_t& kp, float& ku, float& kv, float nt, uint32_t np,
                                           float nu, float nv, int l, int base) {
    const int pos = __popc(row_bits<ROW>(key_less(kt, kp, nt, np), base));
    const float st = __uint_as_float(row_prev<ROW>(__float_as_uint(kt), l, base));
    const uint32_t sp = row_prev<ROW>(kp, l, base);
    const float su = __uint_as_float(row_prev<ROW>(__float_as_uint(ku), l, base));
    const float sv = __uint_as_float(row_prev<ROW>(__float_as_uint(kv), l, base));
    if (l == pos) {
        kt = nt; kp = np; ku = nu; kv = nv;
    } else if (l > pos) {
        kt = st; kp = sp; ku = su; kv = sv;
    }
}

// two keys per lane (K = 2 ROW, the specialised walk at K = 16 on 8-lane rows): lane l holds keys 2l (slot 0) and
// 2l + 1 (slot 1) of the sorted list; the insert counts the keys below the new one in both slots and shifts every key
// at or above that position by one (slot 1 <- own slot 0, slot 0 <- the previous lane's slot 1)
template <int ROW>
__device__ __forceinline__ void row_insert2(float& kt0, uint32_t& kp0, float& ku0, float& kv0, float& kt1, uint32_t& kp1,
                                            float& ku1, float& kv1, float nt, uint32_t np, float nu, float nv, int l,
                                            int base) {
    const int pos = __popc(row_bits<ROW>(key_less(kt0, kp0, nt, np), base)) +
                    __popc(row_bits<ROW>(key_less(kt1, kp1, nt, np), base));
    const float st = __uint_as_float(row_prev<ROW>(__float_as_uint(kt1), l, base));
    const uint32_t sp = row_prev<ROW>(kp1, l, base);
    const float su = __uint_as_float(row_prev<ROW>(__float_as_uint(ku1), l, base));
    const float sv = __uint_as_float(row_prev<ROW>(__float_as_uint(kv1), l, base));
    const int i0 = 2 * l, i1 = 2 * l + 1;
    if (i1 == pos) {
        kt1 = nt; kp1 = np; ku1 = nu; kv1 = nv;
    } else if (i1 > pos) {
        kt1 = kt0; kp1 = kp0; ku1 = ku0; kv1 = kv0;
    }
    if (i0 == pos) {
        kt0 = nt; kp0 = np; ku0 = nu; kv0 = nv;
    } else if (i0 > pos) {
        kt0 = st; kp0 = sp; ku0 = su; kv0 = sv;
    }
}

// exclusive prefix sum (and total) of v in [0, 7] over the lanes of a row
template <int ROW>
__device__ __forceinline__ int row_prefix(int v, int l, int base, int& total) {
    const uint32_t below = (1u << l) - 1u;
    int pre = 0;
    total = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const uint32_t m = row_bits<ROW>((v >> b) & 1, base);
        pre += __popc(m & below) << b;
        total += __popc(m) << b;
    }
    return pre;
}

// anyHit -> algorithm (Common.slangh:102-254) over `found` keys in ascending (t, prim) order;
// lane j of the row holds key j's hash `rng` and normalized view depth `z`.  Every lane of
// the row ends with the same depths / cnt / commit.
template <int K, int N, int IMPL = -1>
__device__ __forceinline__ bool sd_algorithm_row(const SDArgs& a, float rng, float z, bool afl, int found,
                                                 int base, float (&depths)[N], uint32_t& cnt, uint32_t& delivered) {
    bool commit = false;
    const uint64_t afm = __ballot(afl);  // bit base + j: key j fails the alpha test
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float rj = __shfl(rng, base + j);
        float zj = __shfl(z, base + j);
        const bool af = (afm >> (base + j)) & 1u;
        if (commit || j >= found) continue;
        delivered++;
        commit = sd_any_hit_impl<N, IMPL>(a, rj, zj, af, depths, cnt);
    }
    return commit;
}

// the same with two keys per lane (row_insert2's layout: key j in lane j / 2, slot j % 2), no alpha-tested keys
template <int K, int N, int IMPL = -1>
__device__ __forceinline__ bool sd_algorithm_row2(const SDArgs& a, float rng0, float z0, float rng1, float z1, int found,
                                                  int base, float (&depths)[N], uint32_t& cnt, uint32_t& delivered) {
    bool commit = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float rj = __shfl((j & 1) ? rng1 : rng0, base + j / 2);
        const float zj = __shfl((j & 1) ? z1 : z0, base + j / 2);
        if (commit || j >= found) continue;
        delivered++;
        commit = sd_any_hit_impl<N, IMPL>(a, rj, zj, false, depths, cnt);
    }
    return commit;
}

// ROW lanes per ray (8 or 16, >= K: lane j of the row holds key j), 64 / ROW rays per wave.
// SPLIT: the walk only collects the K nearest keys and writes them to `keys` (one K-key slot
// per queue slot); sd_resolve_row_kernel runs the algorithm.  Valid when one chunk of K keys
// always decides the texel: Default / KBuffer with MaxCount <= K.  Otherwise the algorithm
// runs here and the walk continues after the K-th key while it has not committed.
// SPEC: the specialised fused walk of the common trace -- the Default reservoir with MaxCount <= K (a
// commit by the K-th key, so no second chunk of keys) and no alpha-tested triangles: the lower-bound
// (useLB) tests, the alpha test, the other implementations and the chunk continuation compile away.
// (Round 6, not kept: deferring a row's leaves to a second pool stack and giving the WAVE separate node steps and
// leaf steps -- every row then tests up to ROW deferred leaves at once -- so that node steps run the box tests alone
// instead of the union of the box and triangle paths of a wave's mixed items.  Same bits, slower at every config:
// configs[1] 67.5 -> 69.1 us, configs[2] 179 -> 223, configs[3] 197 -> 216 (profiles/round6/trace_ab/defer_*).)
template <int K, int N, int ROW, bool SPLIT, bool CNT, int POOL = kPoolCap, bool SPEC = false>
__device__ __forceinline__ void sd_trace_row_body(const SDArgs& a, const float4* __restrict__ queue,
                                                  uint32_t* __restrict__ qctl, uint2* __restrict__ keys,
                                                  uint32_t* sItem, float* sT, uint32_t bid, uint32_t nb, uint32_t qr) {
    // sItem / sT: the rows' LDS pools (kBlock / ROW x POOL entries each); (bid, nb, qr) as sd_trace_queue_body's
    // one key per lane, or (the specialised fused walk, K = 16 on 8-lane rows) two: row_insert2
    static_assert(K <= ROW || (K == 2 * ROW && SPEC && !SPLIT), "one key per lane, or two in the specialised walk");
    constexpr int KPL = K <= ROW ? 1 : 2;
    constexpr int kKthLane = (K - 1) / KPL;  // the lane holding key K - 1 (slot KPL - 1)
    static_assert(kEntryCap <= (uint32_t)ROW, "entry items start one per lane");
    constexpr int kRow = ROW, kRowRays = kBlock / ROW;
    const int lane = threadIdx.x;
    const int l = lane & (kRow - 1), base = lane & ~(kRow - 1), row = lane / kRow;
    uint32_t* pItem = sItem + row * POOL;
    float* pT = sT + row * POOL;
    const uint32_t part = bid % kQueueParts, wavesPerPart = nb / kQueueParts;
    const uint32_t nLong = __hip_atomic_load(&qctl[part], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // (RSD_TRACE_QRANGE, diagnostics: only the longest-first rays, or only the others)
    const uint32_t q0 = qr == 2u ? nLong : 0u;
    const uint32_t count = (qr == 1u ? nLong : nLong + (a.lpt ? __hip_atomic_load(&qctl[kQctlShort + part],
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u)) - q0;
    const rsd_camera& c = a.cam;
    const float DEFAULT = a.normalize ? 1.0f : 3.40282347e+37f;  // Common.slangh:16
    const int soft = a.poolSoft;
    uint32_t slot = 0;  // queue slot of the row's ray
    uint32_t nEnt = 0;  // entry-grid items of the row's ray (0: the root)

    // ---- per-row state (the same value in the 16 lanes of a row unless noted)
    constexpr int kFetch = 0, kTrace = 1, kExit = 2;
    int phase = kFetch;
    bool first = true;
    int x = 0, y = 0;
    RayCtx r;
    float TMin = 0.0f, TMax = 0.0f, cosT = 0.0f;
    float depths[N];
    uint32_t cnt = 0;     // algorithm count (Common.slangh:137)
    bool useLB = false;   // coverage mask / MaxCount > K: keys after (lbT, lbP) only
    float lbT = 0.0f;
    uint32_t lbP = 0u;
    int pool = 0;         // items in this ray's LDS pool
    uint32_t item = kNoItem;  // per lane: the work item of this step
    float kt = INFINITY;  // per lane: key l of the row's sorted k-list
    uint32_t kp = kNoItem;
    float ku = 0.0f, kv = 0.0f;  // per lane: key l's barycentrics (fused walk: the hit terms' inputs)
    float kt2 = INFINITY, ku2 = 0.0f, kv2 = 0.0f;  // KPL = 2: lane l holds keys 2l (kt ...) and 2l + 1 (kt2 ...)
    uint32_t kp2 = kNoItem;
    // ---- statistics (counters build)
    TraceStats st{0u, 0u, 0u};
    uint32_t active = 0, hitsDelivered = 0, maxSteps = 0, raySteps = 0, maxNodes = 0, rayNodes = 0, rayLeaves = 0;
    unsigned long long sumCycles = 0, maxCycles = 0, c0 = 0;

    unsigned long long tFetch = 0, tStep = 0, tResolve = 0, nStep = 0, nLoop = 0, tS0 = 0, tS1 = 0;
    unsigned long long tMem = 0, tComp = 0, tPool = 0, tMark = 0;  // step split (instrumented build)
    unsigned long long tBox = 0, tTri = 0, tB = 0, tT = 0;  // compute split: box tests + sort, triangle tests
    // clock calibration (instrumented build): the first wave's span in s_memtime ticks and in the
    // 100 MHz s_memrealtime ticks converts the step clocks to microseconds (rsd_counters.shader_clock_mhz)
    unsigned long long cal0 = 0, calR0 = 0;
    if constexpr (CNT) {
        if (bid == 0) {
            cal0 = __builtin_amdgcn_s_memtime();
            calR0 = __builtin_amdgcn_s_memrealtime();
        }
    }
    while (__ballot(phase != kExit) != 0ull) {
        if constexpr (CNT) { tS0 = __builtin_amdgcn_s_memtime(); nLoop += lane == 0; }
        const bool fetching = phase == kFetch;
        if (phase == kFetch) {
            uint32_t qi;
            if (first) {  // the static first ray
                qi = a.spread ? (uint32_t)row * wavesPerPart + bid / kQueueParts
                              : (bid / kQueueParts) * (uint32_t)kRowRays + (uint32_t)row;
                first = false;
            } else {
                uint32_t h = 0;
                if (l == 0) h = atomicAdd(&qctl[(qr == 1u ? kQctlHead2 : kQueueParts) + part], 1u);
                qi = wavesPerPart * (uint32_t)kRowRays + __shfl(h, base);
            }
            if (qi >= count) {
                phase = kExit;
            } else {
                slot = queue_slot(a, part, qi + q0, nLong);
                f3 d;
                uint32_t idx;
                // the entry items load with the record (the setup kernel wrote both)
                const uint32_t e = a.entOn && l < (int)kEntryCap ? a.entQ[(size_t)slot * kEntryCap + l] : kNoItem;
                ray_rec_load(queue, slot, d, TMin, TMax, cosT, idx, nEnt);
                x = (int)(idx % (uint32_t)a.sdW);
                y = (int)(idx / (uint32_t)a.sdW);
                ray_setup(r, mk(c.posW[0], c.posW[1], c.posW[2]), d);
#pragma unroll
                for (int i = 0; i < N; ++i) depths[i] = DEFAULT;
                cnt = 0u;
                useLB = false;
                pool = 0;
                // the root node, or the segment's entry-grid frontier (one item per lane)
                item = nEnt ? ((uint32_t)l < nEnt ? e : kNoItem) : (l == 0 ? 0u : kNoItem);
                kt = INFINITY; kp = kNoItem; ku = kv = 0.0f;
                kt2 = INFINITY; kp2 = kNoItem; ku2 = kv2 = 0.0f;
                phase = kTrace;
                if constexpr (CNT) {
                    active += l == 0;
                    raySteps = 0;
                    rayNodes = 0;
                    rayLeaves = 0;
                    c0 = __builtin_amdgcn_s_memtime();
                }
            }
        }
        if constexpr (CNT) {
            tS1 = __builtin_amdgcn_s_memtime();
            if (fetching && l == 0) tFetch += tS1 - tS0;
        }
        if (phase != kTrace) continue;

        // ---- one traversal step of this row
        if constexpr (SPEC) useLB = false;
        const float tlo = useLB ? fmaxf(TMin, lbT) : TMin;
        float kthT = row_bcastf<ROW, kKthLane>(KPL == 2 ? kt2 : kt, l, base);
        uint32_t kthP = row_bcast<ROW, kKthLane>(KPL == 2 ? kp2 : kp, l, base);
        float thi = fminf(TMax, kthT);
        float ck[4];
        uint32_t ci[4];
        int nc = 0;
        // one fetch per step, all loads issued before the first use: a 4-wide node (128 B), or the
        // leaf's triangle records (48 B each; a leaf of 3-4 triangles reads 192 B -- the BVH
        // allocation is padded by 192 B, so the tail loads never leave it)
        const float4* p = a.nodes + (item & kOffMask);
        float4 q[12];
        const bool isLeaf = item != kNoItem && (item & kLeafBit);
        if constexpr (CNT) tMark = __builtin_amdgcn_s_memtime();
        if (item != kNoItem) {
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = p[j];
            if (isLeaf && (item >> 29 & 3u) >= 2u) {
#pragma unroll
                for (int j = 8; j < 12; ++j) q[j] = p[j];
            }
        }
        if constexpr (CNT) {  // the step's fetch latency (the instrumented build waits here)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            if (l == 0) tMem += t - tMark;
            tMark = t;
        }
        if (item != kNoItem && !isLeaf) {
            st.nodes++;
            rayNodes++;
            const uint32_t rf[4] = {__float_as_uint(q[6].x), __float_as_uint(q[6].y), __float_as_uint(q[6].z),
                                    __float_as_uint(q[6].w)};
            const uint32_t cn[4] = {__float_as_uint(q[7].x), __float_as_uint(q[7].y), __float_as_uint(q[7].z),
                                    __float_as_uint(q[7].w)};
            const float lox[4] = {q[0].x, q[0].y, q[0].z, q[0].w}, hix[4] = {q[1].x, q[1].y, q[1].z, q[1].w};
            const float loy[4] = {q[2].x, q[2].y, q[2].z, q[2].w}, hiy[4] = {q[3].x, q[3].y, q[3].z, q[3].w};
            const float loz[4] = {q[4].x, q[4].y, q[4].z, q[4].w}, hiz[4] = {q[5].x, q[5].y, q[5].z, q[5].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float tn;
                const bool h = rf[j] != kNoItem && box_hit(r, lox[j], hix[j], loy[j], hiy[j], loz[j], hiz[j], tlo,
                                                          thi, tn);
                ck[j] = h ? tn : INFINITY;
                ci[j] = h ? make_item(rf[j], cn[j], a.triOff) : kNoItem;
                nc += h;
            }
            // ascending entry distance; misses (INF) sort last
            cswap(ck[0], ci[0], ck[1], ci[1]);
            cswap(ck[2], ci[2], ck[3], ci[3]);
            cswap(ck[0], ci[0], ck[2], ci[2]);
            cswap(ck[1], ci[1], ck[3], ci[3]);
            cswap(ck[1], ci[1], ck[2], ci[2]);
        }
        if constexpr (CNT) { tB = __builtin_amdgcn_s_memtime(); tT = tB; }
        // ---- leaves: every triangle test of the step first (independent dependency chains), then
        //      the row merges the accepted hits into its k-list, one insert each (the merge
        //      re-checks each hit against the current K-th key)
        const uint32_t lc = isLeaf ? ((item >> 29) & 3u) + 1u : 0u;
        if (isLeaf) st.leaves++;
        if (CNT && isLeaf) rayLeaves++;
        if (__ballot(lc != 0u) != 0ull) {
            float tj[4], uj[4], vj[4];
            uint32_t pj[4];
            bool aj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                aj[j] = false;
                tj[j] = 0.0f; uj[j] = 0.0f; vj[j] = 0.0f;
                pj[j] = 0u;
                if ((uint32_t)j < lc) {
                    st.tris++;
                    const float4 v0 = q[3 * j], v1 = q[3 * j + 1], v2 = q[3 * j + 2];
                    float det, t, bu, bv;
                    if (intersect_tri(r, v0, v1, v2, t, bu, bv, det) && t >= TMin && t <= TMax) {
                        const uint32_t prim = __float_as_uint(v0.w);
                        aj[j] = !culled(det, __float_as_uint(v1.w), a.cull) &&
                                (!useLB || key_less(lbT, lbP, t, prim)) && key_less(t, prim, kthT, kthP);
                        tj[j] = t; pj[j] = prim; uj[j] = bu; vj[j] = bv;
                    }
                }
            }
            if constexpr (CNT) tT = __builtin_amdgcn_s_memtime();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                for (uint32_t m = row_bits<ROW>(aj[j], base); m; m &= m - 1u) {
                    const int srcLane = base + __ffs(m) - 1;
                    const float bt = __shfl(tj[j], srcLane);
                    const uint32_t bp = __shfl(pj[j], srcLane);
                    float nu = 0.0f, nv = 0.0f;
                    if constexpr (!SPLIT) {
                        nu = __shfl(uj[j], srcLane);
                        nv = __shfl(vj[j], srcLane);
                    }
                    if (key_less(bt, bp, kthT, kthP)) {
                        if constexpr (SPLIT) row_insert<ROW>(kt, kp, bt, bp, l, base);
                        else if constexpr (KPL == 2) row_insert2<ROW>(kt, kp, ku, kv, kt2, kp2, ku2, kv2, bt, bp, nu, nv, l, base);
                        else row_insert<ROW>(kt, kp, ku, kv, bt, bp, nu, nv, l, base);
                        kthT = row_bcastf<ROW, kKthLane>(KPL == 2 ? kt2 : kt, l, base);
                        kthP = row_bcast<ROW, kKthLane>(KPL == 2 ? kp2 : kp, l, base);
                    }
                }
            }
        }
        thi = fminf(TMax, kthT);
        // ---- push the surviving children, nearest on top
        int keep = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) keep += (j < nc && ck[j] <= thi) ? 1 : 0;  // ck ascending: a prefix
        int total;
        const int pre = row_prefix<ROW>(keep, l, base, total);
        if (pool + total > POOL) {  // unreachable by the pool bound; never write out of range
            if (a.counters && l == 0) atomicAdd(&a.counters[10], 1ull);  // always checked
            keep = max(0, min(keep, POOL - pool - pre));
            total = POOL - pool;
        }
        if constexpr (CNT) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            if (l == 0) {
                tComp += t - tMark;
                tBox += tB - tMark;
                tTri += tT - tB;
            }
            tMark = t;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < keep) {
                const int slot = pool + pre + (keep - 1 - j);
                pItem[slot] = ci[j];
                pT[slot] = ck[j];
            }
        }
        pool += total;
        __builtin_amdgcn_wave_barrier();  // LDS pushes above before the pops below (one wave)
        // ---- pop the next items
        const int take = min(pool, pool <= soft ? kRow : 1);
        item = kNoItem;
        if (l < take) {
            const uint32_t it = pItem[pool - 1 - l];
            const float tt = pT[pool - 1 - l];
            item = tt <= thi ? it : kNoItem;
        }
        pool -= take;
        __builtin_amdgcn_wave_barrier();
        if constexpr (CNT) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (l == 0) tPool += __builtin_amdgcn_s_memtime() - tMark;
            raySteps++;
            const unsigned long long t2 = __builtin_amdgcn_s_memtime();
            if (l == 0) { tStep += t2 - tS1; nStep++; }
            tS1 = t2;
        }
        if (pool > 0 || row_bits<ROW>(item != kNoItem, base) != 0u) continue;

        // ---- traversal done
        if constexpr (SPLIT) {
            // the K nearest keys of the ray -> sd_resolve_row_kernel
            if (l < K) keys[(size_t)slot * K + l] = make_uint2(__float_as_uint(kt), kp);
            phase = kFetch;
            if constexpr (CNT) {
                uint32_t n = rayNodes;
#pragma unroll
                for (int o = ROW / 2; o >= 1; o >>= 1) n += __shfl_xor(n, o);
                maxNodes = max(maxNodes, n);
                maxSteps = max(maxSteps, raySteps);
                const unsigned long long t3 = __builtin_amdgcn_s_memtime();
                if (l == 0) {
                    tResolve += t3 - tS1;
                    sumCycles += t3 - c0;
                    maxCycles = t3 - c0 > maxCycles ? t3 - c0 : maxCycles;
                }
            }
            continue;
        }
        // TraceRay + anyHit -> algorithm (Common.slangh:102-254) over the found keys, in
        // ascending (t, prim) order; lane j prepares key j
        const int found = min(K, __popc(row_bits<ROW>(kp != kNoItem, base)) +
                                     (KPL == 2 ? __popc(row_bits<ROW>(kp2 != kNoItem, base)) : 0));
        // lane j: key j's terms from the (t, barycentrics) its leaf test found -- sd_hit_terms'
        // values bit for bit; the alpha test (alpha scenes only) re-reads the triangle
        float rng = 0.0f, z = 0.0f;
        bool af = false;
        uint32_t delivered = 0;
        if constexpr (KPL == 2) {  // lane l: keys 2l and 2l + 1 (no alpha test: SPEC)
            float rng2 = 0.0f, z2 = 0.0f;
            if (2 * l < found) {
                rng = sd_hash(ku, kv);
                z = kt * cosT;
                if (a.normalize) z = saturate((z - a.cam.nearZ) / (a.cam.farZ - a.cam.nearZ));
            }
            if (2 * l + 1 < found) {
                rng2 = sd_hash(ku2, kv2);
                z2 = kt2 * cosT;
                if (a.normalize) z2 = saturate((z2 - a.cam.nearZ) / (a.cam.farZ - a.cam.nearZ));
            }
            sd_algorithm_row2<K, N, 0>(a, rng, z, rng2, z2, found, base, depths, cnt, delivered);
            if (l == 0) hitsDelivered += delivered;
            if (l == 0) sd_store<N>(a, x, y, depths);
            phase = kFetch;
            continue;
        }
        if (l < found) {
            if (!SPEC && a.alphaTest) {
                sd_hit_terms(a, r, cosT, a.primRec[kp], rng, z, af);
            } else {
                rng = sd_hash(ku, kv);
                z = kt * cosT;  // RayToViewDepth
                if (a.normalize) z = saturate((z - a.cam.nearZ) / (a.cam.farZ - a.cam.nearZ));
            }
        }
        const bool commit = sd_algorithm_row<K, N, SPEC ? 0 : -1>(a, rng, z, af, found, base, depths, cnt, delivered);
        if (l == 0) hitsDelivered += delivered;
        if (CNT && l == 0) tResolve += __builtin_amdgcn_s_memtime() - tS1;
        if (!SPEC && !commit && found == K) {
            // the stream continues after the K-th key: trace the next chunk of K keys
            useLB = true;
            lbT = __shfl(kt, base + K - 1);
            lbP = __shfl(kp, base + K - 1);
            pool = 0;
            item = nEnt ? ((uint32_t)l < nEnt ? a.entQ[(size_t)slot * kEntryCap + l] : kNoItem) : (l == 0 ? 0u : kNoItem);
            kt = INFINITY; kp = kNoItem; ku = kv = 0.0f;
            continue;
        }
        if (l == 0) sd_store<N>(a, x, y, depths);
        phase = kFetch;
        if constexpr (CNT) {
            // per-ray totals: row sums of the lanes' node counts
            uint32_t n = rayNodes;
#pragma unroll
            for (int o = ROW / 2; o >= 1; o >>= 1) n += __shfl_xor(n, o);
            maxNodes = max(maxNodes, n);
            maxSteps = max(maxSteps, raySteps);
            const unsigned long long dc = __builtin_amdgcn_s_memtime() - c0;
            uint32_t nl = rayLeaves;
#pragma unroll
            for (int o = ROW / 2; o >= 1; o >>= 1) nl += __shfl_xor(nl, o);
            if (l == 0) {
                sumCycles += dc;
                maxCycles = dc > maxCycles ? dc : maxCycles;
                if (a.rayLog) {
                    uint32_t* g = a.rayLog + (size_t)slot * 8u;
                    g[0] = (uint32_t)y * (uint32_t)a.sdW + (uint32_t)x;
                    g[1] = raySteps;
                    g[2] = n;
                    g[3] = nl;
                    g[4] = (uint32_t)found;
                    g[5] = (uint32_t)min(dc, 0xffffffffull);
                    g[6] = __float_as_uint(TMax - TMin);
                    g[7] = __float_as_uint(TMin);
                }
            }
        }
    }
    if constexpr (CNT) {
        atomicAdd(&a.counters[1], (unsigned long long)active);
        atomicAdd(&a.counters[2], (unsigned long long)st.nodes);
        atomicAdd(&a.counters[3], (unsigned long long)st.tris);
        atomicAdd(&a.counters[4], (unsigned long long)hitsDelivered);
        atomicMax(&a.counters[5], (unsigned long long)maxNodes);
        atomicMax(&a.counters[6], (unsigned long long)maxSteps);
        atomicAdd(&a.counters[7], sumCycles);
        atomicMax(&a.counters[8], maxCycles);
        atomicAdd(&a.counters[9], (unsigned long long)st.leaves);
        atomicAdd(&a.counters[11], tFetch);
        atomicAdd(&a.counters[12], tStep);
        atomicAdd(&a.counters[13], tResolve);
        atomicAdd(&a.counters[14], nStep);
        atomicAdd(&a.counters[15], nLoop);
        atomicAdd(&a.counters[16], tMem);
        atomicAdd(&a.counters[17], tComp);
        atomicAdd(&a.counters[18], tPool);
        atomicAdd(&a.counters[23], tBox);
        atomicAdd(&a.counters[24], tTri);
        if (bid == 0 && lane == 0) {
            const unsigned long long cal1 = __builtin_amdgcn_s_memtime(), calR1 = __builtin_amdgcn_s_memrealtime();
            atomicMax(&a.counters[21], cal1 - cal0);
            atomicMax(&a.counters[22], calR1 - calR0);
        }
    }
}

// Phase 3 of the split trace: anyHit -> algorithm over the K nearest keys of every live ray
// (one row of ROW lanes per ray, lane j prepares key j), then the SD texel store
// (StochasticDepthMapRT.rt.slang:90-104).  Persistent rows stride over the queue partitions.
template <int K, int N, int ROW, bool RASTER = false>
__global__ void __launch_bounds__(kBlock) sd_resolve_row_kernel(SDArgs a, const float4* __restrict__ queue,
                                                                uint32_t* __restrict__ qctl,
                                                                const uint2* __restrict__ keys) {
    constexpr int kRowRays = kBlock / ROW;
    const int lane = threadIdx.x;
    const int l = lane & (ROW - 1), base = lane & ~(ROW - 1), row = lane / ROW;
    const uint32_t rows = gridDim.x * (uint32_t)kRowRays, me = blockIdx.x * (uint32_t)kRowRays + (uint32_t)row;
    const rsd_camera& c = a.cam;
    const float DEFAULT = a.normalize ? 1.0f : 3.40282347e+37f;  // Common.slangh:16
    uint32_t delivered = 0;
    // live ray g of the frame = partition part, entry g - (rays in partitions < part)
    uint32_t part = 0, partStart = 0, partCount = qctl[0];
    for (uint32_t g = me;; g += rows) {
        while (part < kQueueParts && g >= partStart + partCount) {
            partStart += partCount;
            if (++part < kQueueParts) partCount = qctl[part];
        }
        if (part >= kQueueParts) break;
        {
            const uint32_t slot = part * a.partCap + (g - partStart);
            f3 d;
            float TMin, TMax, cosT;
            uint32_t idx;
            ray_rec_load(queue, slot, d, TMin, TMax, cosT, idx);
            RayCtx r;
            ray_setup(r, mk(c.posW[0], c.posW[1], c.posW[2]), d);
            float rng = 0.0f, z = 0.0f;
            bool valid = false, af = false;
            if (l < K) {
                if constexpr (RASTER) {  // 64-bit (t, prim) keys of the raster walk
                    const unsigned long long k = a.keys64[(size_t)slot * K + l];
                    valid = k != ~0ull;
                    if (valid) sd_hit_terms(a, r, cosT, a.primRec[(uint32_t)k], rng, z, af);
                } else {  // (t bits, prim) keys of the row walk
                    const uint2 k = keys[(size_t)slot * K + l];
                    valid = k.y != kNoItem;
                    if (valid) sd_hit_terms(a, r, cosT, a.primRec[k.y], rng, z, af);
                }
            }
            const int found = __popc(row_bits<ROW>(valid, base));  // keys are sorted: a prefix
            float depths[N];
#pragma unroll
            for (int i = 0; i < N; ++i) depths[i] = DEFAULT;
            uint32_t cnt = 0;
            sd_algorithm_row<K, N>(a, rng, z, af, found, base, depths, cnt, delivered);
            if (l == 0) sd_store<N>(a, (int)(idx % (uint32_t)a.sdW), (int)(idx / (uint32_t)a.sdW), depths);
        }
    }
    if (a.counters && l == 0 && delivered) atomicAdd(&a.counters[4], (unsigned long long)delivered);
}

}  // namespace rsd
