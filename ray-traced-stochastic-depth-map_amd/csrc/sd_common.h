// sd_common.h -- what every kernel of the SD trace shares (the Ray-SD hot path on gfx950: the k-nearest any-hit
// traversal that fills the stochastic depth map): the kernel argument block, the live-ray queue records, the
// any-hit algorithm for one hit and the texel store.
//
// Reference: StochasticDepthMapRT.rt.slang:39-105 (rayGen / anyHit),
//            Common.slangh:65-92 (initRayDesc), :102-254 (algorithm),
//            IntersectionHelpers.slang:109-180 (watertight triangle test),
//            Camera.slang:46-90 (pinhole rays).
//
// Any-hit order.  DXR calls any-hit in an unspecified order.  Here the
// any-hit stream is CANONICAL: ascending (t, primitive id), each triangle at most once.
// The Default reservoir and the KBuffer commit no later than the MAX_COUNT-th hit and a
// commit ends the stream (TMax = t), so the result only depends on the MAX_COUNT nearest
// hits: each ray keeps a sorted k-list of the k nearest (t, prim) keys in VGPRs, prunes
// the traversal with the k-th key exactly like a DXR commit shrinks TMax, and runs the
// reference algorithm over the sorted list afterwards.  The coverage-mask variant (no
// count bound) continues in chunks of k keys after the last one processed.  The result is
// independent of the BVH and of the traversal order -- the property the CPU oracle checks.
// (The two traversal-order streams, walks 3 and 5, are the exceptions and say so.)
//
// Shape of a trace.  The BVH is 4-wide: 128-B {child boxes, refs} node records, then 48-B triangle records, a
// whole leaf (<= 4) fetched before it is tested (bvh_traverse.h).  The setup evaluates every texel's ray once,
// stores DEFAULT_DEPTH where the interval is empty and appends the live rays to a compact queue split in
// kQueueParts partitions (the longest rays at a partition's front); one of the walks then drains the queue with
// persistent waves.  sd_plan (host only) decides which setup, which walk and every grid; the launchers of
// sd_launch.h branch on its fields and nothing else.
//
//   sd_setup.hip           ray_table_kernel, and the setup: sd_setup_kernel (one pass) or sd_classify_kernel +
//                          sd_live_kernel (two passes), with the ray, the entry-grid lookup and the queue append
//   sd_quad.h              a quad of 4 lanes per ray, depth-first: the DPP quad exchanges, QuadKeys, the walk's body
//   sd_walk_quad.hip       walk 0 (sd_trace_queue_kernel) and walk 3, its traversal-order stream
//   sd_row.h               a row of 8 / 16 lanes per ray, up to a row of items per step: the row exchanges, the
//                          walk's body, and the resolve kernel of the walks that only collect keys
//   sd_walk_row.hip        walks 1 (fused) and 2 (split: keys, then sd_resolve_row_kernel)
//   sd_walk_hybrid.hip     walk 6: row blocks over the longest-first rays, quad blocks over the rest
//   sd_walk_wavefront.hip  walk 5, the row walk's traversal-order stream
//   sd_walk_raster.hip     walk 4: triangles projected onto the texel grid, then sd_resolve_row_kernel
//   sd_trace.hip           host only: workspaces, SDArgs from the plan, the launch sequence, the C ABI
#pragma once
#include "bvh_traverse.h"
#include "entry_grid.h"
#include "rsd_device.h"
#include "rsd_internal.h"

namespace rsd {

// (the queue-control words kQctl*, the workgroup shapes and the other launch-geometry constants: sd_plan.h)
struct SDArgs {
    const float4* nodes;  // BVH base (wide nodes, then triangle records)
    const float4* tris;   // = nodes + triOff
    uint32_t triOff;
    rsd_camera cam;
    const float* linearZ;
    int zW, zH;
    const uint32_t* rayMin;
    const uint32_t* rayMax;
    float* sd;
    int sdW, sdH;
    int guard;
    uint32_t impl, maxCount, jitter, normalize, rayInterval, cull;
    float alpha;
    const int32_t* lutIdx;  // coverage mask: stratified indices [N+1]
    const uint32_t* lut;    // coverage mask: look-up table [2^N]
    unsigned long long* counters;
    uint32_t partCap;  // live-ray queue: capacity of one partition
    // screen-band sharding: the 8-row tile rows t = bandStart + k * bandStep, k < bandN (an
    // interleaved band: start = index, step = count; a contiguous row range: step = 1)
    int bandStart, bandStep, bandN;
    int poolSoft;      // row traversal: above this many pooled items a row pops one item per step
    const float* rayTab;  // per-column / per-row ray terms (ray_table_kernel), see sd_ray
    uint32_t deadFast;    // setup may classify rayMin == asuint(FLT_MAX) texels as dead directly
    uint32_t* qctlNext;   // the other queue-control buffer, zeroed by the setup kernel
    uint32_t consume;     // RSD_SD_CONSUME_INTERVALS: setup resets every texel's interval after use
    uint32_t* rayMinW;    // writable aliases of rayMin / rayMax (consume only)
    uint32_t* rayMaxW;
    uint32_t alphaTest;   // USE_ALPHA_TEST and the scene has alpha data
    AlphaData alphaData;  // spread = RAY_CONE_SPREAD
    uint32_t f16;         // Use16Bit: the map is R16F / RG16F / RGBA16F (N <= 4)
    // raster walk (RSD_WALK_RASTER): per-texel queue slot (-1: no live ray), per-8x8-tile view-depth
    // range of its live rays, the K-key lists of the live rays (64-bit (t bits, prim) keys), the
    // prim -> triangle record map, and the camera projection onto the SD texel grid
    uint32_t raster, keysK, nTris;
    int32_t* slotMap;
    float2* tileRec;
    uint32_t* liveTiles;  // the tiles with live rays (count: qctl[kQctlLiveTiles])
    unsigned long long* keys64;
    const uint32_t* primRec;
    int tilesW;
    float projU[3], projV[3], projW[3];  // U / |U|^2, V / |V|^2, W / |W|^2
    float camWn[3];                      // normalize(W): view depth of a point = dot(P - o, Wn)
    float wClip;                         // near clip in projW units below every valid hit
    // longest-first queue (fused row walk): rays with TMax - TMin > lptLen go to the front of their
    // partition, the others to its back, so the expensive rays are dequeued first
    uint32_t lpt;
    float lptLen;
    // spread (row and quad walks): the static first rays of the persistent waves are dealt row-major over
    // the partition's waves (queue index i -> wave i % waves, row i / waves), so the longest-first rays land
    // one per wave instead of eight to a wave; 0: wave-major (index i -> wave i / rows, row i % rows)
    uint32_t spread;
    uint32_t quadStack;  // entries of each ray's LDS stack in the quad walks (quad_stack_entries)
    uint32_t qrange;     // diagnostics (RSD_TRACE_QRANGE): 0 every ray, 1 the longest-first rays only, 2 the others
    uint32_t hybridRowBlocks;  // hybrid walk: its first blocks run the row walk (sd_trace_hybrid_kernel)
    // two-pass setup (the full-resolution maps): sd_classify_kernel lists the texels pass 1 touched, partition p at
    // touchList[p * touchCap ..), and sd_live_kernel evaluates only those
    uint32_t* touchList;
    uint32_t touchCap;
    uint32_t liveBlocks;  // sd_live_kernel's grid (a multiple of kQueueParts)
    uint32_t rowPrio;          // hybrid walk: issue priority of the row blocks' waves (s_setprio; A/B, RSD_TRACE_ROWPRIO)
    uint32_t prio;             // issue priority of every setup and walk wave (s_setprio; A/B, RSD_TRACE_PRIO)
    // clean tiles (rsd_sd_params.d_tile_state): per 8x8 tile, tileSig when the last trace left every texel it
    // wrote at DEFAULT_DEPTH (0: unknown); such a tile without a live ray is not rewritten
    uint32_t* tileState;
    uint32_t tileSig;
    uint32_t tileCount;  // 8x8 tiles of the map: the texel masks follow the stamps in tileState (2 words per tile)
    // segment entry grid (entry_grid.h, canonical walks): the setup kernel looks up the frontier of
    // each live ray's segment and copies its items to entQ[slot * kEntryCap ..]
    uint32_t entOn;
    const uint4* entSlots;
    const float4* entItems;  // 2 x float4 per entry: {code, lo.xyz} {hi.xyz, 0}
    uint32_t entBits, entProbe;
    int entRmax;
    float entOrigin[3], entExtent;
    uint32_t* entQ;
    // diagnostics (instrumented fused walk, RSD_TRACE_RAYLOG): 8 words per queue slot {texel, steps,
    // nodes, leaves, keys found, clocks, TMax - TMin, TMin}
    uint32_t* rayLog;
    // diagnostics (RSD_SETUP_DIAG, results wrong by design): 1 the setup kernel returns at once (the launch floor of a
    // trace with an empty queue), 2 no texel is live (the setup's streaming part without the live rays' chains)
    uint32_t diag;
};

// queue slot of the qi-th ray of partition part (lpt: the long rays [0, nLong) from the front, the
// short ones from the back)
__device__ __forceinline__ uint32_t queue_slot(const SDArgs& a, uint32_t part, uint32_t qi, uint32_t nLong) {
    const uint32_t base = part * a.partCap;
    return (!a.lpt || qi < nLong) ? base + qi : base + a.partCap - 1u - (qi - nLong);
}

// store, StochasticDepthMapRT.rt.slang:90-104 (Texture2DArray layout [layer][y][x][ch]).
// Use16Bit (StochasticDepthMapRT.cpp:192-198, N <= 4): the typed store converts to binary16,
// round to nearest even (v_cvt_f16_f32; overflow -> inf, e.g. DEFAULT_DEPTH without NORMALIZE).
__device__ __forceinline__ uint32_t f16_bits(float v) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)v);
}
template <int N>
__device__ __forceinline__ void sd_store(const SDArgs& a, int x, int y, const float (&depths)[N]) {
    const size_t plane = sd_plane_texels(a.sdW, a.sdH);
    const size_t o = sd_texel(x, y, a.sdW);
    if constexpr (N <= 4) {
        if (a.f16) {
            if constexpr (N == 1) {
                reinterpret_cast<uint16_t*>(a.sd)[o] = (uint16_t)f16_bits(depths[0]);
            } else if constexpr (N == 2) {
                reinterpret_cast<uint32_t*>(a.sd)[o] = f16_bits(depths[0]) | (f16_bits(depths[1]) << 16);
            } else {
                reinterpret_cast<uint2*>(a.sd)[o] = make_uint2(f16_bits(depths[0]) | (f16_bits(depths[1]) << 16),
                                                               f16_bits(depths[2]) | (f16_bits(depths[3]) << 16));
            }
            return;
        }
    }
    if constexpr (N == 1) {
        a.sd[o] = depths[0];
    } else if constexpr (N == 2) {
        reinterpret_cast<float2*>(a.sd)[o] = make_float2(depths[0], depths[1]);
    } else {
#pragma unroll
        for (int l = 0; l < N / 4; ++l)
            reinterpret_cast<float4*>(a.sd)[l * plane + o] =
                make_float4(depths[4 * l], depths[4 * l + 1], depths[4 * l + 2], depths[4 * l + 3]);
    }
}

// anyHit -> algorithm (Common.slangh:102-254) for ONE delivered hit: hash `rng` of its
// barycentrics, normalized view depth `z`, `af` = the alpha test failed.  Returns the commit
// decision (true: the any-hit shader accepts the hit, DXR TMax = t).
template <int N, int IMPL>
__device__ __forceinline__ bool sd_any_hit_impl(const SDArgs& a, float rng, float z, bool af, float (&depths)[N],
                                                uint32_t& cnt) {
    // IMPL >= 0: the implementation known at compile time (the specialised row walk: 0 = Default)
    if (IMPL < 0 && a.impl == 1u) {  // CoverageMask, Common.slangh:117-131, 189-209
        const int R = (int)floorf(a.alpha * (float)N + rng);
        uint32_t mask = 0u;
        if (R >= N) mask = 0xffffu;
        else if (R != 0) {
            const float rng2 = sd_hash(rng, z);  // hash3D(float3(bary, t))
            const float lo = (float)a.lutIdx[R], hi = (float)a.lutIdx[R + 1];
            mask = a.lut[(int)(lo + rng2 * (hi - lo))];
        }
        if (af) return cnt >= a.maxCount;  // alpha test failed: ignore the hit (count is 0 here)
        float maxT = 0.0f;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if ((mask & (1u << i)) && z < depths[i]) depths[i] = z;
            maxT = hmax(maxT, depths[i]);
        }
        return !(z < maxT);
    } else if (IMPL < 0 && a.impl == 3u) {  // KBuffer, Common.slangh:132-135, 211-232
        if (z >= depths[N - 1]) return true;
        cnt++;
        if (af) return cnt >= a.maxCount;
        const float rayT = z;
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (z < depths[i]) { const float tmp = depths[i]; depths[i] = z; z = tmp; }
        return (depths[N - 1] == rayT) || cnt >= a.maxCount;
    } else {  // Default reservoir, Common.slangh:136-153, 234-247
        uint32_t slot = cnt++;
        if (cnt > (uint32_t)N) slot = (uint32_t)(rng * (float)cnt);
#pragma unroll
        for (int i = 0; i < N; ++i)
            if ((uint32_t)i == slot && !(depths[i] <= z) && !af) depths[i] = z;
        return cnt >= a.maxCount;
    }
}
template <int N>
__device__ __forceinline__ bool sd_any_hit(const SDArgs& a, float rng, float z, bool af, float (&depths)[N],
                                           uint32_t& cnt) {
    return sd_any_hit_impl<N, -1>(a, rng, z, af, depths, cnt);
}

// A live ray in the queue: 2 x 16 B {dir.xyz, TMin} {TMax, cosT, texel, nEnt}; nEnt > 0: the walk starts
// from the nEnt entry-grid items at entQ[slot * kEntryCap] instead of the root
__device__ __forceinline__ void ray_rec_load(const float4* __restrict__ q, uint32_t slot, f3& d, float& TMin,
                                             float& TMax, float& cosT, uint32_t& texel, uint32_t& nEnt) {
    const float4 r0 = q[2u * slot], r1 = q[2u * slot + 1u];
    d = mk(r0.x, r0.y, r0.z);
    TMin = r0.w;
    TMax = r1.x;
    cosT = r1.y;
    texel = __float_as_uint(r1.z);
    nEnt = __float_as_uint(r1.w);
}
__device__ __forceinline__ void ray_rec_load(const float4* __restrict__ q, uint32_t slot, f3& d, float& TMin,
                                             float& TMax, float& cosT, uint32_t& texel) {
    uint32_t nEnt;
    ray_rec_load(q, slot, d, TMin, TMax, cosT, texel, nEnt);
}

// hash + normalized view depth of the hit (t, triangle record tri) -- the barycentrics come
// from re-running the identical triangle test (Common.slangh:110-115)
// (af: an alpha-masked triangle fails the alpha test at the ray-cone LOD of the hit,
// StochasticDepthMapRT.rt.slang:31-37 + Common.slangh:155-175)
__device__ __forceinline__ void sd_hit_terms(const SDArgs& a, const RayCtx& r, float cosT, uint32_t tri, float& rng,
                                             float& z, bool& af) {
    float t, bu, bv, det;
    const float4 v0 = a.tris[3 * tri], v1 = a.tris[3 * tri + 1], v2 = a.tris[3 * tri + 2];
    intersect_tri(r, v0, v1, v2, t, bu, bv, det);
    rng = sd_hash(bu, bv);
    z = t * cosT;  // RayToViewDepth
    if (a.normalize) z = saturate((z - a.cam.nearZ) / (a.cam.farZ - a.cam.nearZ));
    af = a.alphaTest && (__float_as_uint(v1.w) & 4u) &&
         alpha_test_fails(a.alphaData, __float_as_uint(v0.w), v0, v1, v2, bu, bv, true, t, r.d);
}

}  // namespace rsd
