// depth_peel.hip -- the DepthPeeling pass: the second depth layer that SVAO's DualDepth
// primary mode reads (svao_math.h evalDualVisibility, rsd_svao_params.d_depth2).
//
// Reference: DepthPeeling.3d.slang:16-28 (`if (depth <= prev + minSeparationDistance) discard;`
// over a rasterisation of the scene into a depth buffer cleared to 1) and DepthPeeling.cpp:91-115,
// restated for the ray-cast raster of this library like GBufferRaster is (sd_trace.hip
// gbuffer_kernel): per pixel the pixel-centre primary ray, interval [near/cos, far/cos], the
// triangle culling of culled() and the alpha test at LOD 0.  A hit at parameter t has the linear
// depth zlin = t * cos; it is DISCARDED iff zlin <= prev + minSeparationDistance (a NaN threshold
// discards nothing, +inf discards everything), and the surviving hit with the smallest (t, prim)
// key is the pixel's second layer.
//
// The walk is a closest-hit traversal of its own over the pieces of bvh_traverse.h.  What it adds
// to the G-buffer's walk is a per-lane LOWER bound: no surviving hit lies in front of
// tlo ~ (prev + minSeparationDistance) / cos, so child boxes that end before tlo are never pushed
// or fetched.  tlo is conservative (pulled below the exact bound) and only prunes boxes; every
// triangle hit is still judged by the exact predicate above.
#include "bvh_traverse.h"
#include "rsd_device.h"
#include "rsd_internal.h"

namespace rsd {

struct PeelArgs {
    const float4* nodes;  // BVH base (wide nodes, then triangle records)
    uint32_t triOff;
    rsd_camera cam;
    int W, H;
    uint32_t cull;
    const float* prev;  // linear depth of the first layer, W x H
    float minSep;
    uint32_t linearOut;  // 1: zlin, cleared farZ (Renderer.depth2); 0: non-linear [0,1] depth, cleared 1
    float* out;
    uint32_t alphaTest;
    AlphaData alpha;
};

// Closest (t, prim) hit with tmin <= t <= tmax and t * cosT > thr; culling and the LOD-0 alpha test
// applied.  tlo <= every such t: it prunes child boxes only.  Children are visited nearest-first,
// the others wait on the per-lane LDS stack (private overflow) with their entry distance and are
// dropped unfetched once the best hit is nearer than their box.
__device__ __forceinline__ bool peel_closest(const float4* __restrict__ bvh, uint32_t triOff, const RayCtx& r,
                                             float tmin, float tmax, float tlo, float cosT, float thr, uint32_t cull,
                                             KList<1>& kl, uint32_t* __restrict__ ldsItem,
                                             float* __restrict__ ldsT, bool alphaOn, const AlphaData& alpha) {
    kl.clear();
    uint32_t spillItem[kStackTotal - kLdsStack];
    float spillT[kStackTotal - kLdsStack];
    int sp = 0;
    bool found = false;
    uint32_t item = 0;  // root node
    while (true) {
        const float4* p = bvh + (item & kOffMask);
        float4 q[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) q[j] = p[j];
        uint32_t next = kNoItem;
        if (item & kLeafBit) {
            const uint32_t cnt = ((item >> 29) & 3u) + 1u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((uint32_t)j >= cnt) continue;
                float t, bu, bv, det;
                if (!intersect_tri(r, q[3 * j], q[3 * j + 1], q[3 * j + 2], t, bu, bv, det)) continue;
                if (!(t >= tmin && t <= tmax)) continue;
                const uint32_t prim = __float_as_uint(q[3 * j].w);
                const uint32_t flags = __float_as_uint(q[3 * j + 1].w);
                if (culled(det, flags, cull)) continue;
                const float zlin = t * cosT;
                if (zlin <= thr) continue;  // DepthPeeling.3d.slang:26-27
                if (!key_less(t, prim, kl.t[0], kl.p[0])) continue;
                if (alphaOn && (flags & 4u) &&
                    alpha_test_fails(alpha, prim, q[3 * j], q[3 * j + 1], q[3 * j + 2], bu, bv, false, t, r.d))
                    continue;
                kl.insert(t, prim, 0u);
                found = true;
            }
        } else {
            const float thi = fminf(tmax, kl.t[0]);
            const uint4 rf = make_uint4(__float_as_uint(q[6].x), __float_as_uint(q[6].y), __float_as_uint(q[6].z),
                                        __float_as_uint(q[6].w));
            const uint4 ct = make_uint4(__float_as_uint(q[7].x), __float_as_uint(q[7].y), __float_as_uint(q[7].z),
                                        __float_as_uint(q[7].w));
            float k0, k1, k2, k3;
            bool h0 = rf.x != kNoItem && box_hit(r, q[0].x, q[1].x, q[2].x, q[3].x, q[4].x, q[5].x, tlo, thi, k0);
            bool h1 = rf.y != kNoItem && box_hit(r, q[0].y, q[1].y, q[2].y, q[3].y, q[4].y, q[5].y, tlo, thi, k1);
            bool h2 = rf.z != kNoItem && box_hit(r, q[0].z, q[1].z, q[2].z, q[3].z, q[4].z, q[5].z, tlo, thi, k2);
            bool h3 = rf.w != kNoItem && box_hit(r, q[0].w, q[1].w, q[2].w, q[3].w, q[4].w, q[5].w, tlo, thi, k3);
            auto mkitem = [&](uint32_t ref, uint32_t cnt) {
                return cnt ? (kLeafBit | ((cnt - 1u) << 29) | (triOff + 3u * ref)) : 8u * ref;
            };
            uint32_t c0 = h0 ? mkitem(rf.x, ct.x) : kNoItem, c1 = h1 ? mkitem(rf.y, ct.y) : kNoItem;
            uint32_t c2 = h2 ? mkitem(rf.z, ct.z) : kNoItem, c3 = h3 ? mkitem(rf.w, ct.w) : kNoItem;
            // order by the entry distance into [tlo, ...): a box the ray is already inside at tlo
            // is as near as any other such box
            k0 = h0 ? fmaxf(k0, tlo) : INFINITY;
            k1 = h1 ? fmaxf(k1, tlo) : INFINITY;
            k2 = h2 ? fmaxf(k2, tlo) : INFINITY;
            k3 = h3 ? fmaxf(k3, tlo) : INFINITY;
            cswap(k0, c0, k1, c1);
            cswap(k2, c2, k3, c3);
            cswap(k0, c0, k2, c2);
            cswap(k1, c1, k3, c3);
            cswap(k1, c1, k2, c2);
#define RSD_PEEL_PUSH(c, k)                                                          \
    if ((c) != kNoItem) {                                                            \
        if (sp < kLdsStack) { ldsItem[sp * kBlock] = (c); ldsT[sp * kBlock] = (k); } \
        else { spillItem[sp - kLdsStack] = (c); spillT[sp - kLdsStack] = (k); }      \
        ++sp;                                                                        \
    }
            RSD_PEEL_PUSH(c3, k3)
            RSD_PEEL_PUSH(c2, k2)
            RSD_PEEL_PUSH(c1, k1)
#undef RSD_PEEL_PUSH
            next = c0;
        }
        if (next == kNoItem) {
            const float thi = fminf(tmax, kl.t[0]);
            while (sp > 0) {
                --sp;
                const uint32_t it = sp < kLdsStack ? ldsItem[sp * kBlock] : spillItem[sp - kLdsStack];
                const float tt = sp < kLdsStack ? ldsT[sp * kBlock] : spillT[sp - kLdsStack];
                if (tt <= thi) { next = it; break; }
            }
            if (next == kNoItem) break;
        }
        item = next;
    }
    return found;
}

__global__ void __launch_bounds__(kBlock) depth_peel_kernel(PeelArgs a) {
    __shared__ uint32_t sstack[kLdsStack * kBlock];
    __shared__ float sstackT[kLdsStack * kBlock];
    const int lane = threadIdx.x;
    const int x = blockIdx.x * kTile + (lane & (kTile - 1));
    const int y = blockIdx.y * kTile + (lane / kTile);
    if (x >= a.W || y >= a.H) return;
    const rsd_camera& c = a.cam;
    // the primary ray of gbuffer_kernel (Camera.slang:46-59, camera jitter applied)
    const f3 wn = normalize(mk(c.W[0], c.W[1], c.W[2]));
    const f3 d = normalize(cam_dir(c, ((float)x + 0.5f) / (float)a.W + -c.jitterX,
                                   ((float)y + 0.5f) / (float)a.H + c.jitterY));
    const float cosT = dot(wn, d);
    const float invCos = 1.0f / cosT;
    const float tmin = c.nearZ * invCos, tmax = c.farZ * invCos;
    const size_t o = (size_t)y * a.W + x;
    const float thr = a.prev[o] + a.minSep;
    // A survivor has RN(t * cosT) > thr, hence t >= (thr / cosT)(1 - 2^-24).  The quotient and its
    // scaling below round twice more (2^-24 each), so scaling by 1 - 2^-20 keeps tlo under every
    // survivor's t with room to spare (thr normal; a denormal thr lies below tmin anyway).
    // thr <= 0 or NaN: no hit of [tmin, tmax] is discarded.  thr = +inf: tlo = +inf, no box is entered.
    float tlo = tmin;
    if (thr > 0.0f) tlo = fmaxf(tmin, (thr / cosT) * (1.0f - 0x1p-20f));
    RayCtx r;
    ray_setup(r, mk(c.posW[0], c.posW[1], c.posW[2]), d);
    KList<1> kl;
    const bool found = peel_closest(a.nodes, a.triOff, r, tmin, tmax, tlo, cosT, thr, a.cull, kl, &sstack[lane],
                                    &sstackT[lane], a.alphaTest != 0u, a.alpha);
    if (!found) {
        a.out[o] = a.linearOut ? c.farZ : 1.0f;  // no second layer: the cleared depth buffer
        return;
    }
    const float zlin = kl.t[0] * cosT;
    // D3D-style [0,1] depth of a right-handed perspective, as GBufferRaster.depth
    a.out[o] = a.linearOut ? zlin : c.farZ * (zlin - c.nearZ) / (zlin * (c.farZ - c.nearZ));
}

__global__ void depth_peel_clear_kernel(float* __restrict__ out, uint32_t n, float v) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v;
}

}  // namespace rsd

using namespace rsd;

extern "C" rsd_status rsd_depth_peel(rsd_scene* scene, const rsd_camera* cam, uint32_t width, uint32_t height,
                                     uint32_t cull_mode, const float* d_prev_linear_z, float min_separation,
                                     uint32_t linear_out, float* d_depth2, rsd_stream stream) {
    if (!scene || !cam || !d_prev_linear_z || !d_depth2 || width == 0 || height == 0) {
        set_error("rsd_depth_peel: null argument or empty extent");
        return RSD_ERR_INVALID_ARG;
    }
    if (cull_mode > 2) {
        set_error("rsd_depth_peel: cull_mode must be 0, 1 or 2");
        return RSD_ERR_INVALID_ARG;
    }
    if (linear_out > 1) {
        set_error("rsd_depth_peel: linear_out must be 0 or 1");
        return RSD_ERR_INVALID_ARG;
    }
    if ((uint64_t)width * height > 0x7fffffffull) {
        set_error("rsd_depth_peel: extent too large");
        return RSD_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (scene->triangle_count == 0) {  // nothing to rasterise: the cleared depth buffer
        const uint32_t n = width * height;
        hipLaunchKernelGGL(depth_peel_clear_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_depth2, n,
                           linear_out ? cam->farZ : 1.0f);
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? RSD_OK : hip_fail(e, "depth_peel_clear_kernel launch");
    }
    PeelArgs a{scene->d_nodes, scene->tri_offset, *cam, (int)width, (int)height, cull_mode, d_prev_linear_z,
               min_separation, linear_out, d_depth2, scene->d_alpha ? 1u : 0u, scene->alpha};
    dim3 grid((width + kTile - 1) / kTile, (height + kTile - 1) / kTile);
    hipLaunchKernelGGL(depth_peel_kernel, grid, dim3(kBlock), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? RSD_OK : hip_fail(e, "depth_peel_kernel launch");
}
