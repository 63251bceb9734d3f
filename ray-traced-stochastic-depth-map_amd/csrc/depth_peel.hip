// depth_peel.hip -- the DepthPeeling pass: the second depth layer that SVAO's DualDepth
// primary mode reads (svao_math.h evalDualVisibility, rsd_svao_params.d_depth2).
//
// Reference: DepthPeeling.3d.slang:16-28 (`if (depth <= prev + minSeparationDistance) discard;`
// over a rasterisation of the scene into a depth buffer cleared to 1) and DepthPeeling.cpp:91-115,
// restated for the ray-cast raster of this library like GBufferRaster is (gbuffer.hip): per pixel the
// pixel-centre primary ray, interval [near/cos, far/cos], the triangle culling of culled() and the
// alpha test at LOD 0.  A hit at parameter t has the linear depth zlin = t * cos; it is DISCARDED iff
// zlin <= prev + minSeparationDistance (a NaN threshold discards nothing, +inf discards everything),
// and the surviving hit with the smallest (t, prim) key is the pixel's second layer.
//
// The walk is walk_lane (bvh_traverse.h) with the upper bound min(tmax, best t), as in the G-buffer
// kernel.  What the peel adds is a per-lane LOWER bound: no surviving hit lies in front of
// tlo ~ (prev + minSeparationDistance) / cos, so child boxes that end before tlo are never pushed
// or fetched, and the children are ordered by their entry distance into [tlo, ...) (CLAMP_KEYS).
// tlo is conservative (pulled below the exact bound) and only prunes boxes; every triangle hit is
// still judged by the exact predicate above.
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

__global__ void __launch_bounds__(kBlock) depth_peel_kernel(PeelArgs a) {
    __shared__ uint32_t sstack[kLdsStack * kBlock];
    __shared__ float sstackT[kLdsStack * kBlock];
    const int lane = threadIdx.x;
    const int x = blockIdx.x * kTile + (lane & (kTile - 1));
    const int y = blockIdx.y * kTile + (lane / kTile);
    if (x >= a.W || y >= a.H) return;
    const rsd_camera& c = a.cam;
    f3 d;
    float cosT, tmin, tmax;
    primary_ray(c, x, y, a.W, a.H, d, cosT, tmin, tmax);
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
    // the smallest surviving (t, prim) key so far
    float bestT = INFINITY;
    uint32_t bestP = 0xffffffffu;
    bool found = false;
    const bool alphaOn = a.alphaTest != 0u;
    auto far = [&]() RSD_INLINE_LAMBDA { return fminf(tmax, bestT); };
    auto hit = [&](uint32_t, float t, float bu, float bv, float det, float4 v0, float4 v1,
                   float4 v2) RSD_INLINE_LAMBDA {
        if (!(t >= tmin && t <= tmax)) return;
        const uint32_t prim = __float_as_uint(v0.w);
        const uint32_t flags = __float_as_uint(v1.w);
        if (culled(det, flags, a.cull)) return;
        const float zlin = t * cosT;
        if (zlin <= thr) return;  // DepthPeeling.3d.slang:26-27
        if (!key_less(t, prim, bestT, bestP)) return;
        if (alphaOn && (flags & 4u) && alpha_test_fails(a.alpha, prim, v0, v1, v2, bu, bv, false, t, r.d))
            return;
        bestT = t;
        bestP = prim;
        found = true;
    };
    walk_lane<true>(a.nodes, a.triOff, r, tlo, &sstack[lane], &sstackT[lane], far, hit);
    if (!found) {
        a.out[o] = a.linearOut ? c.farZ : 1.0f;  // no second layer: the cleared depth buffer
        return;
    }
    const float zlin = bestT * cosT;
    a.out[o] = a.linearOut ? zlin : raster_depth(c, zlin);
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
