// sd_raster.hip -- the raster StochasticDepthMap pass: the producer of the stochastic depth map that
// Ray-SD is measured against (SVAO's StochasticDepthImpl::Raster, SVAO.cpp:157-187).
//
// Reference: StochasticDepth.ps.slang:57-126 (the fragment shader), Stencil.ps.slang:3-9 and
// StochasticDepthMap.cpp:189-327: the scene is rasterised into an N-sample MSAA depth target cleared to 1,
// every sample at the pixel centre (StochasticDepthMap.cpp:209-211), and each fragment writes a hashed,
// stratified coverage mask (SV_Coverage) under the LESS depth test.  Restated for the ray-cast raster of
// this library like DepthPeeling is (depth_peel.hip): per SD texel (x, y) of the sd_w x sd_h target the
// pixel-centre primary ray over [near/cos, far/cos]; every triangle that intersect_tri accepts in the
// interval and culled() keeps is one fragment, at parameter t.
//
//   stencil     (depth format with stencil, a mask connected; StochasticDepthMap.cpp:228-236, :286-293): the
//               mask is stencilMask (R8Uint) if given, else rayMax (R32Uint); a texel whose mask value is 0
//               gets no fragment and keeps 1.0 in every sample.
//   alpha test  (AlphaTest, :59-62): the scene's alpha test at LOD 0, as in depth_peel.hip.
//   first layer (:66-70): zlin = t * cosT, z = raster_depth(zlin); discarded iff z <= firstDepth, the
//               non-linear depthMap sampled at uv = ((x + .5) / sd_w, (y + .5) / sd_h).  The sampler follows
//               the reconstructed divisor div = (int)(depth_w / (float)sd_w + .5f) (StochasticDepthMap.cpp:
//               273-283): point for odd div, linear (tex_bilinear) for even div; both with Falcor's
//               Sampler::Desc default address mode, Wrap (Sampler.h:127-129).
//   interval    (RayInterval with rayMin and rayMax given, :73-85): posW = o + d t, every multiply and add
//               rounded separately (rsd_gbuffer_world's posW bits), dist = length(posW - o); discarded iff
//               rayMin != 0 && dist <= asfloat(rayMin), or rayMax != 0 && dist >= asfloat(rayMax).
//   coverage    (:87, :103-117): rng = hash(hash(hash(posW.x, posW.y), posW.z), 1.438943289),
//               R = (int)floor(Alpha N + rng); R >= N: all samples; R == 0: discarded; else
//               rng2 = hash(hash(posW.z, posW.y), posW.x) and mask = lut[(int)(a + rng2 (b - a))] with
//               a = idx[R], b = idx[R + 1] (the stratified table of StochasticDepthMap.cpp:92-115, the one
//               the RT CoverageMask implementation reads).
//   value       (:121-123): v = (zlin - near) / (far - near) with linearize, else z; every sample of the
//               mask takes min(sample, v).
// The rules only discard, so the kernel tests them cheapest first (the alpha test after the interval);
// the result is a per-sample minimum over the surviving fragments and does not depend on their order.
// Default and CoverageMask are this path (the shader's #else branch); ReservoirSampling depends on the
// fragments' arrival order (its counter comment, :21) and KBuffer is no raster implementation: both refused.
//
// One lane per SD texel, 8x8 texels per wave, walk_lane with the LDS stack columns; the kernel is
// templated on N so that the N running minima are registers (static indices only).  Stencilled-out lanes
// store their 1.0 values and leave before the walk.  All hits of the interval are needed: no closest-hit
// shrinking.  Three per-lane bounds prune BOXES only (every hit is still judged by the exact rules):
//
//   thi from rayMax.  A fragment with dist >= rmax is discarded.  posW_i = RN(o_i + RN(d_i t)) and
//     q_i = RN(posW_i - o_i) differ from d_i t by at most u |d_i| t + u (|o_i| + |d_i| t)(1 + u) + u |q_i|
//     <= 3.1 u |d_i| t + 1.1 u |o_i| (u = 2^-24; t >= tmin is normal, no underflow).  Hence
//     |q| >= |d| t (1 - 3.1 u) - 1.1 sqrt(3) u omax, omax = max |o_i|; |d| >= 1 - 5 u for the normalised
//     direction (dot, sqrt, reciprocal, product), and the rounded dot product and square root of length()
//     lose at most 3 u more: dist >= t (1 - 12 u) - 2 u omax.  So t > (rmax + 2 u omax) / (1 - 12 u) implies
//     dist >= rmax, and thi = (rmax + 2^-21 omax)(1 + 2^-18) = (rmax + 8 u omax)(1 + 64 u) lies above that
//     with room for its own three roundings.  rmax NaN or +inf: fminf keeps tmax; rmax <= 0: every fragment
//     is discarded and no box is entered.
//   tlo from rayMin.  A fragment with dist <= rmin is discarded.  The same terms bound dist from above:
//     dist <= t (1 + 12 u) + 2 u omax, so t < (rmin - 2 u omax) / (1 + 12 u) implies dist <= rmin;
//     tlo = (rmin - 2^-21 omax)(1 - 2^-18) lies below that.  rmin NaN or below 2^-21 omax: no bound.
//   tlo from firstDepth.  A survivor has raster_depth(zlin) > fd.  raster_depth rounds five times
//     (zlin - near, far *, far - near, zlin *, /), so its value is at most f(zlin)(1 + 5.1 u) with the exact
//     f(z) = A (1 - near / z), A = far / (far - near); for fd > 0 a survivor therefore has
//     f(zlin) > fd (1 - 2^-20), i.e. zlin > near / (1 - g) with g = fd (1 - 2^-20) / A.  g and the quotient
//     are evaluated in binary64; the bound is used only while 1 - g >= 2^-21, so 1 - g (absolute error
//     below 2^-51) and the quotient keep a relative error below 2^-29, which the scaling by 1 - 2^-20 at the
//     rounding to binary32 covers.  zlin = RN(t cosT) > zl then gives t >= (zl / cosT)(1 - 2^-24): the scaling
//     by 1 - 2^-20 of depth_peel.hip:51-56 covers that and the quotient's rounding.  fd <= 0, NaN, or
//     1 - g < 2^-21 (fd above 1): no bound.
#include "bvh_traverse.h"
#include "rsd_device.h"
#include "rsd_internal.h"

namespace rsd {

struct SdRasterArgs {
    const float4* nodes;  // BVH base (wide nodes, then triangle records)
    uint32_t triOff;
    rsd_camera cam;
    int W, H;  // the SD target
    uint32_t cull;
    const float* depth;  // depthMap: non-linear first layer, dW x dH
    int dW, dH;
    uint32_t bilinear;         // even divisor: linear sampler; odd: point
    const uint32_t* rayMin;    // both null unless RayInterval is on and both were given
    const uint32_t* rayMax;
    const uint8_t* stencil8;   // the stencil mask, R8Uint or R32Uint; both null: no stencil
    const uint32_t* stencil32;
    float covAlpha;  // ALPHA
    uint32_t linearize;
    const int32_t* lutIdx;  // stratified indices [N + 1]
    const uint32_t* lut;    // look-up table [2^N]
    float* out;             // [layer][y][x][min(N, 4)]
    uint32_t alphaTest;
    AlphaData alpha;
};

template <int N>
__device__ __forceinline__ void sd_raster_store(const SdRasterArgs& a, int x, int y, const float (&s)[N]) {
    const size_t plane = sd_plane_texels(a.W, a.H);
    const size_t o = sd_texel(x, y, a.W);
    if constexpr (N == 1) {
        a.out[o] = s[0];
    } else if constexpr (N == 2) {
        reinterpret_cast<float2*>(a.out)[o] = make_float2(s[0], s[1]);
    } else {
#pragma unroll
        for (int l = 0; l < N / 4; ++l)
            reinterpret_cast<float4*>(a.out)[l * plane + o] =
                make_float4(s[4 * l], s[4 * l + 1], s[4 * l + 2], s[4 * l + 3]);
    }
}

template <int N>
__global__ void __launch_bounds__(kBlock) sd_raster_map_kernel(SdRasterArgs a) {
    __shared__ uint32_t sstack[kLdsStack * kBlock];
    __shared__ float sstackT[kLdsStack * kBlock];
    const int lane = threadIdx.x;
    const int x = blockIdx.x * kTile + (lane & (kTile - 1));
    const int y = blockIdx.y * kTile + (lane / kTile);
    if (x >= a.W || y >= a.H) return;
    const size_t o = (size_t)y * a.W + x;
    float s[N];
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = 1.0f;  // the cleared depth target
    // Stencil.ps.slang:5-8
    const bool live = a.stencil8 ? a.stencil8[o] != 0u : (a.stencil32 ? a.stencil32[o] != 0u : true);
    if (!live) {
        sd_raster_store<N>(a, x, y, s);
        return;
    }
    const rsd_camera& c = a.cam;
    f3 d;
    float cosT, tmin, tmax;
    primary_ray(c, x, y, a.W, a.H, d, cosT, tmin, tmax);
    // depthBuffer.Sample(S, posH.xy * INV_RESOLUTION), StochasticDepth.ps.slang:68
    const float u = ((float)x + 0.5f) / (float)a.W, v = ((float)y + 0.5f) / (float)a.H;
    float fd;
    if (a.bilinear) {
        fd = tex_bilinear(a.depth, a.dW, a.dH, u, v, true);
    } else {
        const int ix = tex_addr((int)floorf(u * (float)a.dW), a.dW, true);
        const int iy = tex_addr((int)floorf(v * (float)a.dH), a.dH, true);
        fd = a.depth[(size_t)iy * a.dW + ix];
    }
    const uint32_t iMin = a.rayMin ? a.rayMin[o] : 0u;
    const uint32_t iMax = a.rayMax ? a.rayMax[o] : 0u;
    const float rmin = asfloat(iMin), rmax = asfloat(iMax);
    // box bounds (file header): every hit is still judged by the exact rules below
    const float omax = fmaxf(fmaxf(fabsf(c.posW[0]), fabsf(c.posW[1])), fabsf(c.posW[2]));
    float tlo = tmin, thi = tmax;
    if (iMax != 0u) thi = fminf(tmax, (rmax + 0x1p-21f * omax) * (1.0f + 0x1p-18f));
    if (iMin != 0u) {
        const float b = (rmin - 0x1p-21f * omax) * (1.0f - 0x1p-18f);
        if (b > tlo) tlo = b;
    }
    if (fd > 0.0f) {
        const double g = (double)fd * (1.0 - 0x1p-20) * ((double)c.farZ - (double)c.nearZ) / (double)c.farZ;
        const double h = 1.0 - g;
        if (h >= 0x1p-21) {
            const float zl = (float)((double)c.nearZ / h) * (1.0f - 0x1p-20f);
            const float b = (zl / cosT) * (1.0f - 0x1p-20f);
            if (b > tlo) tlo = b;
        }
    }
    RayCtx r;
    ray_setup(r, mk(c.posW[0], c.posW[1], c.posW[2]), d);
    const bool alphaOn = a.alphaTest != 0u;
    const float range = c.farZ - c.nearZ;
    auto far = [&]() RSD_INLINE_LAMBDA { return thi; };
    auto hit = [&](uint32_t, float t, float bu, float bv, float det, float4 v0, float4 v1,
                   float4 v2) RSD_INLINE_LAMBDA {
        if (!(t >= tmin && t <= tmax)) return;
        const uint32_t prim = __float_as_uint(v0.w);
        const uint32_t flags = __float_as_uint(v1.w);
        if (culled(det, flags, a.cull)) return;
        const float zlin = t * cosT;
        const float z = raster_depth(c, zlin);
        if (z <= fd) return;  // StochasticDepth.ps.slang:69-70
        const f3 pw = mk(c.posW[0] + d.x * t, c.posW[1] + d.y * t, c.posW[2] + d.z * t);
        if (a.rayMin) {  // :75-85
            const float dist = length(mk(pw.x - c.posW[0], pw.y - c.posW[1], pw.z - c.posW[2]));
            if (iMin != 0u && dist <= rmin) return;
            if (iMax != 0u && dist >= rmax) return;
        }
        if (alphaOn && (flags & 4u) && alpha_test_fails(a.alpha, prim, v0, v1, v2, bu, bv, false, t, r.d))
            return;  // :59-62
        const float rng = sd_hash(sd_hash(sd_hash(pw.x, pw.y), pw.z), 1.438943289f);  // :87 hash4D
        const int R = (int)floorf(a.covAlpha * (float)N + rng);                      // :103
        uint32_t mask = 0xffffu;
        if (R < N) {
            if (R == 0) return;  // :116-117
            const float rng2 = sd_hash(sd_hash(pw.z, pw.y), pw.x);  // :111 hash3D(posW.zyx)
            const float lo = (float)a.lutIdx[R], hi = (float)a.lutIdx[R + 1];
            mask = a.lut[(int)(lo + rng2 * (hi - lo))];  // :112-113
        }
        const float val = a.linearize ? (zlin - c.nearZ) / range : z;  // :121-123
#pragma unroll
        for (int i = 0; i < N; ++i)
            if ((mask & (1u << i)) && val < s[i]) s[i] = val;
    };
    walk_lane<true>(a.nodes, a.triOff, r, tlo, &sstack[lane], &sstackT[lane], far, hit);
    sd_raster_store<N>(a, x, y, s);
}

__global__ void sd_raster_clear_kernel(float* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = 1.0f;
}

template <int N>
static void launch_sd_raster(const SdRasterArgs& a, hipStream_t s) {
    dim3 grid((a.W + kTile - 1) / kTile, (a.H + kTile - 1) / kTile);
    hipLaunchKernelGGL(sd_raster_map_kernel<N>, grid, dim3(kBlock), 0, s, a);
}

}  // namespace rsd

using namespace rsd;

extern "C" rsd_status rsd_sd_raster(rsd_scene* scene, const rsd_camera* cam, const rsd_sd_raster_params* p,
                                    const float* d_depth, uint32_t depth_w, uint32_t depth_h,
                                    const uint32_t* d_ray_min, const uint32_t* d_ray_max,
                                    const uint8_t* d_stencil_mask, float* d_sd_out, uint32_t sd_w, uint32_t sd_h,
                                    rsd_stream stream) {
    if (!scene || !cam || !p || !d_depth || !d_sd_out || depth_w == 0 || depth_h == 0 || sd_w == 0 || sd_h == 0) {
        set_error("rsd_sd_raster: null argument or empty extent");
        return RSD_ERR_INVALID_ARG;
    }
    const uint32_t N = p->sample_count;
    if (N != 1 && N != 2 && N != 4 && N != 8 && N != 16) {
        set_error("rsd_sd_raster: sample_count must be 1, 2, 4, 8 or 16");
        return RSD_ERR_INVALID_ARG;
    }
    if (p->cull_mode > 2) {
        set_error("rsd_sd_raster: cull_mode must be 0, 1 or 2");
        return RSD_ERR_INVALID_ARG;
    }
    if (!(p->alpha >= 0.0f && p->alpha <= 1024.0f)) {  // R = floor(alpha N + rng) indexes the stratified table
        set_error("rsd_sd_raster: alpha must be in [0, 1024]");
        return RSD_ERR_INVALID_ARG;
    }
    if (p->implementation > RSD_SD_KBUFFER) {
        set_error("rsd_sd_raster: unknown implementation");
        return RSD_ERR_INVALID_ARG;
    }
    if (p->implementation == RSD_SD_RESERVOIR_SAMPLING || p->implementation == RSD_SD_KBUFFER) {
        set_error("rsd_sd_raster: ReservoirSampling depends on the fragments' arrival order and KBuffer is no raster "
                  "implementation; Default and CoverageMask are supported");
        return RSD_ERR_UNSUPPORTED;
    }
    if ((uint64_t)sd_w * sd_h > 0x7fffffffull || (uint64_t)depth_w * depth_h > 0x7fffffffull) {
        set_error("rsd_sd_raster: extent too large");
        return RSD_ERR_INVALID_ARG;
    }
    if ((uintptr_t)d_sd_out % (4u * (N < 4 ? N : 4u)) != 0) {
        set_error("rsd_sd_raster: d_sd_out must be aligned to its texel size");
        return RSD_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)sd_w * sd_h * N;
    if (scene->triangle_count == 0) {  // nothing to rasterise: the cleared map
        hipLaunchKernelGGL(sd_raster_clear_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_sd_out,
                           total);
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? RSD_OK : hip_fail(e, "sd_raster_clear_kernel launch");
    }
    SdRasterArgs a{};
    a.nodes = scene->d_nodes;
    a.triOff = scene->tri_offset;
    a.cam = *cam;
    a.W = (int)sd_w;
    a.H = (int)sd_h;
    a.cull = p->cull_mode;
    a.depth = d_depth;
    a.dW = (int)depth_w;
    a.dH = (int)depth_h;
    const int div = (int)((float)depth_w / (float)sd_w + 0.5f);  // StochasticDepthMap.cpp:273
    a.bilinear = div % 2 == 0 ? 1u : 0u;
    const bool interval = p->ray_interval && d_ray_min && d_ray_max;
    a.rayMin = interval ? d_ray_min : nullptr;
    a.rayMax = interval ? d_ray_max : nullptr;
    if (p->use_stencil) {  // StochasticDepthMap.cpp:228-230
        if (d_stencil_mask) a.stencil8 = d_stencil_mask;
        else a.stencil32 = d_ray_max;
    }
    a.covAlpha = p->alpha;
    a.linearize = p->linearize ? 1u : 0u;
    a.out = d_sd_out;
    a.alphaTest = (p->alpha_test && scene->d_alpha) ? 1u : 0u;
    a.alpha = scene->alpha;
    rsd_status st = sd_coverage_lut(scene->dev->hip_device, N, &a.lutIdx, &a.lut);
    if (st != RSD_OK) return st;
    switch (N) {
        case 1: launch_sd_raster<1>(a, s); break;
        case 2: launch_sd_raster<2>(a, s); break;
        case 4: launch_sd_raster<4>(a, s); break;
        case 8: launch_sd_raster<8>(a, s); break;
        default: launch_sd_raster<16>(a, s); break;
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? RSD_OK : hip_fail(e, "sd_raster_map_kernel launch");
}
