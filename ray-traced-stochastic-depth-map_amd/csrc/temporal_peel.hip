// temporal_peel.hip -- TemporalDepthPeel, Implementation::Iterative (TemporalDepthPeel.cpp:161-270,
// TemporalDepthPeel.ps.slang:319-425): the second depth layer of DualDepth SVAO without scene access.
// The pixel's view ray behind the visible surface, from depth + minSeparationDist to farZ, is taken
// into the previous frame, clipped to its screen, and bisected against the previous frame's second
// layer; the best sample comes back through prevViewToCurView.  One lane per pixel, the post passes'
// 64 x 4 workgroups; the search is a chain of up to maxIterations dependent 2 x 2 gathers.
//
// Numerics: rsd_device.h contract (no contraction, correctly rounded / and sqrt, denormals kept);
// no fast variant -- the exact SVAO kernels consume this depth.  librsd's definitions where HLSL
// leaves things open are in DESIGN.md section 2 "TemporalDepthPeel"; the kernel restates the shader
// literally, quirks included:
//   - the clip moves minUV / maxUV but minZ / maxZ stay those of the unclipped ends (:346, :416);
//   - GetTexelPointWeight's second loop starts at 1 (:202): the nearest texel is lost when it is
//     component 0, and depthPoint is then 0;
//   - the clip's result is ignored: a ray wholly off the previous screen is searched all the same.
// r1, the search over gPrevDepth (:417), never reaches the output and is not computed.
#include "../../include/rsd_graph.h"
#include "rsd_device.h"
#include "rsd_internal.h"

namespace rsd {
namespace {

constexpr int kClipRounds = 8;  // :61 "max number of iterations = 4"; capped, never unbounded

struct PeelArgs {
    const float* z;
    const float* prev2;
    float* out;
    int W, H;
    float c2p[16], p2c[16];  // curViewToPrevView, prevViewToCurView, row-major
    float isx, isy;          // imageScale (:131), evaluated once on the host
    float farZ, sep;
    int maxIter;
};

// ComputeRegionCode (:39-54): LEFT 1, RIGHT 2, BOTTOM 4, TOP 8; a NaN coordinate is inside
__device__ __forceinline__ uint32_t region_code(float u, float v) {
    uint32_t c = 0u;
    if (u < 0.0f) c |= 1u;
    else if (u > 1.0f) c |= 2u;
    if (v < 0.0f) c |= 4u;
    else if (v > 1.0f) c |= 8u;
    return c;
}

// Texel of the Border-0 sampler: the float row / column index decides, so no out-of-range or NaN
// value is ever converted to an integer
__device__ __forceinline__ float border_texel(const float* __restrict__ t, int W, int H, float fx, float fy, int dx,
                                              int dy) {
    const float cx = fx + (float)dx, cy = fy + (float)dy;
    if (!(cx >= 0.0f && cx <= (float)(W - 1) && cy >= 0.0f && cy <= (float)(H - 1))) return 0.0f;
    return t[(size_t)(int)cy * W + (int)cx];
}

// GetRectifiedDepth (:209-235).  Not tex_sample.h's sampler: the shader's own gather, unquantised fraction, Border 0
__device__ __forceinline__ float rectified_depth(const PeelArgs& a, float u, float v, float farLimit) {
    const float px = u * (float)a.W - 0.5f, py = v * (float)a.H - 0.5f;
    const float fx = floorf(px), fy = floorf(py);
    // Gather components (-,+), (+,+), (+,-), (-,-)
    const float n0 = border_texel(a.prev2, a.W, a.H, fx, fy, 0, 1), n1 = border_texel(a.prev2, a.W, a.H, fx, fy, 1, 1);
    const float n2 = border_texel(a.prev2, a.W, a.H, fx, fy, 1, 0), n3 = border_texel(a.prev2, a.W, a.H, fx, fy, 0, 0);
    const float qx = px - fx, qy = py - fy;  // frac
    const float w0 = (1.0f - qx) * qy, w1 = qx * qy, w2 = qx * (1.0f - qy), w3 = (1.0f - qx) * (1.0f - qy);
    if (n0 > farLimit || n1 > farLimit || n2 > farLimit || n3 > farLimit) {
        // GetTexelPointWeight (:189-207), literally
        int maxIdx = 0;
        float maxVal = w0;
        if (w1 > maxVal) { maxIdx = 1; maxVal = w1; }
        if (w2 > maxVal) { maxIdx = 2; maxVal = w2; }
        if (w3 > maxVal) { maxIdx = 3; maxVal = w3; }
        const float r1 = maxIdx == 1 ? 1.0f : 0.0f, r2 = maxIdx == 2 ? 1.0f : 0.0f, r3 = maxIdx == 3 ? 1.0f : 0.0f;
        return 0.0f * n0 + r1 * n1 + r2 * n2 + r3 * n3;
    }
    return 1.0f / (w0 * (1.0f / n0) + w1 * (1.0f / n1) + w2 * (1.0f / n2) + w3 * (1.0f / n3));  // zlerp(n, w)
}

__global__ void __launch_bounds__(kImageBlockW * kImageBlockH) temporal_peel_kernel(PeelArgs a) {
    const int x = (int)(blockIdx.x * kImageBlockW + threadIdx.x), y = (int)(blockIdx.y * kImageBlockH + threadIdx.y);
    if (x >= a.W || y >= a.H) return;
    const size_t o = (size_t)y * a.W + x;
    const float tu = ((float)x + 0.5f) / (float)a.W, tv = ((float)y + 0.5f) / (float)a.H;  // texC
    const float depth = a.z[o];
    const float limit = depth + a.sep, farLimit = 0.99f * a.farZ;

    // UVToViewSpace(texC, .) at depth + minSeparationDist and at farZ, into the previous view (:334-343)
    const float ndcx = tu * 2.0f - 1.0f, ndcy = (1.0f - tv) * 2.0f - 1.0f;
    float eu[2], ev[2], ez[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float d = k == 0 ? limit : a.farZ;
        const float vx = ndcx * d * a.isx, vy = ndcy * d * a.isy, vz = -d;
        const float qx = a.c2p[0] * vx + a.c2p[1] * vy + a.c2p[2] * vz + a.c2p[3];
        const float qy = a.c2p[4] * vx + a.c2p[5] * vy + a.c2p[6] * vz + a.c2p[7];
        const float qz = a.c2p[8] * vx + a.c2p[9] * vy + a.c2p[10] * vz + a.c2p[11];
        eu[k] = qx / (a.isx * qz) * -0.5f + 0.5f;  // ViewSpaceToUV (:137-142)
        ev[k] = qy / (a.isy * qz) * 0.5f + 0.5f;
        ez[k] = -qz;
    }
    float u0 = eu[0], v0 = ev[0], u1 = eu[1], v1 = ev[1];
    const float minZ = ez[0], maxZ = ez[1];

    // CohenSutherlandClipping (:56-121); its result is not used (:346)
    uint32_t c0 = region_code(u0, v0), c1 = region_code(u1, v1);
    for (int round = 0; round < kClipRounds; ++round) {
        if ((c0 | c1) == 0u || (c0 & c1) != 0u) break;
        const uint32_t co = c0 != 0u ? c0 : c1;
        float cu, cv;
        if (co & 8u) {
            cu = u0 + (u1 - u0) * (1.0f - v0) / (v1 - v0);
            cv = 1.0f;
        } else if (co & 4u) {
            cu = u0 + (u1 - u0) * (0.0f - v0) / (v1 - v0);
            cv = 0.0f;
        } else if (co & 2u) {
            cv = v0 + (v1 - v0) * (1.0f - u0) / (u1 - u0);
            cu = 1.0f;
        } else {
            cv = v0 + (v1 - v0) * (0.0f - u0) / (u1 - u0);
            cu = 0.0f;
        }
        if (co == c0) {
            u0 = cu;
            v0 = cv;
            c0 = region_code(u0, v0);
        } else {
            u1 = cu;
            v1 = cv;
            c1 = region_code(u1, v1);
        }
    }

    // SearchDepth over gPrevDepth2 (:254-317)
    const float uvEps = 0.5f / (float)a.W, zEps = a.sep * 0.001f;
    const float du = u1 - u0, dv = v1 - v0;
    const float rz0 = 1.0f / minZ, rz1 = 1.0f / maxZ;
    float bestZ = 0.0f, bestU = 0.0f, bestV = 0.0f, bestErr = 1e10f;
    float tmin = 0.0f, tmax = 1.0f;
    for (int i = 0; i < a.maxIter; ++i) {
        const float t = (tmin + tmax) * 0.5f;
        const float su = u0 + t * du, sv = v0 + t * dv;
        const float zRef = 1.0f / (rz0 + t * (rz1 - rz0));  // zlerp(minZ, maxZ, t)
        const float d = rectified_depth(a, su, sv, farLimit);
        const float err = fabsf(zRef - d);
        if (err < bestErr) {
            bestZ = d;
            bestU = su;
            bestV = sv;
            bestErr = err;
        }
        const float lu = (u0 + tmin * du) - (u0 + tmax * du), lv = (v0 + tmin * dv) - (v0 + tmax * dv);
        if (sqrtf(lu * lu + lv * lv) < uvEps) break;
        if (fabsf(d - zRef) < zEps) break;
        if (zRef < d) tmin = t;
        else tmax = t;  // a NaN sample lands here
    }

    float res = 0.0f;
    if (bestZ != 0.0f) {  // :303 "no information" otherwise
        const float bx = (bestU * 2.0f - 1.0f) * bestZ * a.isx, by = ((1.0f - bestV) * 2.0f - 1.0f) * bestZ * a.isy;
        const float zc = -(a.p2c[8] * bx + a.p2c[9] * by + a.p2c[10] * -bestZ + a.p2c[11]);
        if (zc > limit && zc < farLimit) res = zc;
    }
    a.out[o] = res > limit ? res : depth;  // :422-423
}

}  // namespace
}  // namespace rsd

using namespace rsd;

extern "C" rsd_status rsd_temporal_depth_peel(const float* d_linear_z, const float* d_prev_depth2, uint32_t width,
                                              uint32_t height, const rsd_camera* cam,
                                              const float cur_view_to_prev_view[16],
                                              const float prev_view_to_cur_view[16], float min_separation,
                                              int32_t max_iterations, float* d_depth2, rsd_stream stream) {
    if (!d_linear_z || !d_prev_depth2 || !cam || !cur_view_to_prev_view || !prev_view_to_cur_view || !d_depth2 ||
        width == 0 || height == 0) {
        set_error("rsd_temporal_depth_peel: invalid argument (null pointer or empty extent)");
        return RSD_ERR_INVALID_ARG;
    }
    if (max_iterations < 0 || max_iterations > 256) {
        set_error("rsd_temporal_depth_peel: max_iterations must be 0..256");
        return RSD_ERR_INVALID_ARG;
    }
    const size_t px = (size_t)width * height;
    if (d_depth2 < d_prev_depth2 + px && d_prev_depth2 < d_depth2 + px) {
        set_error("rsd_temporal_depth_peel: d_depth2 must not alias d_prev_depth2");
        return RSD_ERR_INVALID_ARG;
    }
    PeelArgs a{};
    a.z = d_linear_z;
    a.prev2 = d_prev_depth2;
    a.out = d_depth2;
    a.W = (int)width;
    a.H = (int)height;
    for (int i = 0; i < 16; ++i) {
        a.c2p[i] = cur_view_to_prev_view[i];
        a.p2c[i] = prev_view_to_cur_view[i];
    }
    a.isx = 0.5f * (cam->frameWidth / cam->focalLength);
    a.isy = 0.5f * (cam->frameHeight / cam->focalLength);
    a.farZ = cam->farZ;
    a.sep = min_separation;
    a.maxIter = (int)max_iterations;
    hipLaunchKernelGGL(temporal_peel_kernel, image_grid(width, height), image_block(), 0, (hipStream_t)stream, a);
    return launch_status("temporal_peel_kernel launch");
}
