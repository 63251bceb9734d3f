// gbuffer.hip -- primary visibility: the G-buffer that the AO passes and the SD trace read.
//
// Reference: Camera.slang:46-59 (pinhole rays), LinearizeDepth, CompressNormals.ps.slang
// (viewSpace + use16Bit), GBufferRaster (useAlphaTest).  Per pixel the closest (t, prim) hit of the
// pixel-centre primary ray in [near/cos, far/cos], the triangle culling of culled() and the alpha
// test at LOD 0 applied (closest hit with IgnoreHit in the any-hit shader).  rsd_gbuffer writes the
// linear depth t * cos and the view-space face normal packed 2x8 (miss: farZ, 0);
// rsd_gbuffer_raster the non-linear [0,1] depth and the world face normal (miss: 1, 0);
// rsd_gbuffer_world those and the world position (o + d t, 1) of GBufferRaster.posW (miss: 0).
//
// The walk is walk_lane (bvh_traverse.h) with the upper bound min(tmax, best t) and no lower bound
// beyond tmin.
#include <string>
#include <vector>

#include "bvh_traverse.h"
#include "rsd_device.h"
#include "rsd_internal.h"

namespace rsd {

struct GBArgs {
    const float4* nodes;
    const float4* tris;
    uint32_t triOff;
    rsd_camera cam;
    int W, H;
    uint32_t cull;
    float* z;
    uint16_t* n;
    float4* nw;  // raster mode: world face normal (RGBA32F); z then holds non-linear depth
    float4* pw;  // raster mode, or null: world position (RGBA32F, w = 1; miss: 0)
    uint32_t alphaTest;  // the scene has alpha data: alpha test at LOD 0 (GBufferRaster useAlphaTest)
    AlphaData alpha;
};

__global__ void __launch_bounds__(kBlock) gbuffer_kernel(GBArgs a) {
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
    RayCtx r;
    ray_setup(r, mk(c.posW[0], c.posW[1], c.posW[2]), d);
    // the smallest (t, prim) key so far and the index of its triangle record
    float bestT = INFINITY;
    uint32_t bestP = 0xffffffffu, bestTri = 0u;
    int found = 0;  // an int as before: a bool is a lane mask kept with scalar instructions
    const bool alphaOn = a.alphaTest != 0u;
    auto far = [&]() RSD_INLINE_LAMBDA { return fminf(tmax, bestT); };
    auto hit = [&](uint32_t tri, float t, float bu, float bv, float det, float4 v0, float4 v1,
                   float4 v2) RSD_INLINE_LAMBDA {
        if (!(t >= tmin && t <= tmax)) return;
        const uint32_t prim = __float_as_uint(v0.w);
        const uint32_t flags = __float_as_uint(v1.w);
        if (culled(det, flags, a.cull)) return;
        if (!key_less(t, prim, bestT, bestP)) return;
        if (alphaOn && (flags & 4u) && alpha_test_fails(a.alpha, prim, v0, v1, v2, bu, bv, false, t, r.d))
            return;
        bestT = t;
        bestP = prim;
        bestTri = tri;
        found = 1;
    };
    walk_lane<false>(a.nodes, a.triOff, r, tmin, &sstack[lane], &sstackT[lane], far, hit);
    const size_t o = (size_t)y * a.W + x;
    if (!found) {
        if (a.nw) {
            a.z[o] = 1.0f;  // cleared depth
            a.nw[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (a.pw) a.pw[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            a.z[o] = c.farZ;
            a.n[o] = 0;
        }
        return;
    }
    const float zlin = bestT * cosT;
    const float4 v0 = a.tris[3 * bestTri], v1 = a.tris[3 * bestTri + 1], v2 = a.tris[3 * bestTri + 2];
    const f3 e1 = mk(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z);
    const f3 e2 = mk(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z);
    const f3 nw = normalize(cross(e1, e2));
    if (a.nw) {
        a.z[o] = raster_depth(c, zlin);
        a.nw[o] = make_float4(nw.x, nw.y, nw.z, 0.0f);
        if (a.pw) a.pw[o] = make_float4(c.posW[0] + d.x * bestT, c.posW[1] + d.y * bestT, c.posW[2] + d.z * bestT, 1.0f);
        return;
    }
    a.z[o] = zlin;
    const float* m = c.viewMat;
    const f3 nv = mk(m[0] * nw.x + m[1] * nw.y + m[2] * nw.z, m[4] * nw.x + m[5] * nw.y + m[6] * nw.z,
                     m[8] * nw.x + m[9] * nw.y + m[10] * nw.z);
    a.n[o] = (uint16_t)encode_normal_2x8(nv);
}

}  // namespace rsd

using namespace rsd;

extern "C" rsd_status rsd_gbuffer(rsd_scene* scene, const rsd_camera* cam, uint32_t width, uint32_t height,
                                  uint32_t cull_mode, float* d_linear_z, uint16_t* d_normals, rsd_stream stream) {
    if (!scene || !cam || !d_linear_z || !d_normals || width == 0 || height == 0) {
        set_error("rsd_gbuffer: null argument or empty extent");
        return RSD_ERR_INVALID_ARG;
    }
    if (cull_mode > 2) {
        set_error("rsd_gbuffer: cull_mode must be 0, 1 or 2");
        return RSD_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (scene->triangle_count == 0) {
        std::vector<float> z((size_t)width * height, cam->farZ);
        RSD_HIP(hipMemcpyAsync(d_linear_z, z.data(), z.size() * 4, hipMemcpyHostToDevice, s));
        RSD_HIP(hipMemsetAsync(d_normals, 0, (size_t)width * height * 2, s));
        RSD_HIP(hipStreamSynchronize(s));
        return RSD_OK;
    }
    GBArgs a{scene->d_nodes, scene->d_tris, scene->tri_offset, *cam, (int)width, (int)height, cull_mode, d_linear_z,
             d_normals, nullptr, nullptr, scene->d_alpha ? 1u : 0u, scene->alpha};
    dim3 grid((width + kTile - 1) / kTile, (height + kTile - 1) / kTile);
    hipLaunchKernelGGL(gbuffer_kernel, grid, dim3(kBlock), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "gbuffer_kernel launch");
    return RSD_OK;
}

namespace {
rsd_status gbuffer_raster(const char* who, rsd_scene* scene, const rsd_camera* cam, uint32_t width, uint32_t height,
                          uint32_t cull_mode, float* d_depth, float* d_normal_w, float* d_pos_w, hipStream_t s) {
    if (!scene || !cam || !d_depth || !d_normal_w || width == 0 || height == 0 || cull_mode > 2) {
        set_error(std::string(who) + ": invalid argument");
        return RSD_ERR_INVALID_ARG;
    }
    if (scene->triangle_count == 0) {
        std::vector<float> z((size_t)width * height, 1.0f);
        RSD_HIP(hipMemcpyAsync(d_depth, z.data(), z.size() * 4, hipMemcpyHostToDevice, s));
        RSD_HIP(hipMemsetAsync(d_normal_w, 0, (size_t)width * height * 16, s));
        if (d_pos_w) RSD_HIP(hipMemsetAsync(d_pos_w, 0, (size_t)width * height * 16, s));
        RSD_HIP(hipStreamSynchronize(s));
        return RSD_OK;
    }
    GBArgs a{scene->d_nodes, scene->d_tris, scene->tri_offset, *cam, (int)width, (int)height, cull_mode, d_depth,
             nullptr, reinterpret_cast<float4*>(d_normal_w), reinterpret_cast<float4*>(d_pos_w),
             scene->d_alpha ? 1u : 0u, scene->alpha};
    dim3 grid((width + kTile - 1) / kTile, (height + kTile - 1) / kTile);
    hipLaunchKernelGGL(gbuffer_kernel, grid, dim3(kBlock), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? RSD_OK : hip_fail(e, "gbuffer_kernel launch");
}
}  // namespace

extern "C" rsd_status rsd_gbuffer_raster(rsd_scene* scene, const rsd_camera* cam, uint32_t width, uint32_t height,
                                         uint32_t cull_mode, float* d_depth, float* d_normal_w, rsd_stream stream) {
    return gbuffer_raster("rsd_gbuffer_raster", scene, cam, width, height, cull_mode, d_depth, d_normal_w, nullptr,
                          (hipStream_t)stream);
}

extern "C" rsd_status rsd_gbuffer_world(rsd_scene* scene, const rsd_camera* cam, uint32_t width, uint32_t height,
                                        uint32_t cull_mode, float* d_depth, float* d_normal_w, float* d_pos_w,
                                        rsd_stream stream) {
    if (!d_pos_w) {
        set_error("rsd_gbuffer_world: invalid argument");
        return RSD_ERR_INVALID_ARG;
    }
    return gbuffer_raster("rsd_gbuffer_world", scene, cam, width, height, cull_mode, d_depth, d_normal_w, d_pos_w,
                          (hipStream_t)stream);
}
