// gbuffer_motion.hip -- the raster-style G-buffer with the motion vectors of moving geometry
// (rsd_gbuffer_motion): rsd_gbuffer_world's depth, world face normal and world position, plus
// GBufferRaster.mvec and the world-space motion of the hit, in one launch and one BVH walk per pixel.
//
// A kernel of its own beside gbuffer.hip's gbuffer_kernel, whose code object stays what it was: the same
// primary ray, the same walk (walk_lane, upper bound min(tmax, best t)), the same closest (t, prim) key, the
// same culling and alpha test at LOD 0, and for depth / normal / posW the same expressions, hence the same
// bits.  What it adds, all after the walk and for the winning hit alone: its barycentrics, three index loads and
// three loads of the previous positions (rsd_scene_track_motion; DynamicData::prev_positions).
//
// The barycentrics are not carried through the walk beside bestT.  That form was built first and is wrong on
// gfx950 with this compiler: with `bestU = bu` in the hit functor, the copy of the functor behind the alpha test
// loses the assignment (the accepting block moves five of the six values; bestU keeps its previous value), so
// every alpha-tested hit came out with bu = 0.  Instead the winning record, which the normal needs anyway, goes
// through intersect_tri once more: the same function of the same bits, hence the walk's own (t, bu, bv), and
// the walk keeps gbuffer_kernel's live registers.
//
// Definition (include/rsd.h rsd_gbuffer_motion, DESIGN.md section 4 "Motion vectors of moving geometry";
// every product and sum rounded to float32 on its own: this file is compiled with -ffp-contract=off like
// the other exact kernels).  Winning hit: record vertices v0, v1, v2, prim = v0.w, barycentrics bu (weighs
// v1) and bv (weighs v2) of intersect_tri:
//   i_j = indices[3 prim + j]      d_j = prev_positions[i_j] - v_j
//   b0 = (1 - bu) - bv             D = (b0 d0 + bu d1) + bv d2
//   P = o + d t (posW)             P_prev = P + D
//   mvec = motion_vector_kernel's projection (post.hip) of P_prev with the previous camera, minus the pixel
//   centre; (2, 2) behind the previous camera;  mvecW = (D, 0);  a miss: mvec = (0, 0), mvecW = 0.
#include <string>
#include <vector>

#include "bvh_traverse.h"
#include "rsd_device.h"
#include "rsd_internal.h"

namespace rsd {

struct GBMotionArgs {
    const float4* nodes;
    const float4* tris;
    uint32_t triOff;
    rsd_camera cam;
    int W, H;
    uint32_t cull;
    float* z;      // non-linear [0, 1] depth
    float4* nw;    // world face normal
    float4* pw;    // world position, or null
    float2* mvec;
    float4* mvecW;  // or null
    uint32_t alphaTest;
    AlphaData alpha;
    const uint32_t* indices;  // the dynamic scene's index buffer
    const float* prevPos;     // float3[vertex_count]: the positions at the last snapshot
    float prevPosW[3];        // the previous camera's position
    float pU[3], pV[3], pW[3];  // its U / |U|^2, V / |V|^2, W / |W|^2 (mvec_prev_axes)
};

__global__ void __launch_bounds__(kBlock) gbuffer_motion_kernel(GBMotionArgs a) {
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
    int found = 0;  // an int, not a bool: a bool is a lane mask kept with scalar instructions
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
        a.z[o] = 1.0f;  // cleared depth
        a.nw[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (a.pw) a.pw[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        a.mvec[o] = make_float2(0.0f, 0.0f);
        if (a.mvecW) a.mvecW[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float zlin = bestT * cosT;
    const float4 v0 = a.tris[3 * bestTri], v1 = a.tris[3 * bestTri + 1], v2 = a.tris[3 * bestTri + 2];
    // the winning hit's barycentrics: the walk's own test of the same record (see the head of this file)
    float tHit, bestU = 0.0f, bestV = 0.0f, detHit;
    if (!intersect_tri(r, v0, v1, v2, tHit, bestU, bestV, detHit)) bestU = bestV = 0.0f;  // cannot happen: it won
    // the motion's loads, once, for the winning hit alone: issued here so that they are in flight while the
    // normal is computed
    const uint32_t i0 = a.indices[3 * (size_t)bestP], i1 = a.indices[3 * (size_t)bestP + 1],
                   i2 = a.indices[3 * (size_t)bestP + 2];
    const float* q0 = a.prevPos + 3 * (size_t)i0;
    const float* q1 = a.prevPos + 3 * (size_t)i1;
    const float* q2 = a.prevPos + 3 * (size_t)i2;
    const f3 d0 = mk(q0[0] - v0.x, q0[1] - v0.y, q0[2] - v0.z);
    const f3 d1 = mk(q1[0] - v1.x, q1[1] - v1.y, q1[2] - v1.z);
    const f3 d2 = mk(q2[0] - v2.x, q2[1] - v2.y, q2[2] - v2.z);
    const f3 e1 = mk(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z);
    const f3 e2 = mk(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z);
    const f3 nw = normalize(cross(e1, e2));
    a.z[o] = raster_depth(c, zlin);
    a.nw[o] = make_float4(nw.x, nw.y, nw.z, 0.0f);
    const f3 P = mk(c.posW[0] + d.x * bestT, c.posW[1] + d.y * bestT, c.posW[2] + d.z * bestT);
    if (a.pw) a.pw[o] = make_float4(P.x, P.y, P.z, 1.0f);
    const float b0 = (1.0f - bestU) - bestV;
    const f3 D = mk((b0 * d0.x + bestU * d1.x) + bestV * d2.x, (b0 * d0.y + bestU * d1.y) + bestV * d2.y,
                    (b0 * d0.z + bestU * d1.z) + bestV * d2.z);
    if (a.mvecW) a.mvecW[o] = make_float4(D.x, D.y, D.z, 0.0f);
    // motion_vector_kernel's projection (post.hip), of P + D
    const float u = ((float)x + 0.5f) / (float)a.W, v = ((float)y + 0.5f) / (float)a.H;
    const f3 rel = mk((P.x + D.x) - a.prevPosW[0], (P.y + D.y) - a.prevPosW[1], (P.z + D.z) - a.prevPosW[2]);
    const float pa = rel.x * a.pU[0] + rel.y * a.pU[1] + rel.z * a.pU[2];
    const float pb = rel.x * a.pV[0] + rel.y * a.pV[1] + rel.z * a.pV[2];
    const float pw = rel.x * a.pW[0] + rel.y * a.pW[1] + rel.z * a.pW[2];
    float2 mv = make_float2(2.0f, 2.0f);
    if (pw > 0.0f) mv = make_float2((pa / pw + 1.0f) * 0.5f - u, (1.0f - pb / pw) * 0.5f - v);
    a.mvec[o] = mv;
}

}  // namespace rsd

using namespace rsd;

extern "C" rsd_status rsd_gbuffer_motion(rsd_scene* scene, const rsd_camera* cam, const rsd_camera* prev_cam,
                                         uint32_t width, uint32_t height, uint32_t cull_mode, float* d_depth,
                                         float* d_normal_w, float* d_pos_w, float* d_mvec, float* d_mvec_w,
                                         rsd_stream stream) {
    if (!scene || !cam || !prev_cam || !d_depth || !d_normal_w || !d_mvec || width == 0 || height == 0 ||
        cull_mode > 2) {
        set_error("rsd_gbuffer_motion: invalid argument");
        return RSD_ERR_INVALID_ARG;
    }
    if (!scene->dyn.prev_positions) {
        set_error("rsd_gbuffer_motion: motion is not tracked (rsd_scene_track_motion)");
        return RSD_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (scene->triangle_count == 0) {
        const size_t n = (size_t)width * height;
        std::vector<float> z(n, 1.0f);
        RSD_HIP(hipMemcpyAsync(d_depth, z.data(), n * 4, hipMemcpyHostToDevice, s));
        RSD_HIP(hipMemsetAsync(d_normal_w, 0, n * 16, s));
        if (d_pos_w) RSD_HIP(hipMemsetAsync(d_pos_w, 0, n * 16, s));
        RSD_HIP(hipMemsetAsync(d_mvec, 0, n * 8, s));
        if (d_mvec_w) RSD_HIP(hipMemsetAsync(d_mvec_w, 0, n * 16, s));
        RSD_HIP(hipStreamSynchronize(s));
        return RSD_OK;
    }
    GBMotionArgs a{};
    a.nodes = scene->d_nodes;
    a.tris = scene->d_tris;
    a.triOff = scene->tri_offset;
    a.cam = *cam;
    a.W = (int)width;
    a.H = (int)height;
    a.cull = cull_mode;
    a.z = d_depth;
    a.nw = reinterpret_cast<float4*>(d_normal_w);
    a.pw = reinterpret_cast<float4*>(d_pos_w);
    a.mvec = reinterpret_cast<float2*>(d_mvec);
    a.mvecW = reinterpret_cast<float4*>(d_mvec_w);
    a.alphaTest = scene->d_alpha ? 1u : 0u;
    a.alpha = scene->alpha;
    a.indices = scene->dyn.indices;
    a.prevPos = scene->dyn.prev_positions;
    for (int k = 0; k < 3; ++k) a.prevPosW[k] = prev_cam->posW[k];
    mvec_prev_axes(*prev_cam, a.pU, a.pV, a.pW);
    dim3 grid((width + kTile - 1) / kTile, (height + kTile - 1) / kTile);
    hipLaunchKernelGGL(gbuffer_motion_kernel, grid, dim3(kBlock), 0, s, a);
    return launch_status("gbuffer_motion_kernel launch");
}
