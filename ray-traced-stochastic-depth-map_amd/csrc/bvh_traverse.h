// bvh_traverse.h -- BVH traversal primitives shared by librsd's ray kernels (the SD trace,
// the primary-visibility G-buffer, the depth peel and the Raytraced secondary mode of SVAO
// pass 2), and walk_lane, the one-ray-per-lane walk of the last three.
//
// Reference: IntersectionHelpers.slang:109-180 (watertight triangle test), the DXR triangle
// culling of the instance flags (Scene.cpp:3446-3452), Camera.slang:46-90 (pinhole rays).
// BVH layout: csrc/bvh_build.h.
#pragma once
#include "rsd_device.h"
#include "../../include/rsd.h"
#include "alpha_test.h"
#include "sd_plan.h"  // kTile, kQueueParts, kBlock

namespace rsd {

// __forceinline__ spelled for a lambda's call operator
#define RSD_INLINE_LAMBDA __attribute__((always_inline))

constexpr int kLdsStack = 16;
constexpr int kStackTotal = 96;        // 4-wide: <= 3 pushes per level, <= 30 levels

struct RayCtx {
    f3 o, d;
    int kx, ky, kz;
    float Sx, Sy, Sz;
    f3 invd, oLo, oHi;  // box test: 1 / d, and o / d for the lo and the hi plane (apart on a clamped axis: ray_setup)
};

__device__ __forceinline__ float comp(f3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

__device__ __forceinline__ void ray_setup(RayCtx& r, f3 o, f3 d) {
    r.o = o;
    r.d = d;
    float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    int axis = 0;
    if (ay > ax && ay > az) axis = 1;
    if (az > ax && az > ay) axis = 2;
    r.kz = axis;
    r.kx = axis == 2 ? 0 : axis + 1;
    r.ky = r.kx == 2 ? 0 : r.kx + 1;
    if (comp(d, r.kz) < 0.0f) { int s = r.kx; r.kx = r.ky; r.ky = s; }
    float dz = comp(d, r.kz);
    r.Sx = comp(d, r.kx) / dz;
    r.Sy = comp(d, r.ky) / dz;
    r.Sz = 1.0f / dz;
    // box test reciprocal: avoid 0 * inf = NaN for axis-parallel rays
    auto safe = [](float v) { return fabsf(v) > 1e-20f ? v : copysignf(1e-20f, v); };
    r.invd = mk(1.0f / safe(d.x), 1.0f / safe(d.y), 1.0f / safe(d.z));
    // box_hit computes a plane's distance as fma(plane, invd, -o * invd).  On a clamped axis (d = 0) a plane through
    // the origin's own coordinate comes out at distance (plane - o) 1e20 = 0 instead of "never": a box that only
    // touches the ray's plane would end at t = 0 and be dropped with the hit on its boundary edge.  There the slab
    // is widened by e = 1e20 (2^-22 |o| + 1e-10): 1e10 at least, beyond every TMax, and four times the rounding of
    // o * invd.  A box whose plane lies within about 4 floats of the origin's coordinate (or within 1e-10 of it) is
    // therefore kept as well: false positives only; a box farther off ends up 1e20 |lo - o| - e away and is
    // rejected as before.  The sign of invd says which plane the ray enters through, so e is folded into the
    // subtrahends of the lo and the hi plane.  Every other axis keeps o * invd itself: box_hit gives the bits it
    // always gave.
    auto planes = [](float o, float d, float invd, float& lo, float& hi) {
        const float c = o * invd;
        const bool clamped = !(fabsf(d) > 1e-20f);
        const float e = fabsf(invd) * (fabsf(o) * 2.384185791015625e-07f + 1e-10f);
        lo = !clamped ? c : (invd > 0.0f ? c + e : c - e);
        hi = !clamped ? c : (invd > 0.0f ? c - e : c + e);
    };
    planes(o.x, d.x, r.invd.x, r.oLo.x, r.oHi.x);
    planes(o.y, d.y, r.invd.y, r.oLo.y, r.oHi.y);
    planes(o.z, d.z, r.invd.z, r.oLo.z, r.oHi.z);
}

// IntersectionHelpers.slang:109-180 -- bit-identical to the oracle (no contraction).
__device__ __forceinline__ bool intersect_tri(const RayCtx& r, float4 a, float4 b, float4 c, float& t, float& bu,
                                              float& bv, float& detOut) {
    f3 A = mk(a.x - r.o.x, a.y - r.o.y, a.z - r.o.z);
    f3 B = mk(b.x - r.o.x, b.y - r.o.y, b.z - r.o.z);
    f3 C = mk(c.x - r.o.x, c.y - r.o.y, c.z - r.o.z);
    const float Akz = comp(A, r.kz), Bkz = comp(B, r.kz), Ckz = comp(C, r.kz);
    const float Ax = comp(A, r.kx) - r.Sx * Akz;
    const float Ay = comp(A, r.ky) - r.Sy * Akz;
    const float Bx = comp(B, r.kx) - r.Sx * Bkz;
    const float By = comp(B, r.ky) - r.Sy * Bkz;
    const float Cx = comp(C, r.kx) - r.Sx * Ckz;
    const float Cy = comp(C, r.ky) - r.Sy * Ckz;
    float U = Cx * By - Cy * Bx;
    float V = Ax * Cy - Ay * Cx;
    float W = Bx * Ay - By * Ax;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {
        double CxBy = (double)Cx * (double)By, CyBx = (double)Cy * (double)Bx;
        U = (float)(CxBy - CyBx);
        double AxCy = (double)Ax * (double)Cy, AyCx = (double)Ay * (double)Cx;
        V = (float)(AxCy - AyCx);
        double BxAy = (double)Bx * (double)Ay, ByAx = (double)By * (double)Ax;
        W = (float)(BxAy - ByAx);
    }
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return false;
    const float det = U + V + W;
    if (det == 0.0f) return false;
    const float Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
    const float T = U * Az + V * Bz + W * Cz;
    const float rcpDet = 1.0f / det;
    t = T * rcpDet;
    bu = V * rcpDet;
    bv = W * rcpDet;
    detOut = det;
    return true;
}

// det > 0 <=> counter-clockwise seen from the ray origin = Falcor front face (unless
// the mesh is frontFaceCW); double-sided disables culling (Scene.cpp:3446-3452).
__device__ __forceinline__ bool culled(float det, uint32_t flags, uint32_t cull) {
    if (cull == 0u || (flags & 1u)) return false;
    const bool front = (det > 0.0f) != ((flags & 2u) != 0u);
    return cull == 1u ? !front : front;
}

// Conservative slab test: entry/exit widened by a relative 1e-5 (and the slab of a clamped axis by ray_setup's e) so
// that a node is skipped only if it cannot hold a reported hit in [tlo, thi].  The oracle restates it bit for bit (o_box4: the traversal and
// wavefront orders are defined through it).
__device__ __forceinline__ bool box_hit(const RayCtx& r, float lox, float hix, float loy, float hiy, float loz,
                                        float hiz, float tlo, float thi, float& tnear) {
    float x0 = fmaf(lox, r.invd.x, -r.oLo.x), x1 = fmaf(hix, r.invd.x, -r.oHi.x);
    float y0 = fmaf(loy, r.invd.y, -r.oLo.y), y1 = fmaf(hiy, r.invd.y, -r.oHi.y);
    float z0 = fmaf(loz, r.invd.z, -r.oLo.z), z1 = fmaf(hiz, r.invd.z, -r.oHi.z);
    float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    float m = 1e-5f * (fabsf(tn) + fabsf(tf));
    tn -= m;
    tf += m;
    tnear = tn;
    return fmaxf(tn, tlo) <= fminf(tf, thi);
}

__device__ __forceinline__ bool key_less(float ta, uint32_t pa, float tb, uint32_t pb) {
    return ta < tb || (ta == tb && pa < pb);
}

struct TraceStats {
    uint32_t nodes, tris, leaves;
};

__device__ __forceinline__ void cswap(float& ta, uint32_t& ra, float& tb, uint32_t& rb) {
    const bool s = tb < ta;
    const float t = ta;
    const uint32_t r = ra;
    ta = s ? tb : ta;
    ra = s ? rb : ra;
    tb = s ? t : tb;
    rb = s ? r : rb;
}

// Work items of the traversal: one 32-bit word.  bit31 = leaf, bits 29-30 = leaf triangle
// count - 1, bits 0-28 = offset in 16-B units from the BVH base (wide nodes and triangle
// records share one allocation).  Every step fetches 12 x 16 B at the item's offset -- a
// 128-B node (+ 64 B ignored) or a whole leaf of <= 4 48-B triangle records -- with the
// same instructions, so a wave whose lanes mix node steps and leaf steps still pays ONE
// memory latency per step.  The SD trace is latency-bound (few active rays, long tails).
constexpr uint32_t kLeafBit = 0x80000000u;
constexpr uint32_t kOffMask = 0x1fffffffu;
constexpr uint32_t kNoItem = 0xffffffffu;

__device__ __forceinline__ uint32_t make_item(uint32_t ref, uint32_t cnt, uint32_t triOff) {
    return cnt ? (kLeafBit | ((cnt - 1u) << 29) | (triOff + 3u * ref)) : 8u * ref;
}

// The per-lane stack of walk_lane: (item, entry distance) pairs, the first kLdsStack of them in the
// lane's column of two LDS arrays of kLdsStack x kBlock words (entry i at [i * kBlock]), the others
// in two private arrays of kStackTotal - kLdsStack words.  The private arrays are not members: their
// variable indices would keep a struct that held them in private memory as a whole, sp included.
struct LaneStack {
    uint32_t* ldsItem;
    float* ldsT;
    uint32_t* spillItem;
    float* spillT;
    int sp;
    __device__ __forceinline__ void push(uint32_t item, float t) {
        if (sp < kLdsStack) { ldsItem[sp * kBlock] = item; ldsT[sp * kBlock] = t; }
        else { spillItem[sp - kLdsStack] = item; spillT[sp - kLdsStack] = t; }
        ++sp;
    }
    // the topmost item whose entry distance is <= thi (those above it are dropped), or kNoItem
    __device__ __forceinline__ uint32_t pop_within(float thi) {
        while (sp > 0) {
            --sp;
            const uint32_t it = sp < kLdsStack ? ldsItem[sp * kBlock] : spillItem[sp - kLdsStack];
            const float tt = sp < kLdsStack ? ldsT[sp * kBlock] : spillT[sp - kLdsStack];
            if (tt <= thi) return it;
        }
        return kNoItem;
    }
};

// One ray per lane through the whole BVH, for the kernels whose lanes walk on their own (the G-buffer,
// the depth peel; svao_rt.hip's trace_ao restates it).  Children whose box meets [tlo, far()] are
// visited nearest-first; the others wait on the stack with their entry distance, and a popped item is
// dropped without a fetch once far() is nearer than its box.
//   ldsItem, ldsT   the lane's columns of the LDS part of its stack (LaneStack).
//   far()   the caller's current upper bound, read at a node before its box tests and before popping.
//   hit(tri, t, bu, bv, det, v0, v1, v2)   every leaf triangle that intersect_tri accepts, in leaf
//           order; tri = index of its record in the triangle array.  The range test, culling, the key
//           comparison, the alpha test and the caller's state are the functor's.
//   CLAMP_KEYS   children are ordered and stacked by fmaxf(entry distance, tlo) instead of the entry
//           distance: with a lower bound inside the scene, a box the ray is already in at tlo is as
//           near as any other such box.
// far and hit are lambdas marked RSD_INLINE_LAMBDA.
template <bool CLAMP_KEYS, class Far, class Hit>
__device__ __forceinline__ void walk_lane(const float4* __restrict__ bvh, uint32_t triOff, const RayCtx& r, float tlo,
                                          uint32_t* __restrict__ ldsItem, float* __restrict__ ldsT, Far far, Hit hit) {
    uint32_t spillItem[kStackTotal - kLdsStack];
    float spillT[kStackTotal - kLdsStack];
    LaneStack stack{ldsItem, ldsT, spillItem, spillT, 0};
    uint32_t item = 0;  // root node
    while (true) {
        const float4* p = bvh + (item & kOffMask);
        float4 q[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) q[j] = p[j];
        uint32_t next = kNoItem;
        if (item & kLeafBit) {
            const uint32_t cnt = ((item >> 29) & 3u) + 1u;
            const uint32_t first = ((item & kOffMask) - triOff) / 3u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((uint32_t)j >= cnt) continue;
                float t, bu, bv, det;
                if (!intersect_tri(r, q[3 * j], q[3 * j + 1], q[3 * j + 2], t, bu, bv, det)) continue;
                hit(first + (uint32_t)j, t, bu, bv, det, q[3 * j], q[3 * j + 1], q[3 * j + 2]);
            }
        } else {
            const float thi = far();
            const uint4 rf = make_uint4(__float_as_uint(q[6].x), __float_as_uint(q[6].y), __float_as_uint(q[6].z),
                                        __float_as_uint(q[6].w));
            const uint4 ct = make_uint4(__float_as_uint(q[7].x), __float_as_uint(q[7].y), __float_as_uint(q[7].z),
                                        __float_as_uint(q[7].w));
            float k0, k1, k2, k3;
            bool h0 = rf.x != kNoItem && box_hit(r, q[0].x, q[1].x, q[2].x, q[3].x, q[4].x, q[5].x, tlo, thi, k0);
            bool h1 = rf.y != kNoItem && box_hit(r, q[0].y, q[1].y, q[2].y, q[3].y, q[4].y, q[5].y, tlo, thi, k1);
            bool h2 = rf.z != kNoItem && box_hit(r, q[0].z, q[1].z, q[2].z, q[3].z, q[4].z, q[5].z, tlo, thi, k2);
            bool h3 = rf.w != kNoItem && box_hit(r, q[0].w, q[1].w, q[2].w, q[3].w, q[4].w, q[5].w, tlo, thi, k3);
            uint32_t c0 = h0 ? make_item(rf.x, ct.x, triOff) : kNoItem;
            uint32_t c1 = h1 ? make_item(rf.y, ct.y, triOff) : kNoItem;
            uint32_t c2 = h2 ? make_item(rf.z, ct.z, triOff) : kNoItem;
            uint32_t c3 = h3 ? make_item(rf.w, ct.w, triOff) : kNoItem;
            k0 = h0 ? (CLAMP_KEYS ? fmaxf(k0, tlo) : k0) : INFINITY;
            k1 = h1 ? (CLAMP_KEYS ? fmaxf(k1, tlo) : k1) : INFINITY;
            k2 = h2 ? (CLAMP_KEYS ? fmaxf(k2, tlo) : k2) : INFINITY;
            k3 = h3 ? (CLAMP_KEYS ? fmaxf(k3, tlo) : k3) : INFINITY;
            cswap(k0, c0, k1, c1);
            cswap(k2, c2, k3, c3);
            cswap(k0, c0, k2, c2);
            cswap(k1, c1, k3, c3);
            cswap(k1, c1, k2, c2);
            if (c3 != kNoItem) stack.push(c3, k3);
            if (c2 != kNoItem) stack.push(c2, k2);
            if (c1 != kNoItem) stack.push(c1, k1);
            next = c0;
        }
        if (next == kNoItem) {
            next = stack.pop_within(far());
            if (next == kNoItem) break;
        }
        item = next;
    }
}

__device__ __forceinline__ f3 cam_dir(const rsd_camera& c, float px, float py) {
    const float ndcx = 2.0f * px + -1.0f;
    const float ndcy = -2.0f * py + 1.0f;
    return mk(ndcx * c.U[0] + ndcy * c.V[0] + c.W[0], ndcx * c.U[1] + ndcy * c.V[1] + c.W[1],
              ndcx * c.U[2] + ndcy * c.V[2] + c.W[2]);
}

// The primary ray through the centre of pixel (x, y) of a W x H image, camera jitter applied
// (Camera.slang:46-59): unit direction d, cosT = its cosine to the view axis, and the camera's
// [nearZ, farZ] as the ray's parameter interval.
__device__ __forceinline__ void primary_ray(const rsd_camera& c, int x, int y, int W, int H, f3& d, float& cosT,
                                            float& tmin, float& tmax) {
    const f3 wn = normalize(mk(c.W[0], c.W[1], c.W[2]));
    d = normalize(cam_dir(c, ((float)x + 0.5f) / (float)W + -c.jitterX, ((float)y + 0.5f) / (float)H + c.jitterY));
    cosT = dot(wn, d);
    const float invCos = 1.0f / cosT;
    tmin = c.nearZ * invCos;
    tmax = c.farZ * invCos;
}

// D3D-style [0,1] depth of a right-handed perspective, as GBufferRaster.depth:
// far (z - near) / (z (far - near))
__device__ __forceinline__ float raster_depth(const rsd_camera& c, float zlin) {
    return c.farZ * (zlin - c.nearZ) / (zlin * (c.farZ - c.nearZ));
}

}  // namespace rsd
