// alpha_test.h -- the alpha test of alpha-masked materials on the device.
//
// Reference: MaterialFactory::alphaTest (Scene/Material/MaterialFactory.slang:124-151),
// StandardMaterial::evalOpacity (Rendering/Materials/StandardMaterial.slang:128-132, the
// base-colour alpha), evalBasicAlphaTest (Scene/Material/AlphaTest.slang:81-84: alpha <
// threshold fails), Scene::computeVertexData (Scene/Scene.slang:444-480: texC and face normal
// interpolation), ray-cone LOD (StochasticDepthMapRT.rt.slang:31-37, TexLODHelpers.slang:97-129,
// ExplicitRayConesLodTextureSampler TextureSampler.slang:81-97; coneTexLODValue is 0 for
// getVertexData).  Sampling (librsd's definition, DESIGN.md "Alpha test"): trilinear over the
// host-built 2x2 box mip chain, wrap addressing, 8 sub-texel bits and 8 LOD-fraction bits;
// log2 evaluated in double and rounded once.  The CPU oracle restates exactly this.
#pragma once
#include "rsd_device.h"
#include "rsd_internal.h"

namespace rsd {

// bilinear of one R8Unorm mip, wrap (tex_sample.h's rule, all four taps)
__device__ __forceinline__ float alpha_bilinear(const uint8_t* __restrict__ lvl, int w, int h, float u, float v) {
    const TexSplit s = tex_split(w, h, u, v);
    return unorm8_bilinear_at(lvl, s, tex_taps(s, w, h, true));
}

// SampleLevel(uv, level): trilinear between the two nearest mips, LOD clamped to the chain
__device__ __forceinline__ float alpha_sample(const AlphaData& A, uint32_t texIndex, float u, float v, float level) {
    const uint4 tx = A.textures[texIndex];
    const int mips = (int)tx.z;
    float lod = level != level ? 0.0f : fminf(fmaxf(level, 0.0f), (float)(mips - 1));
    const TexAxis m = tex_split_axis(lod);  // the LOD fraction has the sampler's 8 bits
    const int l0 = m.i;
    const float qf = m.q, f = m.w;
    size_t off = tx.w;
    int w = (int)tx.x, h = (int)tx.y;
    for (int m = 0; m < l0; ++m) {
        off += (size_t)w * h;
        w = max(1, w >> 1);
        h = max(1, h >> 1);
    }
    const float s0 = alpha_bilinear(A.texels + off, w, h, u, v);
    if (qf == 0.0f || l0 + 1 >= mips) return s0;
    const float s1 = alpha_bilinear(A.texels + off + (size_t)w * h, max(1, w >> 1), max(1, h >> 1), u, v);
    return s0 * (1.0f - f) + s1 * f;
}

// MaterialFactory::alphaTest: true = the hit is discarded.  (bu, bv) = DXR barycentrics;
// lodRayCone: the ray-cone LOD with the hit distance t and direction d, else LOD 0.
__device__ __forceinline__ bool alpha_test_fails(const AlphaData& A, uint32_t prim, float4 v0, float4 v1, float4 v2,
                                                 float bu, float bv, bool lodRayCone, float t, f3 d) {
    const uint32_t mat = A.triMat[prim];
    const float4 m = A.materials[mat];
    const uint32_t tex = __float_as_uint(m.z);
    float alpha = m.y;
    if (tex != 0xffffffffu) {
        const float* uv = A.triUV + 6 * (size_t)prim;
        const float b0 = 1.0f - bu - bv;  // TriangleHit::getBarycentricWeights
        float tu = uv[0] * b0, tv = uv[1] * b0;
        tu += uv[2] * bu;
        tv += uv[3] * bu;
        tu += uv[4] * bv;
        tv += uv[5] * bv;
        float level = 0.0f;
        if (lodRayCone) {
            const uint4 tx = A.textures[tex];
            const f3 e1 = mk(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z), e2 = mk(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z);
            const f3 n = normalize(cross(e1, e2));
            const float width = A.spread * t + 0.0f;  // RayCone(0, spread).propagateDistance(t)
            const float lambda = 0.0f + (float)log2((double)(fabsf(width) / fabsf(dot(d, n))));
            level = 0.5f * (float)log2((double)(float)(tx.x * tx.y)) + lambda;  // + 0.5 log2(w h)
        }
        alpha = alpha_sample(A, tex, tu, tv, level);
    }
    return alpha < m.x;  // evalBasicAlphaTest
}

}  // namespace rsd
