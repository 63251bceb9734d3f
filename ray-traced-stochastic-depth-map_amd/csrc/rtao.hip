// rtao.hip -- the RTAO pass: ray-traced ambient occlusion, the ground truth that screen-space AO is
// judged against (include/rsd.h rsd_rtao).
//
// Reference: RenderPasses/RTAO/Ray.rt.slang:56-212 (rayGen, AOOnce, AOMoreThanOnce, CalculateAO, the
// Jenkins hash), RTAO.cpp:134-141 (maxAORayTHit), :190-234 (the RGBA8Snorm sample table),
// RTAOData.slang; Utils/Sampling/UniformSampleGenerator.slang:53-71, Pseudorandom/SplitMix64.slang:56-82,
// Pseudorandom/Xoshiro.slang:46-68, SampleGeneratorInterface.slang:50-65, Utils/Math/BitTricks.slang:47-62,
// MathHelpers.slang:360-370 (sample_cosine_hemisphere_polar).
//
// One lane per pixel, 8x8 pixels per wave, as in depth_peel.hip; the spp rays of a pixel run one after the
// other inside its lane.  Each ray is one walk_lane (bvh_traverse.h) with the upper bound
// min(TMax, best t): the closest hit in [TMin, TMax] by the (t, prim) key, no face culling (the reference's
// TraceRay sets no cull flag), alpha-masked triangles alpha-tested at LOD 0 (its any-hit shader).
// Everything but exp, sin and cos rounds operation by operation as written (rsd_device.h), so a CPU
// restatement reproduces the rays, the hit parameters and ray_distance bit for bit.
#include <cmath>
#include <random>

#include "bvh_traverse.h"
#include "rsd_device.h"
#include "rsd_internal.h"

namespace rsd {

struct RtaoArgs {
    const float4* nodes;  // BVH base, or null: a scene without triangles (every ray misses)
    uint32_t triOff;
    int W, H;
    const float4* posW;   // RGBA32F: world position, w == 0 marks a miss of the G-buffer
    const float4* faceN;  // RGBA32F: world face normal (xyz)
    uint32_t frame;
    float maxAORayTHit, maxTheoreticalTHit;  // RTAOData
    uint32_t spp, falloff;
    float lambda, minAmbient, normalScale;
    const uint32_t* table;  // RSD_RTAO_SAMPLE_COUNT RGBA8Snorm samples
    float* ambient;
    float* rayDistance;
    float4* rayLog;  // or null
    uint32_t alphaTest;
    AlphaData alpha;
};

// Ray.rt.slang:61-77
__host__ __device__ inline uint32_t jenkins(uint32_t a) {
    a -= (a << 6);
    a ^= (a >> 17);
    a -= (a << 9);
    a ^= (a << 4);
    a -= (a << 3);
    a ^= (a << 10);
    a ^= (a >> 15);
    return a;
}
__device__ __forceinline__ uint32_t rtao_hash(uint32_t x, uint32_t y, uint32_t frame) {
    return jenkins(x * 449u + y * 2857u + jenkins(frame));
}

// RGBA8Snorm fetch: max(c / 127, -1)
__device__ __forceinline__ float snorm8(uint32_t packed, int k) {
    return fmaxf((float)(int)(int8_t)(uint8_t)(packed >> (8 * k)) / 127.0f, -1.0f);
}

// BitTricks.slang:47-62
__device__ __forceinline__ uint32_t spread16(uint32_t v) {
    v &= 0x0000ffffu;
    v = (v | (v << 8)) & 0x00ff00ffu;
    v = (v | (v << 4)) & 0x0f0f0f0fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}
__device__ __forceinline__ uint64_t splitmix64(uint64_t& state) {
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }

// UniformSampleGenerator: xoshiro128** seeded by SplitMix64(interleave(pixel), sampleNumber)
struct UniformGen {
    uint32_t s0, s1, s2, s3;
    __device__ __forceinline__ UniformGen(uint32_t x, uint32_t y, uint32_t sampleNumber) {
        uint64_t st = ((uint64_t)sampleNumber << 32) | (uint64_t)(spread16(x) | (spread16(y) << 1));
        const uint64_t a = splitmix64(st), b = splitmix64(st);
        s0 = (uint32_t)a;
        s1 = (uint32_t)(a >> 32);
        s2 = (uint32_t)b;
        s3 = (uint32_t)(b >> 32);
    }
    __device__ __forceinline__ uint32_t next() {
        const uint32_t r = rotl32(s0 * 5u, 7) * 9u;
        const uint32_t t = s1 << 9;
        s2 ^= s0;
        s3 ^= s1;
        s1 ^= s2;
        s0 ^= s3;
        s2 ^= t;
        s3 = rotl32(s3, 11);
        return r;
    }
    // sampleNext1D: the upper 24 bits over 2^24
    __device__ __forceinline__ float next1D() { return (float)(next() >> 8) * 0x1p-24f; }
};

// Ray.rt.slang:79-96; t = 0: the ray missed
__device__ __forceinline__ float calculate_ao(const RtaoArgs& a, float tHit) {
    float ambient = 1.0f;
    if (tHit > 0.0f) {
        float occ = 1.0f;
        if (a.falloff) {
            const float t = tHit / a.maxTheoreticalTHit;
            occ = expf(-a.lambda * t * t);
        }
        ambient = 1.0f - (1.0f - a.minAmbient) * occ;
    }
    return ambient;
}

__global__ void __launch_bounds__(kBlock) rtao_kernel(RtaoArgs a) {
    __shared__ uint32_t sstack[kLdsStack * kBlock];
    __shared__ float sstackT[kLdsStack * kBlock];
    const int lane = threadIdx.x;
    const int x = blockIdx.x * kTile + (lane & (kTile - 1));
    const int y = blockIdx.y * kTile + (lane / kTile);
    if (x >= a.W || y >= a.H) return;
    const size_t o = (size_t)y * a.W + x;
    const float4 wp = a.posW[o];
    if (wp.w == 0.0f) {  // Ray.rt.slang:188-193: the G-buffer missed
        a.rayDistance[o] = a.maxAORayTHit;
        a.ambient[o] = 1.0f;
        if (a.rayLog)
            for (uint32_t i = 0; i < a.spp; ++i) a.rayLog[o * a.spp + i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 fn = a.faceN[o];
    const f3 n = normalize(mk(fn.x, fn.y, fn.z));
    const f3 bitangent = fabsf(n.x) > fabsf(n.y) ? mk(-n.z, 0.0f, n.x) : mk(0.0f, n.z, -n.y);  // getTangentVector
    const f3 tangent = cross(bitangent, n);
    const f3 origin = mk(wp.x, wp.y, wp.z) + n * a.normalScale;
    const float tmin = 0.001f, tmax = a.maxAORayTHit;
    const bool alphaOn = a.alphaTest != 0u;
    UniformGen sg((uint32_t)x, (uint32_t)y, a.frame);  // AOMoreThanOnce's generator (unused with spp = 1)
    float ambientSum = 0.0f;
    // AOMoreThanOnce starts tHit at maxAORayTHit, not at 0, before it adds the spp rays' distances and
    // divides by spp (Ray.rt.slang:154, 172, 176): the reference's sum is kept as it is.  AOOnce has one
    // ray and no sum: 0 + its value is exact.
    float tSum = a.spp > 1u ? a.maxAORayTHit : 0.0f;
    for (uint32_t i = 0; i < a.spp; ++i) {
        f3 s;
        if (a.spp > 1u) {  // sample_cosine_hemisphere_polar(sampleNext2D(sg))
            const float ux = sg.next1D();
            const float uy = sg.next1D();
            const float rr = sqrtf(ux);
            const float phi = 6.28318530717958647693f * uy;
            s = mk(rr * cosf(phi), rr * sinf(phi), sqrtf(1.0f - ux));
        } else {  // AOOnce: gSamples[hash(pixel, frameIndex) % numSamples]
            const uint32_t packed = a.table[rtao_hash((uint32_t)x, (uint32_t)y, a.frame) % RSD_RTAO_SAMPLE_COUNT];
            s = mk(snorm8(packed, 0), snorm8(packed, 1), snorm8(packed, 2));
        }
        const f3 dir = normalize(tangent * s.x + bitangent * s.y + n * s.z);
        float bestT = INFINITY;
        uint32_t bestP = 0xffffffffu;
        int found = 0;
        if (a.nodes) {
            RayCtx r;
            ray_setup(r, origin, dir);
            auto far = [&]() RSD_INLINE_LAMBDA { return fminf(tmax, bestT); };
            auto hit = [&](uint32_t, float t, float bu, float bv, float, float4 v0, float4 v1,
                           float4 v2) RSD_INLINE_LAMBDA {
                if (!(t >= tmin && t <= tmax)) return;
                const uint32_t prim = __float_as_uint(v0.w);
                const uint32_t flags = __float_as_uint(v1.w);
                if (!key_less(t, prim, bestT, bestP)) return;
                if (alphaOn && (flags & 4u) && alpha_test_fails(a.alpha, prim, v0, v1, v2, bu, bv, false, t, r.d))
                    return;
                bestT = t;
                bestP = prim;
                found = 1;
            };
            walk_lane<false>(a.nodes, a.triOff, r, tmin, &sstack[lane], &sstackT[lane], far, hit);
        }
        const float t = found ? bestT : 0.0f;  // the payload: 0 = miss
        if (a.rayLog) a.rayLog[o * a.spp + i] = make_float4(dir.x, dir.y, dir.z, t);
        ambientSum += calculate_ao(a, t);
        tSum += t > 0.0f ? t : a.maxAORayTHit;
    }
    if (a.spp > 1u) {
        a.ambient[o] = ambientSum / (float)a.spp;
        a.rayDistance[o] = tSum / (float)a.spp;
    } else {  // AOOnce: the one ray's values
        a.ambient[o] = ambientSum;
        a.rayDistance[o] = tSum;
    }
}

__global__ void rtao_pack_kernel(const float* __restrict__ ambient, const float* __restrict__ rayDistance, uint32_t n,
                                 uint8_t* __restrict__ ambient8, uint16_t* __restrict__ rayDistance16) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (ambient8) ambient8[i] = unorm8(ambient[i]);
    if (rayDistance16) {
        const _Float16 h = (_Float16)rayDistance[i];  // round to nearest even
        rayDistance16[i] = __builtin_bit_cast(uint16_t, h);
    }
}

namespace {

struct Derived {
    float maxAORayTHit, maxTheoreticalTHit;
};

// the parameter checks of rsd_rtao and RTAO.cpp:134-141
rsd_status derive(const char* who, const rsd_rtao_params* p, Derived& d) {
    const std::string w(who);
    if (!p) {
        set_error(w + ": null params");
        return RSD_ERR_INVALID_ARG;
    }
    if (p->spp == 0) {
        set_error(w + ": spp must be at least 1");
        return RSD_ERR_INVALID_ARG;
    }
    if (!std::isfinite(p->max_t_hit) || !(p->max_t_hit > 0.0f)) {
        set_error(w + ": max_t_hit must be finite and positive");
        return RSD_ERR_INVALID_ARG;
    }
    d.maxTheoreticalTHit = p->max_t_hit;
    d.maxAORayTHit = p->max_t_hit;
    if (p->apply_exponential_falloff) {
        if (!(p->min_occlusion_cutoff > 0.0f && p->min_occlusion_cutoff < 1.0f)) {
            set_error(w + ": min_occlusion_cutoff must lie in (0, 1) with the exponential falloff");
            return RSD_ERR_INVALID_ARG;
        }
        const float lambda = p->exponential_falloff_decay_constant;
        const float t = std::sqrt(logf(p->min_occlusion_cutoff) / -lambda);
        d.maxAORayTHit = t * p->max_t_hit;
        if (!std::isfinite(d.maxAORayTHit) || !(d.maxAORayTHit > 0.0f)) {
            set_error(w + ": exponential_falloff_decay_constant gives no finite positive ray length");
            return RSD_ERR_INVALID_ARG;
        }
    }
    return RSD_OK;
}

}  // namespace

}  // namespace rsd

using namespace rsd;

extern "C" rsd_status rsd_rtao_sample_table(uint32_t out[RSD_RTAO_SAMPLE_COUNT]) {
    if (!out) {
        set_error("rsd_rtao_sample_table: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    std::mt19937 rng(89);
    // uniform_real_distribution<float>(0, 1) of the reference's standard library, written out: one raw draw
    // scaled by 2^-32, and a quotient that rounds up to 1 replaced by the float below 1
    auto draw = [&]() {
        const float u = (float)(uint32_t)rng() * 0x1p-32f;
        return u >= 1.0f ? std::nextafterf(1.0f, 0.0f) : u;
    };
    auto snorm = [](float v) {  // packSnorm4x8: round(clamp(v, -1, 1) * 127)
        const float c = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
        return (uint32_t)(uint8_t)(int8_t)(int)std::round(c * 127.0f);
    };
    for (uint32_t i = 0; i < RSD_RTAO_SAMPLE_COUNT; ++i) {
        const float ux = draw();
        const float uy = draw();
        const float phi = uy * 2.0f * (float)M_PI;
        const float t = std::sqrt(1.0f - ux);
        const float s = std::sqrt(1.0f - t * t);
        out[i] = snorm(s * std::cos(phi)) | (snorm(s * std::sin(phi)) << 8) | (snorm(t) << 16) | (snorm(0.0f) << 24);
    }
    return RSD_OK;
}

extern "C" rsd_status rsd_rtao_ray_t_max(const rsd_rtao_params* params, float* out) {
    Derived d;
    if (!out) {
        set_error("rsd_rtao_ray_t_max: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    const rsd_status st = derive("rsd_rtao_ray_t_max", params, d);
    if (st == RSD_OK) *out = d.maxAORayTHit;
    return st;
}

extern "C" rsd_status rsd_rtao(rsd_scene* scene, const rsd_rtao_params* params, uint32_t width, uint32_t height,
                               const float* d_pos_w, const float* d_face_normal_w, uint32_t frame_index,
                               float* d_ambient, float* d_ray_distance, float* d_ray_log, rsd_stream stream) {
    if (!scene || !params || !d_pos_w || !d_face_normal_w || !d_ambient || !d_ray_distance || width == 0 ||
        height == 0) {
        set_error("rsd_rtao: null argument or empty extent");
        return RSD_ERR_INVALID_ARG;
    }
    Derived d;
    if (rsd_status st = derive("rsd_rtao", params, d); st != RSD_OK) return st;
    if ((uint64_t)width * height > 0x7fffffffull) {
        set_error("rsd_rtao: extent too large");
        return RSD_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    {  // the sample table of this scene's device, uploaded by the first call
        std::lock_guard<std::mutex> lock(scene->ws_mutex);
        if (!scene->d_rtao_table) {
            std::vector<uint32_t> table(RSD_RTAO_SAMPLE_COUNT);
            rsd_rtao_sample_table(table.data());
            uint32_t* dt = nullptr;
            RSD_HIP(hipMalloc(&dt, table.size() * 4));
            hipError_t e = hipMemcpy(dt, table.data(), table.size() * 4, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(dt);
                return hip_fail(e, "rsd_rtao: sample table upload");
            }
            scene->d_rtao_table = dt;
        }
    }
    RtaoArgs a{scene->triangle_count ? scene->d_nodes : nullptr,
               scene->tri_offset,
               (int)width,
               (int)height,
               reinterpret_cast<const float4*>(d_pos_w),
               reinterpret_cast<const float4*>(d_face_normal_w),
               frame_index,
               d.maxAORayTHit,
               d.maxTheoreticalTHit,
               params->spp,
               params->apply_exponential_falloff ? 1u : 0u,
               params->exponential_falloff_decay_constant,
               params->minimum_ambient_illumination,
               params->normal_scale,
               scene->d_rtao_table,
               d_ambient,
               d_ray_distance,
               reinterpret_cast<float4*>(d_ray_log),
               scene->d_alpha ? 1u : 0u,
               scene->alpha};
    dim3 grid((width + kTile - 1) / kTile, (height + kTile - 1) / kTile);
    hipLaunchKernelGGL(rtao_kernel, grid, dim3(kBlock), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? RSD_OK : hip_fail(e, "rtao_kernel launch");
}

extern "C" rsd_status rsd_rtao_pack(const float* d_ambient, const float* d_ray_distance, uint32_t count,
                                    uint8_t* d_ambient_unorm8, uint16_t* d_ray_distance_f16, rsd_stream stream) {
    if ((d_ambient == nullptr) != (d_ambient_unorm8 == nullptr) ||
        (d_ray_distance == nullptr) != (d_ray_distance_f16 == nullptr) || (!d_ambient && !d_ray_distance) ||
        count == 0) {
        set_error("rsd_rtao_pack: each input needs its output, at least one pair, and a count");
        return RSD_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(rtao_pack_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_ambient,
                       d_ray_distance, count, d_ambient_unorm8, d_ray_distance_f16);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? RSD_OK : hip_fail(e, "rtao_pack_kernel launch");
}
