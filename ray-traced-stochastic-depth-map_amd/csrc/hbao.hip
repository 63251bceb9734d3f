// hbao.hip -- the HBAO render pass (RenderPasses/HBAO: HBAO.ps.slang:134-247, HBAOData.slang, HBAO.cpp:140-194):
// horizon-based AO with interleaved texture access, the screen-space baseline SVAO is judged against.  The
// linear depth arrives deinterleaved (rsd_deinterleave: 16 layers of ceil(w/4) x ceil(h/4)); layer s shades
// the full-resolution pixels (4 x + s % 4, 4 y + s / 4) with one Rand entry, 8 directions x 4 steps of point
// taps into its own layer, and writes (bright, dark) as RG8Unorm into the same layer of the output, which
// rsd_interleave turns back into a frame.  DualDepth reads the second layer only for the taps that lie in
// the positive hemisphere but beyond the radius (RecomputeAO, :122-132).
//
// One launch covers the 16 layers (blockIdx.z); a wave is a 64-wide run of one layer row, so the centre tap
// and every snapped tap of a step are contiguous reads of that layer.  The layer's Rand entry and its 8
// rotated directions are kernel arguments (uniform per block): the only per-pixel transcendental left is the
// final pow.  No LDS tile: the tap footprint, radius / 4 quarter texels, depends on the depth.
//
// Numerics: rsd_device.h contract (no contraction, correctly rounded / and sqrt, rsqrt(x) = 1 / sqrt(x),
// saturate(NaN) = 0, lerp(a, b, t) = a + t (b - a), HLSL round = rintf); no fast variant.  librsd's
// definitions where HLSL leaves things open are in DESIGN.md section 2 "HBAO"; the shader's quirks stay:
//   - texC = pixel centre x 1 / (width, height) while the taps step by 1 / (qw, qh): on a frame whose size
//     is no multiple of 4 the centre tap and the snapped taps read shifted texels;
//   - a layer texel whose full-resolution pixel lies outside the frame is shaded like any other;
//   - the dark channel has no distance falloff (:101).
#include "../../include/rsd.h"
#include "rsd_device.h"
#include "rsd_internal.h"

namespace rsd {
namespace {

constexpr int kDirections = 8, kSteps = 4;  // HBAO.ps.slang:4-5

struct HbaoArgs {
    const float* depth;
    const float* depth2;
    const float4* normal;
    uint8_t* out;
    int W, H, qw, qh, g;
    float resX, resY, invResX, invResY, invQX, invQY;  // HBAOData resolution, invResolution, invQuarterResolution
    float isx, isy;                                    // imageScale (:65), evaluated once on the host
    float farZ, radius, negInvRsq, bias, exponent;
    float view[9];                                     // float3x3(viewMat), row-major
    float rand[16][4];                                 // per layer (sin, cos, r1, r2)
    float dir[16][kDirections][2];                     // Rotate2D(Rand.xy, Alpha i) (:48-57, :171-174)
};

struct Shade {
    float px, py, pz, nx, ny, nz;  // ViewPosition, ViewNormal
    float negInvRsq, bias;
};

// angleTerm of ComputeAO / RecomputeAO (:112-131); the bright channel is angle * distance, the dark one angle
__device__ __forceinline__ float ao_terms(const Shade& s, float sx, float sy, float sz, float& distanceTerm) {
    const float vx = sx - s.px, vy = sy - s.py, vz = sz - s.pz;
    const float vv = vx * vx + vy * vy + vz * vz;
    const float ndotv = (s.nx * vx + s.ny * vy + s.nz * vz) * (1.0f / sqrtf(vv));
    distanceTerm = saturate(vv * s.negInvRsq + 1.0f);
    return saturate(ndotv - s.bias);
}

template <bool DUAL>
__global__ void __launch_bounds__(kImageBlockW * kImageBlockH) hbao_kernel(HbaoArgs a) {
    const int x = a.g + (int)(blockIdx.x * kImageBlockW + threadIdx.x);
    const int y = a.g + (int)(blockIdx.y * kImageBlockH + threadIdx.y);
    if (x >= a.qw - a.g || y >= a.qh - a.g) return;  // guard-band scissor on the quarter target (HBAO.cpp:181)
    const int layer = (int)blockIdx.z;
    const size_t plane = (size_t)a.qw * a.qh;
    const float* __restrict__ z1 = a.depth + (size_t)layer * plane;
    uchar2* __restrict__ out = reinterpret_cast<uchar2*>(a.out) + (size_t)layer * plane + (size_t)y * a.qw + x;

    // :137-138 svPos = floor(svPos) * 4 + quarterOffset + 0.5, texC = svPos * invResolution
    const float tcx = ((float)x * 4.0f + (float)(layer & 3) + 0.5f) * a.invResX;
    const float tcy = ((float)y * 4.0f + (float)(layer >> 2) + 0.5f) * a.invResY;
    const float depth = z1[(size_t)tex_point(tcy, a.qh) * a.qw + tex_point(tcx, a.qw)];
    const uchar2 one = make_uchar2(255, 255);
    if (depth >= a.farZ) {  // :140
        *out = one;
        return;
    }
    Shade s;
    const float ndcx = tcx * 2.0f - 1.0f, ndcy = (1.0f - tcy) * 2.0f - 1.0f;  // UVToViewSpace (:62-67)
    s.px = ndcx * depth * a.isx;
    s.py = ndcy * depth * a.isy;
    s.pz = -depth;
    const float4 nw = a.normal[(size_t)tex_point(tcy, a.H) * a.W + tex_point(tcx, a.W)];
    s.nx = a.view[0] * nw.x + a.view[1] * nw.y + a.view[2] * nw.z;  // mul(float3x3(viewMat), n) (:147)
    s.ny = a.view[3] * nw.x + a.view[4] * nw.y + a.view[5] * nw.z;
    s.nz = a.view[6] * nw.x + a.view[7] * nw.y + a.view[8] * nw.z;
    if (s.px * s.nx + s.py * s.ny + s.pz * s.nz > 0.0f) {  // :148-149
        s.nx = -s.nx;
        s.ny = -s.ny;
        s.nz = -s.nz;
    }
    s.negInvRsq = a.negInvRsq;
    s.bias = a.bias;
    // GetAORadiusInPixels (:80-93)
    const float ruvx = a.radius / (a.isx * depth) * 0.5f, ruvy = a.radius / (a.isy * depth) * 0.5f;
    const float rpx = ruvx * a.resX, rpy = ruvy * a.resY;
    const float radiusPixels = rpx + 0.5f * (rpy - rpx);
    if (radiusPixels < 1.0f) {  // :156
        *out = one;
        return;
    }
    const float stepPixels = (radiusPixels / 4.0f) / (float)(kSteps + 1);  // :162
    const float randZ = a.rand[layer][2];
    float aoX = 0.0f, aoY = 0.0f;
    for (int i = 0; i < kDirections; ++i) {
        const float dx = a.dir[layer][i][0], dy = a.dir[layer][i][1];
        float rayPixels = randZ * stepPixels + 1.0f;  // :177
#pragma unroll
        for (int k = 0; k < kSteps; ++k) {
            const float u = tcx + rintf(rayPixels * dx) * a.invQX, v = tcy + rintf(rayPixels * dy) * a.invQY;  // :183
            const size_t tap = (size_t)tex_point(v, a.qh) * a.qw + tex_point(u, a.qw);
            const float sndcx = u * 2.0f - 1.0f, sndcy = (1.0f - v) * 2.0f - 1.0f;
            const float d1 = z1[tap];
            float dist;
            const float angle = ao_terms(s, sndcx * d1 * a.isx, sndcy * d1 * a.isy, -d1, dist);
            float bright = angle * dist, dark = angle * 1.0f;
            if (DUAL) {
                if (angle > 0.0f && dist <= 0.0f) {  // RecomputeAO (:131): only these taps read the second layer
                    const float d2 = a.depth2[(size_t)layer * plane + tap];
                    float dist2;
                    const float angle2 = ao_terms(s, sndcx * d2 * a.isx, sndcy * d2 * a.isy, -d2, dist2);
                    bright = hmax(bright, angle2 * dist2);
                    dark = hmax(dark, angle2 * 1.0f);
                }
            }
            aoX += bright;
            aoY += dark;
            rayPixels += stepPixels;
        }
    }
    aoX /= (float)(kDirections * kSteps);  // :241
    aoY /= (float)(kDirections * kSteps);
    const float rx = acc_pow(saturate(1.0f - aoX * 2.0f), a.exponent);  // :243-244
    const float ry = acc_pow(saturate(1.0f - aoY * 2.0f), a.exponent);
    *out = make_uchar2(unorm8(rx), unorm8(ry));
}

// MT19937 (Matsumoto & Nishimura 1998), what std::mt19937 is
struct Mt19937 {
    uint32_t mt[624];
    int idx;
    explicit Mt19937(uint32_t seed) : idx(624) {
        mt[0] = seed;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    }
    uint32_t next() {
        if (idx >= 624) {
            for (int i = 0; i < 624; ++i) {
                const uint32_t yv = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
                mt[i] = mt[(i + 397) % 624] ^ (yv >> 1) ^ ((yv & 1u) ? 0x9908b0dfu : 0u);
            }
            idx = 0;
        }
        uint32_t yv = mt[idx++];
        yv ^= yv >> 11;
        yv ^= (yv << 7) & 0x9d2c5680u;
        yv ^= (yv << 15) & 0xefc60000u;
        yv ^= yv >> 18;
        return yv;
    }
};

}  // namespace
}  // namespace rsd

using namespace rsd;

extern "C" rsd_status rsd_hbao_noise_table(float out[16][4]) {
    if (!out) {
        set_error("rsd_hbao_noise_table: null output");
        return RSD_ERR_INVALID_ARG;
    }
    // HBAO::genNoiseTexture (HBAO.cpp:225-251) with std::uniform_real_distribution<float> written out: one
    // 32-bit draw u -> (float)u / 2^32, scaled to [min, max)
    Mt19937 gen(0u);
    auto canonical = [&]() { return (float)gen.next() / 4294967296.0f; };
    for (int i = 0; i < 16; ++i) {
        const float theta = canonical() * (2.0f * 3.141f);
        const float r1 = canonical(), r2 = canonical();
        out[i][0] = (float)sin((double)theta);
        out[i][1] = (float)cos((double)theta);
        out[i][2] = r1;
        out[i][3] = r2;
    }
    return RSD_OK;
}

extern "C" rsd_status rsd_hbao(const float* d_depth_layers, const float* d_depth2_layers, const float* d_normal_w,
                               uint32_t width, uint32_t height, const rsd_camera* cam, const rsd_hbao_params* params,
                               uint8_t* d_ambient_layers, rsd_stream stream) {
    if (!d_depth_layers || !d_normal_w || !cam || !params || !d_ambient_layers || width == 0 || height == 0) {
        set_error("rsd_hbao: invalid argument (null pointer or empty extent)");
        return RSD_ERR_INVALID_ARG;
    }
    if (!(params->radius > 0.0f)) {
        set_error("rsd_hbao: radius must be positive");
        return RSD_ERR_INVALID_ARG;
    }
    if (params->depth_mode == 2u) {  // HBAO.cpp:119, :177: the stochastic depth texture is never bound
        set_error("rsd_hbao: the StochasticDepth depth mode is not implemented (SingleDepth, DualDepth)");
        return RSD_ERR_UNSUPPORTED;
    }
    if (params->depth_mode > 2u) {
        set_error("rsd_hbao: depth_mode must be 0 (SingleDepth) or 1 (DualDepth)");
        return RSD_ERR_INVALID_ARG;
    }
    if (params->depth_mode == 1u && !d_depth2_layers) {
        set_error("rsd_hbao: invalid argument (DualDepth needs d_depth2_layers)");
        return RSD_ERR_INVALID_ARG;
    }
    HbaoArgs a{};
    a.depth = d_depth_layers;
    a.depth2 = d_depth2_layers;
    a.normal = reinterpret_cast<const float4*>(d_normal_w);
    a.out = d_ambient_layers;
    a.W = (int)width;
    a.H = (int)height;
    a.qw = (int)((width + 3) / 4);
    a.qh = (int)((height + 3) / 4);
    a.g = (int)(params->guard_band / 4u);
    if (2 * a.g >= a.qw || 2 * a.g >= a.qh) return RSD_OK;  // an empty scissor: nothing is drawn
    a.resX = (float)width;  // HBAO.cpp:162-165
    a.resY = (float)height;
    a.invResX = 1.0f / a.resX;
    a.invResY = 1.0f / a.resY;
    a.invQX = 1.0f / (float)a.qw;
    a.invQY = 1.0f / (float)a.qh;
    a.isx = 0.5f * (cam->frameWidth / cam->focalLength);
    a.isy = 0.5f * (cam->frameHeight / cam->focalLength);
    a.farZ = cam->farZ;
    a.radius = params->radius;
    a.negInvRsq = -1.0f / (params->radius * params->radius);  // HBAO::setRadius (:212-217)
    a.bias = params->ndotv_bias;
    a.exponent = params->power_exponent;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) a.view[r * 3 + c] = cam->viewMat[r * 4 + c];
    const float alpha = 2.0f * 3.141f / (float)kDirections;  // :164
    for (int s = 0; s < 16; ++s) {
        for (int c = 0; c < 4; ++c) a.rand[s][c] = params->rand[s][c];
        for (int i = 0; i < kDirections; ++i) {
            const float angle = alpha * (float)i;
            const float ct = (float)cos((double)angle), st = (float)sin((double)angle);
            a.dir[s][i][0] = params->rand[s][0] * ct - params->rand[s][1] * st;
            a.dir[s][i][1] = params->rand[s][0] * st + params->rand[s][1] * ct;
        }
    }
    const dim3 grid = image_grid(a.qw - 2 * a.g, a.qh - 2 * a.g, 16);
    if (params->depth_mode == 1u)
        hipLaunchKernelGGL(hbao_kernel<true>, grid, image_block(), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(hbao_kernel<false>, grid, image_block(), 0, (hipStream_t)stream, a);
    return launch_status("hbao_kernel launch");
}
