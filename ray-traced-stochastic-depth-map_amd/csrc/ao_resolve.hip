// ao_resolve.hip -- the two passes of the reference that turn the dual AO map (bright, dark) of SVAO's dualAO
// and of HBAO into one AO value:
//
// AOGuidedBlur (RenderPasses/AOGuidedBlur: AOGuidedBlur.ps.slang:105-208, AOGuidedBlur.cpp:121-173): a separable
// depth-guided Gauss blur of (bright, dark) and of their squares, x into an RGBA8Unorm ping-pong image
// (means.xy, meansSq.xy -- the 8-bit quantisation between the passes is part of the result), then y, whose
// tail weighs the unblurred bright and dark by the other channel's deviation from its mean (:174-204).
//
// AOVarianceFix (RenderPasses/AOVarianceFix: AOVarianceFix.ps.slang:37-99, AOVarianceFix.cpp:115-159): the same
// idea in one pass over the centre and its four cross neighbours, on separate R8Unorm bright and dark images,
// through a linear sampler.
//
// Both run per array slice of a deinterleaved image (AOGuidedBlur.cpp:155, AOVarianceFix.cpp:149): L layers of
// qw x qh, 16 after DeinterleaveTexture or HBAO, 1 for a plain image.  One launch per direction covers every
// layer (blockIdx.z); a wave is a 64-wide run of one layer row, so the centre and every tap of the x pass are
// contiguous reads of that layer.  The scissor is guardBand / int(sqrt(L) + 0.5) on the layer
// (AOGuidedBlur.cpp:145-150) while uvMin / uvMax are the GuardBand pass's, of the full-size frame
// (GuardBand.cpp:62-63, AOGuidedBlur.cpp:152-153): texels outside the scissor are written in neither pass.
// The 2 R + 1 spatial weights do not depend on the pixel: the host evaluates them once (kernel arguments).
//
// Numerics: rsd_device.h contract (no contraction, correctly rounded / and sqrt, fminf / fmaxf for HLSL min /
// max); exp evaluated in double and rounded once, as blur_kernel does for exp2.  The shaders' quirks stay:
//   - the tap position is accumulated, uv += uvStep (:118, :144), not recomputed per tap;
//   - the centre depth is max(z, 1.401298e-45) (:110): a depth of 0 gives every tap the weight exp(-500) = 0
//     and the pixel the fallback colour (:149-153);
//   - the y pass's fallback squares the ping-pong means, it does not read .zw (:152);
//   - DEV_EXPONENT 1 and ENHANCE_CONTRAST 1 (:34-35): pow(x, 1.0) is x, pow(x, 0.5) is sqrtf(x);
//   - a source without a second channel reads dark = 0 (Texture2D<float2> of an R8Unorm image);
//   - AOVarianceFix clamps with saturate (:58, NaN -> 0) where AOGuidedBlur uses min(., 1) (:133, NaN -> 1).
// The eight debug OUTPUT_* modes are not built; CLAMP_RESULTS is commented out in the shader (:155, :201-202).
#include <cmath>

#include "../../include/rsd_graph.h"
#include "rsd_device.h"
#include "rsd_internal.h"

namespace rsd {
namespace {

constexpr int kMaxRadius = 20;  // AOGuidedBlur.cpp:180

struct GuidedArgs {
    const uint8_t* src;   // the pass's gSrcTex: the source (x pass) or the ping-pong image (y pass)
    const uint8_t* orig;  // gBrightDarkTex, read by the y pass's tail
    const float* z;
    uint8_t* dst;
    int qw, qh, g, R;
    int srcTexel;  // bytes per source texel: 1 (R8Unorm) or 2 (RG8Unorm)
    uint32_t localDeviation;
    GuardUv uv;
    float spatial[2 * kMaxRadius + 1];  // kernel(R - it, SPATIAL_VARIANCE) (:123)
};

// kernel(offset, variance) (:60-63) for the depth weight: DEPTH_VARIANCE 0.001
__device__ __forceinline__ float depth_kernel(float offset) {
    return (float)exp((double)(-0.5f * offset * offset / 0.001f));
}

// One texel of gSrcTex as four bytes: the RGBA8Unorm ping-pong image, or the source, whose missing channels
// read 0 (the dark channel of an R8Unorm source)
template <bool RGBA>
__device__ __forceinline__ uchar4 load_texel4(const uint8_t* __restrict__ t, size_t i, int srcTexel) {
    if (RGBA) return reinterpret_cast<const uchar4*>(t)[i];
    if (srcTexel == 2) {
        const uchar2 v = reinterpret_cast<const uchar2*>(t)[i];
        return make_uchar4(v.x, v.y, 0, 0);
    }
    return make_uchar4(t[i], 0, 0, 0);
}

template <bool YPASS>
__global__ void __launch_bounds__(kImageBlockW * kImageBlockH) ao_guided_blur_kernel(GuidedArgs a) {
    const int x = a.g + (int)(blockIdx.x * kImageBlockW + threadIdx.x);
    const int y = a.g + (int)(blockIdx.y * kImageBlockH + threadIdx.y);
    if (x >= a.qw - a.g || y >= a.qh - a.g) return;  // guard-band scissor on the layer (AOGuidedBlur.cpp:150)
    const size_t plane = (size_t)a.qw * a.qh, base = (size_t)blockIdx.z * plane;
    const float* __restrict__ z = a.z + base;
    const uint8_t* __restrict__ src = a.src + base * (YPASS ? 4 : a.srcTexel);
    const float tcx = ((float)x + 0.5f) / (float)a.qw, tcy = ((float)y + 0.5f) / (float)a.qh;
    const float ccx = fminf(fmaxf(tcx, a.uv.minX), a.uv.maxX), ccy = fminf(fmaxf(tcy, a.uv.minY), a.uv.maxY);
    const size_t centre = (size_t)tex_point(ccy, a.qh) * a.qw + tex_point(ccx, a.qw);
    const float localDepth = fmaxf(z[centre], __uint_as_float(1u));  // :110
    const uchar4 local = load_texel4<YPASS>(src, centre, a.srcTexel);  // :111
    const float localX = unorm8_to_float(local.x), localY = unorm8_to_float(local.y);
    const float stepX = (1.0f / (float)a.qw) * (YPASS ? 0.0f : 1.0f);  // :114-116
    const float stepY = (1.0f / (float)a.qh) * (YPASS ? 1.0f : 0.0f);
    float u = tcx - stepX * (float)a.R, v = tcy - stepY * (float)a.R;  // :118
    float meanX = 0.0f, meanY = 0.0f, sqX = 0.0f, sqY = 0.0f, weightSum = 0.0f;
    for (int it = 0; it <= 2 * a.R; ++it) {
        const float cu = fminf(fmaxf(u, a.uv.minX), a.uv.maxX), cv = fminf(fmaxf(v, a.uv.minY), a.uv.maxY);
        const size_t tap = (size_t)tex_point(cv, a.qh) * a.qw + tex_point(cu, a.qw);
        const uchar4 t = load_texel4<YPASS>(src, tap, a.srcTexel);
        const float aoX = unorm8_to_float(t.x), aoY = unorm8_to_float(t.y);
        // :125-127 the y pass finds the squares in the last two channels
        const float aoSqX = YPASS ? unorm8_to_float(t.z) : aoX * aoX;
        const float aoSqY = YPASS ? unorm8_to_float(t.w) : aoY * aoY;
        const float relativeDepth = fminf(fabsf(z[tap] / localDepth - 1.0f), 1.0f);  // :133
        const float w = a.spatial[it] * depth_kernel(relativeDepth) * 1.0f;          // :139
        weightSum += w;
        meanX += w * aoX;
        meanY += w * aoY;
        sqX += w * aoSqX;
        sqY += w * aoSqY;
        u += stepX;  // :144
        v += stepY;
    }
    const float norm = fmaxf(weightSum, 1e-4f);  // :147-148
    meanX /= norm;
    meanY /= norm;
    sqX /= norm;
    sqY /= norm;
    if (weightSum < 1e-4f) {  // :149-153
        meanX = localX;
        meanY = localY;
        sqX = localX * localX;
        sqY = localY * localY;
    }
    const size_t o = base + (size_t)y * a.qw + x;
    if (!YPASS) {  // :207 into the RGBA8Unorm ping-pong image
        reinterpret_cast<uchar4*>(a.dst)[o] = make_uchar4(unorm8(meanX), unorm8(meanY), unorm8(sqX), unorm8(sqY));
        return;
    }
    // OUTPUT_RESULT (:167-204)
    const uchar4 orig = load_texel4<false>(a.orig + base * a.srcTexel, centre, a.srcTexel);  // :168
    const float origX = unorm8_to_float(orig.x), origY = unorm8_to_float(orig.y);
    float devX, devY;
    if (a.localDeviation) {  // :175-180
        devX = fabsf(origX - meanX);
        devY = fabsf(origY - meanY);
    } else {  // :188-193
        devX = sqrtf(fabsf(sqX - meanX * meanX));
        devY = sqrtf(fabsf(sqY - meanY * meanY));
    }
    devY = fmaxf(devY, 0.01f);  // DARK_EPSILON
    devX *= 1.0f;               // ENHANCE_CONTRAST
    const float sum = devX + devY;
    const float c = origX * (devY / sum) + origY * (devX / sum);  // dot(cOriginal, dev.yx / (dev.x + dev.y))
    a.dst[o] = unorm8(c);
}

// ---------------------------------------------------------------------- AOVarianceFix
struct VarianceArgs {
    const uint8_t* bright;
    const uint8_t* dark;
    const float* z;
    uint8_t* dst;
    int qw, qh, g;
    GuardUv uv;
    float spatial;  // kernel(1, 10) * kernel(0, 10) (:56), the same for the four neighbours
};

// The linear / clamp sampler (AOVarianceFix.cpp:57): tex_sample.h's rule, all four taps.  A tap's footprint is
// split and addressed once for its three images: depth here, bright and dark through unorm8_bilinear_at
__device__ __forceinline__ float float_bilinear_at(const float* __restrict__ t, const TexSplit& s, const TexTaps& p) {
    return tex_lerp(s, t[p.t00], t[p.t10], t[p.t01], t[p.t11]);
}

__global__ void __launch_bounds__(kImageBlockW * kImageBlockH) ao_variance_fix_kernel(VarianceArgs a) {
    const int x = a.g + (int)(blockIdx.x * kImageBlockW + threadIdx.x);
    const int y = a.g + (int)(blockIdx.y * kImageBlockH + threadIdx.y);
    if (x >= a.qw - a.g || y >= a.qh - a.g) return;  // guard-band scissor on the layer (AOVarianceFix.cpp:144)
    const size_t base = (size_t)blockIdx.z * ((size_t)a.qw * a.qh);
    const float* __restrict__ z = a.z + base;
    const uint8_t* __restrict__ bright = a.bright + base;
    const uint8_t* __restrict__ dark = a.dark + base;
    const float tcx = ((float)x + 0.5f) / (float)a.qw, tcy = ((float)y + 0.5f) / (float)a.qh;
    const float stepX = 1.0f / (float)a.qw, stepY = 1.0f / (float)a.qh;  // :45-47
    const TexSplit sc = tex_split(a.qw, a.qh, fminf(fmaxf(tcx, a.uv.minX), a.uv.maxX),
                                  fminf(fmaxf(tcy, a.uv.minY), a.uv.maxY));
    const TexTaps pc = tex_taps(sc, a.qw, a.qh, false);
    const float localDepth = fmaxf(float_bilinear_at(z, sc, pc), __uint_as_float(1u));  // :39
    const float localX = unorm8_bilinear_at(bright, sc, pc), localY = unorm8_bilinear_at(dark, sc, pc);
    float meanX = localX, meanY = localY, weightSum = 1.0f;
    constexpr float ox[4] = {-1.0f, 0.0f, 1.0f, 0.0f}, oy[4] = {0.0f, -1.0f, 0.0f, 1.0f};  // :50
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const float u = tcx + ox[it] * stepX, v = tcy + oy[it] * stepY;  // :53
        const TexSplit s = tex_split(a.qw, a.qh, fminf(fmaxf(u, a.uv.minX), a.uv.maxX),
                                     fminf(fmaxf(v, a.uv.minY), a.uv.maxY));
        const TexTaps p = tex_taps(s, a.qw, a.qh, false);
        const float relativeDepth = saturate(fabsf(float_bilinear_at(z, s, p) / localDepth - 1.0f));  // :58
        const float w = a.spatial * 1.0f * depth_kernel(relativeDepth);                               // :62
        weightSum += w;
        meanX += w * unorm8_bilinear_at(bright, s, p);
        meanY += w * unorm8_bilinear_at(dark, s, p);
    }
    const float norm = fmaxf(weightSum, 1e-4f);  // :85
    meanX /= norm;
    meanY /= norm;
    if (meanX < 1e-4f || meanY < 1e-4f) {  // :86-87
        meanX = localX;
        meanY = localY;
    }
    const float devX = fabsf(localX - meanX);                // :89-91
    const float devY = fmaxf(fabsf(localY - meanY), 0.01f);  // :92
    const float sum = devX + devY;
    a.dst[base + (size_t)y * a.qw + x] = unorm8(localX * (devY / sum) + localY * (devX / sum));  // :94-96
}

// The pass with enabled = False (AOGuidedBlur.cpp:130-138): a blit of every slice into the R8Unorm output, which
// keeps the first channel
__global__ void __launch_bounds__(256) ao_first_channel_kernel(const uint8_t* __restrict__ src, uint32_t srcTexel,
                                                               uint64_t n, uint8_t* __restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) dst[i] = src[i * srcTexel];
}

// kernel(offset, variance) (:60-63) of a constant offset, on the host
float host_kernel(float offset, float variance) { return (float)std::exp((double)(-0.5f * offset * offset / variance)); }

// The layer extent, the scissor on it and the GuardBand pass's uv bounds of the full-size frame
struct LayerRect {
    int qw, qh, g;
    GuardUv uv;
    bool empty;
};
LayerRect layer_rect(uint32_t width, uint32_t height, uint32_t layers, uint32_t guard_band) {
    LayerRect r{};
    r.qw = (int)(layers == 16 ? (width + 3) / 4 : width);
    r.qh = (int)(layers == 16 ? (height + 3) / 4 : height);
    // AOGuidedBlur.cpp:145-148
    r.g = (int)(layers > 1 ? guard_band / (uint32_t)(int)(std::sqrt((double)layers) + 0.5) : guard_band);
    r.empty = 2 * (int64_t)r.g >= r.qw || 2 * (int64_t)r.g >= r.qh;
    r.uv = guard_uv(width, height, guard_band);
    return r;
}
dim3 resolve_grid(const LayerRect& r, uint32_t layers) { return image_grid(r.qw - 2 * r.g, r.qh - 2 * r.g, layers); }

}  // namespace
}  // namespace rsd

using namespace rsd;

extern "C" rsd_status rsd_ao_guided_blur(const rsd_ao_guided_blur_params* params, const uint8_t* d_src,
                                         const float* d_depth_layers, uint8_t* d_pingpong, uint8_t* d_dst,
                                         rsd_stream stream) {
    if (!params || !d_src || !d_depth_layers || !d_pingpong || !d_dst) {
        set_error("rsd_ao_guided_blur: invalid argument (null pointer)");
        return RSD_ERR_INVALID_ARG;
    }
    if (params->width == 0 || params->height == 0) {
        set_error("rsd_ao_guided_blur: invalid argument (empty extent)");
        return RSD_ERR_INVALID_ARG;
    }
    if (params->kernel_radius < 1 || params->kernel_radius > (uint32_t)kMaxRadius) {
        set_error("rsd_ao_guided_blur: kernel_radius must be 1..20");
        return RSD_ERR_INVALID_ARG;
    }
    if (params->src_texel_bytes != 1 && params->src_texel_bytes != 2) {
        set_error("rsd_ao_guided_blur: src_texel_bytes must be 1 (R8Unorm) or 2 (RG8Unorm)");
        return RSD_ERR_INVALID_ARG;
    }
    if (params->layers != 1 && params->layers != 16) {
        set_error("rsd_ao_guided_blur: layers must be 1 (a plain image) or 16 (a deinterleaved one)");
        return RSD_ERR_UNSUPPORTED;
    }
    const LayerRect r = layer_rect(params->width, params->height, params->layers, params->guard_band);
    if (r.empty) return RSD_OK;  // an empty scissor: nothing is drawn
    GuidedArgs a{};
    a.z = d_depth_layers;
    a.orig = d_src;
    a.qw = r.qw;
    a.qh = r.qh;
    a.g = r.g;
    a.R = (int)params->kernel_radius;
    a.srcTexel = (int)params->src_texel_bytes;
    a.localDeviation = params->local_deviation ? 1u : 0u;
    a.uv = r.uv;
    for (int it = 0; it <= 2 * a.R; ++it) a.spatial[it] = host_kernel((float)(a.R - it), 16.4f);  // SPATIAL_VARIANCE
    const dim3 grid = resolve_grid(r, params->layers);
    hipStream_t s = (hipStream_t)stream;
    a.src = d_src;  // blur in x (AOGuidedBlur.cpp:161-165)
    a.dst = d_pingpong;
    hipLaunchKernelGGL(ao_guided_blur_kernel<false>, grid, image_block(), 0, s, a);
    const rsd_status st = launch_status("ao_guided_blur_kernel (x) launch");
    if (st != RSD_OK) return st;
    a.src = d_pingpong;  // blur in y (:167-171)
    a.dst = d_dst;
    hipLaunchKernelGGL(ao_guided_blur_kernel<true>, grid, image_block(), 0, s, a);
    return launch_status("ao_guided_blur_kernel (y) launch");
}

extern "C" rsd_status rsd_ao_first_channel(const uint8_t* d_src, uint32_t src_texel_bytes, uint64_t texels,
                                           uint8_t* d_dst, rsd_stream stream) {
    if (!d_src || !d_dst || texels == 0 || texels > 0x7fffffffull * 256u) {
        set_error("rsd_ao_first_channel: invalid argument (null pointer or texel count)");
        return RSD_ERR_INVALID_ARG;
    }
    if (src_texel_bytes != 1 && src_texel_bytes != 2) {
        set_error("rsd_ao_first_channel: src_texel_bytes must be 1 (R8Unorm) or 2 (RG8Unorm)");
        return RSD_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(ao_first_channel_kernel, dim3((uint32_t)((texels + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, d_src, src_texel_bytes, texels, d_dst);
    return launch_status("ao_first_channel_kernel launch");
}

extern "C" rsd_status rsd_ao_variance_fix(const rsd_ao_variance_fix_params* params, const uint8_t* d_bright,
                                          const uint8_t* d_dark, const float* d_depth_layers, uint8_t* d_dst,
                                          rsd_stream stream) {
    if (!params || !d_bright || !d_dark || !d_depth_layers || !d_dst) {
        set_error("rsd_ao_variance_fix: invalid argument (null pointer)");
        return RSD_ERR_INVALID_ARG;
    }
    if (params->width == 0 || params->height == 0) {
        set_error("rsd_ao_variance_fix: invalid argument (empty extent)");
        return RSD_ERR_INVALID_ARG;
    }
    if (params->layers != 1 && params->layers != 16) {
        set_error("rsd_ao_variance_fix: layers must be 1 (a plain image) or 16 (a deinterleaved one)");
        return RSD_ERR_UNSUPPORTED;
    }
    const LayerRect r = layer_rect(params->width, params->height, params->layers, params->guard_band);
    if (r.empty) return RSD_OK;  // an empty scissor: nothing is drawn
    VarianceArgs a{};
    a.bright = d_bright;
    a.dark = d_dark;
    a.z = d_depth_layers;
    a.dst = d_dst;
    a.qw = r.qw;
    a.qh = r.qh;
    a.g = r.g;
    a.uv = r.uv;
    a.spatial = host_kernel(1.0f, 10.0f) * host_kernel(0.0f, 10.0f);
    hipLaunchKernelGGL(ao_variance_fix_kernel, resolve_grid(r, params->layers), image_block(), 0, (hipStream_t)stream, a);
    return launch_status("ao_variance_fix_kernel launch");
}
