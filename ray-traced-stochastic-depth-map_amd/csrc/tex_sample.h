// tex_sample.h -- librsd's texture sampler, the one definition every kernel that filters a texture calls
// (DESIGN.md section 2 "Numerics").  D3D conventions: texel centres at integer + 0.5, so a sample at
// (u, v) lies x = u W - 0.5 texels from the centre of texel 0.  The fraction of x is quantised to 8
// sub-texel bits, round to nearest; a fraction that rounds to 256 / 256 carries into the next texel with
// weight 0.  The CPU oracle and the tests' checkers restate this rule on their own, bit for bit.
//
// Host and device (the RSD_HD pattern of bvh_refit.h): plain C++ without HIP, so that
// tests/native/check_tex_sample.cpp runs it under the sanitizers.  Float expressions round one by one in
// the order written (-ffp-contract=off, rsd_device.h).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RSD_HD __host__ __device__ inline
#else
#define RSD_HD inline
#endif

namespace rsd {

// Texel index under AddressMode::Wrap (Falcor's sampler default; a non-negative modulo) or Clamp
RSD_HD int tex_addr(int i, int n, bool wrap) {
    if (wrap) { i %= n; return i < 0 ? i + n : i; }
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// One axis of the rule: x = i + q / 256 with q in 0 .. 255 (kept as a float), w = q / 256.  Also the LOD
// fraction of alpha_sample.  Precondition: x is finite and floor(x) + 1 fits an int.
struct TexAxis {
    int i;
    float q, w;
};
RSD_HD TexAxis tex_split_axis(float x) {
    const float f0 = floorf(x);
    float q = floorf((x - f0) * 256.0f + 0.5f);
    int i = (int)f0;
    if (q >= 256.0f) { i += 1; q = 0.0f; }
    return TexAxis{i, q, q * (1.0f / 256.0f)};
}

// The bilinear footprint of (u, v) on a W x H texture: its taps are (ix, iy), (ix + 1, iy), (ix, iy + 1),
// (ix + 1, iy + 1) BEFORE addressing (they may lie outside the texture: tex_addr), weighted by wx, wy.
// Precondition: u W and v H are finite and within int range ((int)floorf of anything else is undefined on the host
// and saturates on the device).  The alpha test's coordinates meet it by the upload's contract: rsd_scene_upload_alpha
// refuses a sampled texcoord that is not finite or exceeds 32768 in magnitude (rsd.h rsd_alpha_desc.texcoords), and
// W, H <= 32768.
struct TexSplit {
    int ix, iy;
    float qx, qy, wx, wy;
};
RSD_HD TexSplit tex_split(int W, int H, float u, float v) {
    const TexAxis x = tex_split_axis(u * (float)W - 0.5f), y = tex_split_axis(v * (float)H - 0.5f);
    return TexSplit{x.i, y.i, x.q, y.q, x.w, y.w};
}

// All four taps of a footprint as offsets into a W x H image, addressed.  For the samplers that fetch all
// four whatever the weights; tex_bilinear (rsd_device.h) addresses its taps itself, after its early returns.
struct TexTaps {
    size_t t00, t10, t01, t11;
};
RSD_HD TexTaps tex_taps(const TexSplit& s, int W, int H, bool wrap) {
    const int x0 = tex_addr(s.ix, W, wrap), x1 = tex_addr(s.ix + 1, W, wrap);
    const int y0 = tex_addr(s.iy, H, wrap), y1 = tex_addr(s.iy + 1, H, wrap);
    return TexTaps{(size_t)y0 * W + x0, (size_t)y0 * W + x1, (size_t)y1 * W + x0, (size_t)y1 * W + x1};
}

// The filtered value of the four taps: x pairs first, then y
RSD_HD float tex_lerp(const TexSplit& s, float t00, float t10, float t01, float t11) {
    const float r0 = t00 * (1.0f - s.wx) + t10 * s.wx;
    const float r1 = t01 * (1.0f - s.wx) + t11 * s.wx;
    return r0 * (1.0f - s.wy) + r1 * s.wy;
}

// Texel of a point sample with clamp addressing: floor(uv n) clamped while still a float -- to
// [0, 2^31 - 128], the largest float an int holds -- so no out-of-range value is converted to an integer;
// a NaN coordinate addresses texel 0 (fmaxf returns its other operand).  The upper clamp to the texture
// is on the integer: n - 1 stays a scalar, where (float)(n - 1) would cost every lane a register.
RSD_HD int tex_point(float uv, int n) {
    const int t = (int)fminf(fmaxf(floorf(uv * (float)n), 0.0f), 2147483520.0f);
    return t > n - 1 ? n - 1 : t;
}

// The GuardBand pass's uv bounds of a width x height frame (GuardBand.cpp:62-63): the centres of the
// first and the last pixel inside the band.  Evaluated on the host, passed to the kernels as it is.
struct GuardUv {
    float minX, minY, maxX, maxY;
};
inline GuardUv guard_uv(uint32_t width, uint32_t height, uint32_t guard_band) {
    return GuardUv{((float)guard_band + 0.5f) / (float)width, ((float)guard_band + 0.5f) / (float)height,
                   ((float)width - ((float)guard_band + 0.5f)) / (float)width,
                   ((float)height - ((float)guard_band + 0.5f)) / (float)height};
}

}  // namespace rsd
