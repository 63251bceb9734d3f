/* ao_resolve_ref.c -- scalar CPU restatement of the reference's AOGuidedBlur and AOVarianceFix pixel shaders
 * (AOGuidedBlur.ps.slang, AOVarianceFix.ps.slang, and the slice loops of AOGuidedBlur.cpp / AOVarianceFix.cpp),
 * written from the shaders alone: it shares no code with csrc/ao_resolve.hip.  The GPU tests compare bit for bit
 * against it; tests/test_ao_resolve.py pins it with answers known in advance.
 *
 * Conventions (DESIGN.md "AO resolve"): binary32, one rounding per operation (build with -ffp-contract=off and
 * SSE arithmetic), exp evaluated in double and rounded once, HLSL min / max return the non-NaN operand,
 * saturate(NaN) = 0, unorm8 store = floor(saturate(x) * 255 + 0.5), unorm8 load = c / 255, point sampling =
 * clamp(floor(uv * n)), linear sampling = the 8-bit sub-texel bilinear rule with clamp addressing.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum {
    C_TAP_ZERO = 0,      /* taps whose depth weight is exactly 0 */
    C_TAP_HALF = 1,      /* taps whose depth weight is above 0.5 */
    C_TAP_CLAMPED = 2,   /* taps whose uv the clamp to [uvMin, uvMax] changed */
    C_FALLBACK_X = 3,    /* x-pass pixels with weightSum < 1e-4 */
    C_FALLBACK_Y = 4,    /* y-pass pixels with weightSum < 1e-4 */
    C_LDEV_RAISED = 5,   /* pixels whose ldev.y was raised to DARK_EPSILON */
    C_LDEV_KEPT = 6,     /* ... and those where it was not */
    C_ADEV_RAISED = 7,   /* the same for adev.y (AOVarianceFix: its only deviation) */
    C_ADEV_KEPT = 8,
    C_TIE_OUT = 9,       /* outputs with x * 255 exactly half way between two bytes */
    C_TIE_PING = 10,     /* the same for the four ping-pong channels */
    C_MEANS_FALLBACK = 11, /* AOVarianceFix pixels with a mean below 1e-4 */
    C_WRITTEN = 12,      /* pixels inside the scissor */
    C_COUNT = 16
};

typedef struct { float x, y; } f2;
typedef struct { float x, y, z, w; } f4;

typedef struct {
    int w, h;           /* the slice */
    f2 uv_min, uv_max;  /* ScissorCB */
    uint64_t* counters;
} ctx_t;

static float hmin(float a, float b) { return fminf(a, b); }
static float hmax(float a, float b) { return fmaxf(a, b); }
static float sat(float x) { return !(x > 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x); }
static float gauss(float offset, float variance) { return (float)exp((double)(-0.5f * offset * offset / variance)); }

static uint8_t to_unorm8(float x, uint64_t* tie) {
    if (x != x) return 0;
    x = sat(x);
    const float s = x * 255.0f;
    if (tie && s - floorf(s) == 0.5f) *tie += 1;
    return (uint8_t)floorf(s + 0.5f);
}
static float from_unorm8(uint8_t c) { return (float)c / 255.0f; }

static f2 clamp_uv(const ctx_t* c, f2 uv, int count) {
    f2 r;
    r.x = hmin(hmax(uv.x, c->uv_min.x), c->uv_max.x);
    r.y = hmin(hmax(uv.y, c->uv_min.y), c->uv_max.y);
    if (count && (r.x != uv.x || r.y != uv.y)) c->counters[C_TAP_CLAMPED] += 1;
    return r;
}

static int point_index(const ctx_t* c, f2 uv) {
    int tx = (int)floorf(uv.x * (float)c->w), ty = (int)floorf(uv.y * (float)c->h);
    if (tx < 0) tx = 0;
    if (tx > c->w - 1) tx = c->w - 1;
    if (ty < 0) ty = 0;
    if (ty > c->h - 1) ty = c->h - 1;
    return ty * c->w + tx;
}

/* a point sample of an 8-bit image with `channels` bytes per texel; missing channels read 0 */
static f4 point_unorm(const ctx_t* c, const uint8_t* tex, int channels, f2 uv) {
    const uint8_t* t = tex + (size_t)point_index(c, uv) * channels;
    f4 r = {0.0f, 0.0f, 0.0f, 0.0f};
    r.x = from_unorm8(t[0]);
    if (channels > 1) r.y = from_unorm8(t[1]);
    if (channels > 2) r.z = from_unorm8(t[2]);
    if (channels > 3) r.w = from_unorm8(t[3]);
    return r;
}

static int scissor_of(int guard_band, int layers) {
    return layers > 1 ? guard_band / (int)(sqrt((double)layers) + 0.5) : guard_band;
}

static void uv_bounds(ctx_t* c, int full_w, int full_h, int guard_band) {
    c->uv_min.x = ((float)guard_band + 0.5f) / (float)full_w;
    c->uv_min.y = ((float)guard_band + 0.5f) / (float)full_h;
    c->uv_max.x = ((float)full_w - ((float)guard_band + 0.5f)) / (float)full_w;
    c->uv_max.y = ((float)full_h - ((float)guard_band + 0.5f)) / (float)full_h;
}

/* ------------------------------------------------------------------------------------------ AOGuidedBlur
 * main() of AOGuidedBlur.ps.slang for one pixel and one direction; src has src_channels bytes per texel. */
static void guided_pixel(const ctx_t* c, const uint8_t* src, int src_channels, const float* depth,
                         const uint8_t* bright_dark, int bd_channels, f2 dir, int radius, int local_deviation,
                         int px, int py, uint8_t* out_rgba, uint8_t* out_r) {
    uint64_t* n = c->counters;
    const int second = dir.y != 0.0f;
    f2 texc = {((float)px + 0.5f) / (float)c->w, ((float)py + 0.5f) / (float)c->h};
    f2 means = {0.0f, 0.0f}, means_sq = {0.0f, 0.0f};
    float weight_sum = 0.0f;
    const float local_depth = hmax(depth[point_index(c, clamp_uv(c, texc, 0))], 1.401298e-45f);
    const f4 local4 = point_unorm(c, src, src_channels, clamp_uv(c, texc, 0));
    const f2 local = {local4.x, local4.y};
    f2 uv_step = {(1.0f / (float)c->w) * dir.x, (1.0f / (float)c->h) * dir.y};
    f2 uv = {texc.x - uv_step.x * (float)radius, texc.y - uv_step.y * (float)radius};
    for (int it = 0; it <= radius * 2; ++it) {
        const float spatial = gauss((float)(radius - it), 16.4f);
        const f2 cuv = clamp_uv(c, uv, 1);
        const f4 s = point_unorm(c, src, src_channels, cuv);
        f2 ao = {s.x, s.y};
        f2 ao_sq = {ao.x * ao.x, ao.y * ao.y};
        if (second) {
            ao_sq.x = s.z;
            ao_sq.y = s.w;
        }
        const float relative = hmin(fabsf(depth[point_index(c, cuv)] / local_depth - 1.0f), 1.0f);
        const float depth_weight = gauss(relative, 0.001f);
        if (depth_weight == 0.0f) n[C_TAP_ZERO] += 1;
        if (depth_weight > 0.5f) n[C_TAP_HALF] += 1;
        const float w = spatial * depth_weight * 1.0f;
        weight_sum += w;
        means.x += w * ao.x;
        means.y += w * ao.y;
        means_sq.x += w * ao_sq.x;
        means_sq.y += w * ao_sq.y;
        uv.x += uv_step.x;
        uv.y += uv_step.y;
    }
    const float d = hmax(weight_sum, 1e-4f);
    means.x /= d;
    means.y /= d;
    means_sq.x /= d;
    means_sq.y /= d;
    if (weight_sum < 1e-4f) {
        n[second ? C_FALLBACK_Y : C_FALLBACK_X] += 1;
        means = local;
        means_sq.x = local.x * local.x;
        means_sq.y = local.y * local.y;
    }
    if (!second) {
        out_rgba[0] = to_unorm8(means.x, &n[C_TIE_PING]);
        out_rgba[1] = to_unorm8(means.y, &n[C_TIE_PING]);
        out_rgba[2] = to_unorm8(means_sq.x, &n[C_TIE_PING]);
        out_rgba[3] = to_unorm8(means_sq.y, &n[C_TIE_PING]);
        return;
    }
    float col = means.x;
    const f4 o4 = point_unorm(c, bright_dark, bd_channels, clamp_uv(c, texc, 0));
    const f2 original = {o4.x, o4.y};
    f2 ldev = {fabsf(original.x - means.x), fabsf(original.y - means.y)}; /* pow(., 1.0) */
    n[ldev.y < 0.01f ? C_LDEV_RAISED : C_LDEV_KEPT] += 1;
    ldev.y = hmax(ldev.y, 0.01f);
    ldev.x *= 1.0f;
    f2 wt = {ldev.y / (ldev.x + ldev.y), ldev.x / (ldev.x + ldev.y)};
    if (local_deviation) col = original.x * wt.x + original.y * wt.y;
    f2 adev = {sqrtf(fabsf(means_sq.x - means.x * means.x)), sqrtf(fabsf(means_sq.y - means.y * means.y))};
    n[adev.y < 0.01f ? C_ADEV_RAISED : C_ADEV_KEPT] += 1;
    adev.y = hmax(adev.y, 0.01f);
    adev.x *= 1.0f;
    wt.x = adev.y / (adev.x + adev.y);
    wt.y = adev.x / (adev.x + adev.y);
    if (!local_deviation) col = original.x * wt.x + original.y * wt.y;
    *out_r = to_unorm8(col, &n[C_TIE_OUT]);
}

/* src: [layers][qh][qw][src_channels] bytes; depth: [layers][qh][qw]; pingpong: [layers][qh][qw][4];
 * dst: [layers][qh][qw].  Texels outside the scissor keep what pingpong and dst held. */
void ao_guided_blur_ref(const uint8_t* src, int src_channels, const float* depth, int qw, int qh, int layers,
                        int full_w, int full_h, int guard_band, int radius, int local_deviation, uint8_t* pingpong,
                        uint8_t* dst, uint64_t* counters) {
    ctx_t c;
    c.w = qw;
    c.h = qh;
    c.counters = counters;
    memset(counters, 0, C_COUNT * sizeof(uint64_t));
    uv_bounds(&c, full_w, full_h, guard_band);
    const int g = scissor_of(guard_band, layers);
    const size_t plane = (size_t)qw * qh;
    const f2 dir_x = {1.0f, 0.0f}, dir_y = {0.0f, 1.0f};
    for (int slice = 0; slice < layers; ++slice) {
        const uint8_t* s = src + slice * plane * src_channels;
        const float* z = depth + slice * plane;
        uint8_t* pp = pingpong + slice * plane * 4;
        uint8_t* out = dst + slice * plane;
        for (int y = g; y < qh - g; ++y)
            for (int x = g; x < qw - g; ++x)
                guided_pixel(&c, s, src_channels, z, s, src_channels, dir_x, radius, local_deviation, x, y,
                             pp + ((size_t)y * qw + x) * 4, 0);
        for (int y = g; y < qh - g; ++y)
            for (int x = g; x < qw - g; ++x) {
                guided_pixel(&c, pp, 4, z, s, src_channels, dir_y, radius, local_deviation, x, y, 0,
                             out + (size_t)y * qw + x);
                counters[C_WRITTEN] += 1;
            }
    }
}

/* ------------------------------------------------------------------------------------------ AOVarianceFix */
typedef struct {
    int i00, i10, i01, i11;
    float wx, wy;
} taps_t;

static int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

static taps_t linear_taps(const ctx_t* c, f2 uv) {
    taps_t t;
    const float x = uv.x * (float)c->w - 0.5f, y = uv.y * (float)c->h - 0.5f;
    const float fx = floorf(x), fy = floorf(y);
    float qx = floorf((x - fx) * 256.0f + 0.5f), qy = floorf((y - fy) * 256.0f + 0.5f);
    int ix = (int)fx, iy = (int)fy;
    if (qx >= 256.0f) {
        ix += 1;
        qx = 0.0f;
    }
    if (qy >= 256.0f) {
        iy += 1;
        qy = 0.0f;
    }
    const int x0 = clampi(ix, c->w), x1 = clampi(ix + 1, c->w), y0 = clampi(iy, c->h), y1 = clampi(iy + 1, c->h);
    t.i00 = y0 * c->w + x0;
    t.i10 = y0 * c->w + x1;
    t.i01 = y1 * c->w + x0;
    t.i11 = y1 * c->w + x1;
    t.wx = qx * (1.0f / 256.0f);
    t.wy = qy * (1.0f / 256.0f);
    return t;
}
static float blend(const taps_t* t, float a, float b, float cc, float d) {
    const float r0 = a * (1.0f - t->wx) + b * t->wx, r1 = cc * (1.0f - t->wx) + d * t->wx;
    return r0 * (1.0f - t->wy) + r1 * t->wy;
}
static float linear_unorm(const ctx_t* c, const uint8_t* tex, f2 uv) {
    const taps_t t = linear_taps(c, uv);
    return blend(&t, from_unorm8(tex[t.i00]), from_unorm8(tex[t.i10]), from_unorm8(tex[t.i01]), from_unorm8(tex[t.i11]));
}
static float linear_float(const ctx_t* c, const float* tex, f2 uv) {
    const taps_t t = linear_taps(c, uv);
    return blend(&t, tex[t.i00], tex[t.i10], tex[t.i01], tex[t.i11]);
}

static uint8_t variance_pixel(const ctx_t* c, const uint8_t* bright, const uint8_t* dark, const float* depth, int px,
                              int py) {
    static const f2 offsets[4] = {{-1.0f, 0.0f}, {0.0f, -1.0f}, {1.0f, 0.0f}, {0.0f, 1.0f}};
    uint64_t* n = c->counters;
    const f2 texc = {((float)px + 0.5f) / (float)c->w, ((float)py + 0.5f) / (float)c->h};
    const f2 ctc = clamp_uv(c, texc, 0);
    const float local_depth = hmax(linear_float(c, depth, ctc), 1.401298e-45f);
    const f2 local = {linear_unorm(c, bright, ctc), linear_unorm(c, dark, ctc)};
    f2 means = local;
    float weight_sum = 1.0f;
    const f2 uv_step = {1.0f / (float)c->w, 1.0f / (float)c->h};
    for (int it = 0; it < 4; ++it) {
        const f2 uv = {texc.x + offsets[it].x * uv_step.x, texc.y + offsets[it].y * uv_step.y};
        const f2 cuv = clamp_uv(c, uv, 1);
        const float spatial = gauss(offsets[it].x, 10.0f) * gauss(offsets[it].y, 10.0f);
        const float relative = sat(fabsf(linear_float(c, depth, cuv) / local_depth - 1.0f));
        const float depth_weight = gauss(relative, 0.001f);
        if (depth_weight == 0.0f) n[C_TAP_ZERO] += 1;
        if (depth_weight > 0.5f) n[C_TAP_HALF] += 1;
        const float w = spatial * 1.0f * depth_weight;
        weight_sum += w;
        means.x += w * linear_unorm(c, bright, cuv);
        means.y += w * linear_unorm(c, dark, cuv);
    }
    const float d = hmax(weight_sum, 1e-4f);
    means.x /= d;
    means.y /= d;
    if (means.x < 1e-4f || means.y < 1e-4f) {
        n[C_MEANS_FALLBACK] += 1;
        means = local;
    }
    f2 adev = {fabsf(local.x - means.x), fabsf(local.y - means.y)};
    n[adev.y < 0.01f ? C_ADEV_RAISED : C_ADEV_KEPT] += 1;
    adev.y = hmax(adev.y, 0.01f);
    const f2 wt = {adev.y / (adev.x + adev.y), adev.x / (adev.x + adev.y)};
    return to_unorm8(local.x * wt.x + local.y * wt.y, &n[C_TIE_OUT]);
}

void ao_variance_fix_ref(const uint8_t* bright, const uint8_t* dark, const float* depth, int qw, int qh, int layers,
                         int full_w, int full_h, int guard_band, uint8_t* dst, uint64_t* counters) {
    ctx_t c;
    c.w = qw;
    c.h = qh;
    c.counters = counters;
    memset(counters, 0, C_COUNT * sizeof(uint64_t));
    uv_bounds(&c, full_w, full_h, guard_band);
    const int g = scissor_of(guard_band, layers);
    const size_t plane = (size_t)qw * qh;
    for (int slice = 0; slice < layers; ++slice)
        for (int y = g; y < qh - g; ++y)
            for (int x = g; x < qw - g; ++x) {
                dst[slice * plane + (size_t)y * qw + x] =
                    variance_pixel(&c, bright + slice * plane, dark + slice * plane, depth + slice * plane, x, y);
                counters[C_WRITTEN] += 1;
            }
}
