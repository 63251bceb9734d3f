/* temporal_peel_ref.c -- the CPU checker of the TemporalDepthPeel tests: a scalar restatement of the
 * Iterative implementation (TemporalDepthPeel.ps.slang:319-425) under librsd's definitions (DESIGN.md
 * section 2 "TemporalDepthPeel"), one pixel at a time, in float32 operation by operation
 * (gcc -ffp-contract=off, SSE arithmetic).  It shares no code with csrc/temporal_peel.hip.  Besides
 * depth2 it reports, per pixel, a flag word that says which parts of the shader the pixel went through
 * (the TP_* bits below), so that the tests can show their inputs reach every one of them.
 *
 * first_sample (optional, 3 floats per pixel) receives where each pixel's search starts, which the synthetic
 * inputs use to place a layer that the ray meets exactly.
 *
 * Built by tests/temporal_peel_checker.py. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define TP_EXIT_MASK 3u      /* how the search ended: */
#define TP_EXIT_UV 1u        /*   the search interval got shorter than half a texel in uv */
#define TP_EXIT_Z 2u         /*   the sample met the ray to within minSeparationDist * 0.001 */
#define TP_EXIT_ITER 3u      /*   maxIterations steps were taken */
#define TP_CLIPPED 4u        /* Cohen-Sutherland moved an end point */
#define TP_POINT 8u          /* some sample returned depthPoint (a texel above 0.99 farZ in its footprint) */
#define TP_QUIRK0 16u        /* ... and its largest weight was component 0: depthPoint = 0 */
#define TP_BEST_ZERO 32u     /* bestZ == 0: no information */
#define TP_CLIP_CAP 64u      /* the clip loop used all its 8 rounds without a verdict */
#define TP_OFFSCREEN 128u    /* the clip rejected the ray (both ends beyond the same edge) */
#define TP_ON_BOUND 256u     /* the best sample came back exactly at depth + minSeparationDist (not written: `>`) */

typedef struct { float x, y; } v2;
typedef struct { float x, y, z; } v3;

typedef struct {
    const float* prev2;
    int w, h;
    float far_z, scale_x, scale_y, sep;
    const float* to_prev; /* curViewToPrevView */
    const float* to_cur;  /* prevViewToCurView */
    int max_iter;
} ctx_t;

static float lerp1(float a, float b, float t) { return a + t * (b - a); }

static v2 lerp2(v2 a, v2 b, float t) {
    v2 r = { lerp1(a.x, b.x, t), lerp1(a.y, b.y, t) };
    return r;
}

/* mul(M, float4(p, 1)).xyz, each row summed left to right */
static v3 xform(const float* m, v3 p) {
    v3 r;
    r.x = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
    r.y = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
    r.z = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
    return r;
}

static v3 uv_to_view(const ctx_t* c, v2 uv, float view_depth) {
    float nx = uv.x * 2.0f - 1.0f;
    float ny = (1.0f - uv.y) * 2.0f - 1.0f;
    v3 r = { nx * view_depth * c->scale_x, ny * view_depth * c->scale_y, -view_depth };
    return r;
}

static v2 view_to_uv(const ctx_t* c, v3 p) {
    float nx = p.x / (c->scale_x * p.z);
    float ny = p.y / (c->scale_y * p.z);
    v2 r = { nx * -0.5f + 0.5f, ny * 0.5f + 0.5f };
    return r;
}

static unsigned outcode(v2 p) {
    unsigned code = 0;
    if (p.x < 0.0f) code |= 1u; /* LEFT */
    else if (p.x > 1.0f) code |= 2u; /* RIGHT */
    if (p.y < 0.0f) code |= 4u; /* BOTTOM */
    else if (p.y > 1.0f) code |= 8u; /* TOP */
    return code;
}

/* the shader's while (true), at most 8 rounds */
static unsigned clip_segment(v2* p0, v2* p1) {
    unsigned flags = 0, k0 = outcode(*p0), k1 = outcode(*p1);
    int rounds = 0;
    for (;;) {
        if ((k0 | k1) == 0) return flags;
        if ((k0 & k1) != 0) return flags | TP_OFFSCREEN;
        if (rounds == 8) return flags | TP_CLIP_CAP;
        ++rounds;
        unsigned out = k0 != 0 ? k0 : k1;
        v2 q;
        if (out & 8u) {
            q.x = p0->x + (p1->x - p0->x) * (1.0f - p0->y) / (p1->y - p0->y);
            q.y = 1.0f;
        } else if (out & 4u) {
            q.x = p0->x + (p1->x - p0->x) * (0.0f - p0->y) / (p1->y - p0->y);
            q.y = 0.0f;
        } else if (out & 2u) {
            q.y = p0->y + (p1->y - p0->y) * (1.0f - p0->x) / (p1->x - p0->x);
            q.x = 1.0f;
        } else {
            q.y = p0->y + (p1->y - p0->y) * (0.0f - p0->x) / (p1->x - p0->x);
            q.x = 0.0f;
        }
        flags |= TP_CLIPPED;
        if (out == k0) {
            *p0 = q;
            k0 = outcode(q);
        } else {
            *p1 = q;
            k1 = outcode(q);
        }
    }
}

/* Border addressing, colour 0: column col + dc, row row + dr of the previous layer, 0 off the image.
 * col and row are floor() results; whether the texel exists is decided on the floats. */
static float fetch(const ctx_t* c, float col, float row, float dc, float dr) {
    float cc = col + dc, rr = row + dr;
    int inside = cc >= 0.0f && cc <= (float)(c->w - 1) && rr >= 0.0f && rr <= (float)(c->h - 1);
    if (!inside) return 0.0f;
    return c->prev2[(size_t)(long)rr * (size_t)c->w + (size_t)(long)cc];
}

static float rectified_depth(const ctx_t* c, v2 uv, unsigned* flags) {
    float sx = uv.x * (float)c->w - 0.5f, sy = uv.y * (float)c->h - 0.5f;
    float col = floorf(sx), row = floorf(sy);
    float n[4], w[4], res[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    n[0] = fetch(c, col, row, 0.0f, 1.0f);
    n[1] = fetch(c, col, row, 1.0f, 1.0f);
    n[2] = fetch(c, col, row, 1.0f, 0.0f);
    n[3] = fetch(c, col, row, 0.0f, 0.0f);
    float fx = sx - floorf(sx), fy = sy - floorf(sy);
    w[0] = (1.0f - fx) * fy;
    w[1] = fx * fy;
    w[2] = fx * (1.0f - fy);
    w[3] = (1.0f - fx) * (1.0f - fy);
    float depth = 1.0f / (w[0] * (1.0f / n[0]) + w[1] * (1.0f / n[1]) + w[2] * (1.0f / n[2]) + w[3] * (1.0f / n[3]));
    int max_idx = 0;
    float max_val = w[0];
    for (int i = 1; i < 4; ++i)
        if (w[i] > max_val) {
            max_idx = i;
            max_val = w[i];
        }
    for (int i = 1; i < 4; ++i) /* from 1, as in the shader */
        if (i == max_idx) res[i] = 1.0f;
    float depth_point = res[0] * n[0] + res[1] * n[1] + res[2] * n[2] + res[3] * n[3];
    float lim = 0.99f * c->far_z;
    if (n[0] > lim || n[1] > lim || n[2] > lim || n[3] > lim) {
        *flags |= TP_POINT;
        if (max_idx == 0) *flags |= TP_QUIRK0;
        return depth_point;
    }
    return depth;
}

/* first: when not null, receives the first sample of the search (uv.x, uv.y, zRef; untouched when max_iter is 0) */
static float one_pixel(const ctx_t* c, int px, int py, float depth, unsigned* flags_out, float* first) {
    unsigned flags = 0;
    v2 tex = { ((float)px + 0.5f) / (float)c->w, ((float)py + 0.5f) / (float)c->h };
    v3 pmin = xform(c->to_prev, uv_to_view(c, tex, depth + c->sep));
    v3 pmax = xform(c->to_prev, uv_to_view(c, tex, c->far_z));
    v2 uv_min = view_to_uv(c, pmin), uv_max = view_to_uv(c, pmax);
    float z_min = -pmin.z, z_max = -pmax.z;
    flags |= clip_segment(&uv_min, &uv_max);

    float best_z = 0.0f, best_err = 1e10f, lo = 0.0f, hi = 1.0f;
    v2 best_uv = { 0.0f, 0.0f };
    float uv_eps = 0.5f / (float)c->w;
    unsigned how = TP_EXIT_ITER;
    for (int i = 0; i < c->max_iter; ++i) {
        float t = (lo + hi) * 0.5f;
        v2 uv = lerp2(uv_min, uv_max, t);
        float z_ref = 1.0f / lerp1(1.0f / z_min, 1.0f / z_max, t);
        if (i == 0 && first) {
            first[0] = uv.x;
            first[1] = uv.y;
            first[2] = z_ref;
        }
        float d = rectified_depth(c, uv, &flags);
        float err = fabsf(z_ref - d);
        if (err < best_err) {
            best_z = d;
            best_uv = uv;
            best_err = err;
        }
        v2 a = lerp2(uv_min, uv_max, lo), b = lerp2(uv_min, uv_max, hi);
        float dx = a.x - b.x, dy = a.y - b.y;
        if (sqrtf(dx * dx + dy * dy) < uv_eps) {
            how = TP_EXIT_UV;
            break;
        }
        if (fabsf(d - z_ref) < c->sep * 0.001f) {
            how = TP_EXIT_Z;
            break;
        } else if (z_ref < d) {
            lo = t;
        } else {
            hi = t;
        }
    }
    flags |= how;

    float found = 0.0f;
    if (best_z == 0.0f) {
        flags |= TP_BEST_ZERO;
    } else {
        v3 p = xform(c->to_cur, uv_to_view(c, best_uv, best_z));
        if (-p.z == depth + c->sep) flags |= TP_ON_BOUND;
        if (-p.z > depth + c->sep && -p.z < 0.99f * c->far_z) found = -p.z;
    }
    *flags_out = flags;
    float out = depth;
    if (found > depth + c->sep) out = found;
    return out;
}

void temporal_peel_ref(const float* linear_z, const float* prev_depth2, uint32_t width, uint32_t height,
                       float far_z, float frame_width, float frame_height, float focal_length,
                       const float* cur_view_to_prev_view, const float* prev_view_to_cur_view, float min_separation,
                       int32_t max_iterations, float* depth2, uint32_t* flags, float* first_sample) {
    ctx_t c;
    c.prev2 = prev_depth2;
    c.w = (int)width;
    c.h = (int)height;
    c.far_z = far_z;
    c.scale_x = 0.5f * (frame_width / focal_length);
    c.scale_y = 0.5f * (frame_height / focal_length);
    c.sep = min_separation;
    c.to_prev = cur_view_to_prev_view;
    c.to_cur = prev_view_to_cur_view;
    c.max_iter = max_iterations;
    for (int y = 0; y < c.h; ++y)
        for (int x = 0; x < c.w; ++x) {
            size_t o = (size_t)y * width + (size_t)x;
            unsigned f = 0;
            depth2[o] = one_pixel(&c, x, y, linear_z[o], &f, first_sample ? first_sample + 3 * o : NULL);
            flags[o] = f;
        }
}
