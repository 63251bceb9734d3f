/* hbao_ref.c -- the CPU checker of the HBAO tests: a scalar restatement of the reference's HBAO pixel shader
 * (HBAO.ps.slang:134-247 with HBAOData.slang and the per-slice constants of HBAO.cpp:159-193), one texel of
 * one layer at a time, written from the shader and sharing no code with csrc/hbao.hip.  Built by
 * tests/hbao_checker.py with gcc -O2 -ffp-contract=off -msse2 -mfpmath=sse: binary32, one rounding per
 * operation, in the order the shader writes them.
 *
 * librsd's definitions where HLSL leaves things open (DESIGN.md section 2 "HBAO"):
 *   rsqrt(x) = 1 / sqrt(x); saturate(NaN) = 0; max(a, NaN) = a; lerp(a, b, t) = a + t (b - a);
 *   round = round half to even; cos / sin / pow evaluated in double and rounded once (pow(x, 2) = x x);
 *   a point sample addresses texel clamp(floor(uv n), 0, n - 1), and texel 0 for a NaN coordinate;
 *   RG8Unorm stores floor(saturate(v) 255 + 0.5).
 *
 * Besides the bytes every texel gets a flag word saying which way it went. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define HB_FAR 1u       /* linearDepth >= farZ: (1, 1) */
#define HB_SMALL 2u     /* RadiusInPixels < 1: (1, 1) */
#define HB_SCISSORED 4u /* outside the guard-band scissor: not written */
#define HB_RAGGED 8u    /* the texel's full-resolution pixel lies outside the frame */
#define HB_NAN_TAP 16u  /* a tap whose NdotV is NaN (VdotV is 0: 0 * inf, or NaN), which saturate turns into 0 */
#define HB_TIE 32u      /* a tap whose RayPixels * Direction lies exactly between two texels (round half to even) */
#define HB_RECOMPUTE_SHIFT 8/* bits 8..15: taps for which RecomputeAO asked for the second layer */

typedef struct { float x, y; } vec2;
typedef struct { float x, y, z; } vec3;

typedef struct {
    const float *depth, *depth2, *normal;
    int W, H, qw, qh;
    float far_z, scale_x, scale_y;
    float radius, neg_inv_rsq, bias, exponent;
    const float* view;
    int dual;
} hb_ctx;

static float sat(float v) { return v > 0.0f ? (v > 1.0f ? 1.0f : v) : 0.0f; /* NaN > 0 is false */ }

static int texel_of(float uv, int n) {
    float t = floorf(uv * (float)n);
    if (isnan(t) || t < 0.0f) return 0;
    if (t > (float)(n - 1)) return n - 1;
    return (int)t;
}

/* Texture2D<float>.SampleLevel(point / clamp sampler, uv, 0) of layer `layer` */
static float sample_quarter(const hb_ctx* c, const float* tex, int layer, vec2 uv) {
    int tx = texel_of(uv.x, c->qw), ty = texel_of(uv.y, c->qh);
    return tex[((size_t)layer * c->qh + ty) * c->qw + tx];
}

/* UVToViewSpace (:62-67) */
static vec3 uv_to_view(const hb_ctx* c, vec2 uv, float view_depth) {
    vec2 ndc;
    vec3 p;
    ndc.x = uv.x * 2.0f - 1.0f;
    ndc.y = (1.0f - uv.y) * 2.0f - 1.0f;
    p.x = ndc.x * view_depth * c->scale_x;
    p.y = ndc.y * view_depth * c->scale_y;
    p.z = -view_depth;
    return p;
}

static float dot3(vec3 a, vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

/* the two terms of ComputeAO / RecomputeAO (:112-131); returns whether NdotV is NaN */
static int kernel_terms(const hb_ctx* c, vec3 P, vec3 N, vec3 S, float* angle, float* distance) {
    vec3 V;
    float vdotv, ndotv;
    V.x = S.x - P.x;
    V.y = S.y - P.y;
    V.z = S.z - P.z;
    vdotv = dot3(V, V);
    ndotv = dot3(N, V) * (1.0f / sqrtf(vdotv));
    *angle = sat(ndotv - c->bias);
    *distance = sat(vdotv * c->neg_inv_rsq + 1.0f); /* Falloff(...).x; .y is 1 */
    return isnan(ndotv);
}

static uint8_t unorm8(float v) { return (uint8_t)floorf(sat(v) * 255.0f + 0.5f); }

static float power(float x, float y) { return y == 2.0f ? x * x : (float)pow((double)x, (double)y); }

/* main() of the shader for layer `layer`, quarter texel (qx, qy); returns the flags, writes rg[2] */
static uint32_t shade(const hb_ctx* c, int layer, int qx, int qy, const float rnd[4], const vec2 dir[8], uint8_t rg[2]) {
    uint32_t flags = 0, recompute = 0;
    vec2 sv, texc;
    vec3 P, N, Nw;
    float linear_depth, radius_px, step_px, ax, ay, rx, ry;
    const float* nt;
    int i, step;
    sv.x = floorf((float)qx + 0.5f) * 4.0f + (float)(layer % 4) + 0.5f; /* :137 */
    sv.y = floorf((float)qy + 0.5f) * 4.0f + (float)(layer / 4) + 0.5f;
    if (sv.x > (float)c->W || sv.y > (float)c->H) flags |= HB_RAGGED;
    texc.x = sv.x * (1.0f / (float)c->W); /* invResolution = float2(1) / resolution (HBAO.cpp:163) */
    texc.y = sv.y * (1.0f / (float)c->H);
    rg[0] = rg[1] = 255;
    linear_depth = sample_quarter(c, c->depth, layer, texc);
    if (linear_depth >= c->far_z) return flags | HB_FAR;
    P = uv_to_view(c, texc, linear_depth);
    nt = c->normal + ((size_t)texel_of(texc.y, c->H) * c->W + texel_of(texc.x, c->W)) * 4;
    Nw.x = nt[0];
    Nw.y = nt[1];
    Nw.z = nt[2];
    N.x = c->view[0] * Nw.x + c->view[1] * Nw.y + c->view[2] * Nw.z; /* mul(float3x3(viewMat), n) */
    N.y = c->view[4] * Nw.x + c->view[5] * Nw.y + c->view[6] * Nw.z;
    N.z = c->view[8] * Nw.x + c->view[9] * Nw.y + c->view[10] * Nw.z;
    if (dot3(P, N) > 0.0f) {
        N.x = -N.x;
        N.y = -N.y;
        N.z = -N.z;
    }
    { /* GetAORadiusInPixels (:80-93) */
        float ux = c->radius / (c->scale_x * linear_depth) * 0.5f;
        float uy = c->radius / (c->scale_y * linear_depth) * 0.5f;
        float a = ux * (float)c->W, b = uy * (float)c->H;
        radius_px = a + 0.5f * (b - a);
    }
    if (radius_px < 1.0f) return flags | HB_SMALL;
    step_px = (radius_px / 4.0f) / 5.0f;
    ax = ay = 0.0f;
    for (i = 0; i < 8; ++i) {
        float ray_px = rnd[2] * step_px + 1.0f;
        for (step = 0; step < 4; ++step) {
            vec2 uv;
            vec3 S;
            float angle, distance, bright, dark, d;
            float ox = ray_px * dir[i].x, oy = ray_px * dir[i].y;
            if (fabsf(ox - truncf(ox)) == 0.5f || fabsf(oy - truncf(oy)) == 0.5f) flags |= HB_TIE;
            uv.x = texc.x + rintf(ox) * (1.0f / (float)c->qw);
            uv.y = texc.y + rintf(oy) * (1.0f / (float)c->qh);
            d = sample_quarter(c, c->depth, layer, uv);
            S = uv_to_view(c, uv, d);
            if (kernel_terms(c, P, N, S, &angle, &distance)) flags |= HB_NAN_TAP;
            bright = angle * distance;
            dark = angle * 1.0f;
            if (c->dual && angle > 0.0f && distance <= 0.0f) { /* RecomputeAO returned true */
                float angle2, distance2, b2, d2;
                ++recompute;
                d = sample_quarter(c, c->depth2, layer, uv);
                S = uv_to_view(c, uv, d);
                if (kernel_terms(c, P, N, S, &angle2, &distance2)) flags |= HB_NAN_TAP;
                b2 = angle2 * distance2;
                d2 = angle2 * 1.0f;
                if (b2 > bright) bright = b2;
                if (d2 > dark) dark = d2;
            }
            ax += bright;
            ay += dark;
            ray_px += step_px;
        }
    }
    ax /= 32.0f;
    ay /= 32.0f;
    rx = power(sat(1.0f - ax * 2.0f), c->exponent);
    ry = power(sat(1.0f - ay * 2.0f), c->exponent);
    rg[0] = unorm8(rx);
    rg[1] = unorm8(ry);
    return flags | (recompute << HB_RECOMPUTE_SHIFT);
}

/* depth / depth2: [16][qh][qw] floats; normal_w: [H][W][4]; view: the camera's 4 x 4 row-major view matrix;
 * rnd: [16][4]; out: [16][qh][qw][2] bytes, written inside the scissor only; flags: [16][qh][qw] */
void hbao_ref(const float* depth, const float* depth2, const float* normal_w, uint32_t W, uint32_t H, float far_z,
              float frame_w, float frame_h, float focal, const float* view, float radius, float bias, float exponent,
              uint32_t depth_mode, uint32_t guard_band, const float* rnd, uint8_t* out, uint32_t* flags) {
    hb_ctx c;
    int layer, qx, qy, i, g = (int)(guard_band / 4u);
    const float alpha = 2.0f * 3.141f / 8.0f;
    c.depth = depth;
    c.depth2 = depth2;
    c.normal = normal_w;
    c.W = (int)W;
    c.H = (int)H;
    c.qw = (int)((W + 3u) / 4u);
    c.qh = (int)((H + 3u) / 4u);
    c.far_z = far_z;
    c.scale_x = 0.5f * (frame_w / focal);
    c.scale_y = 0.5f * (frame_h / focal);
    c.radius = radius;
    c.neg_inv_rsq = -1.0f / (radius * radius);
    c.bias = bias;
    c.exponent = exponent;
    c.view = view;
    c.dual = depth_mode == 1u;
    for (layer = 0; layer < 16; ++layer) {
        const float* r = rnd + 4 * layer;
        vec2 dir[8];
        for (i = 0; i < 8; ++i) { /* Rotate2D(Rand.xy, Alpha * i) (:48-57) */
            float theta = alpha * (float)i;
            float ct = (float)cos((double)theta), st = (float)sin((double)theta);
            dir[i].x = r[0] * ct - r[1] * st;
            dir[i].y = r[0] * st + r[1] * ct;
        }
        for (qy = 0; qy < c.qh; ++qy)
            for (qx = 0; qx < c.qw; ++qx) {
                size_t o = ((size_t)layer * c.qh + qy) * c.qw + qx;
                uint8_t rg[2];
                uint32_t f = shade(&c, layer, qx, qy, r, dir, rg);
                if (qx < g || qy < g || qx >= c.qw - g || qy >= c.qh - g) {
                    flags[o] = f | HB_SCISSORED;
                    continue;
                }
                flags[o] = f;
                out[2 * o] = rg[0];
                out[2 * o + 1] = rg[1];
            }
    }
}

/* The checker's own MT19937 (seed 0) and the noise table of HBAO::genNoiseTexture (HBAO.cpp:225-251):
 * per entry theta in [0, 2 * 3.141f), r1, r2, a draw u mapped to (float)u / 2^32.  first3: the first raw draws. */
static uint32_t mt_state[624];
static int mt_pos;

static void mt_seed(uint32_t s) {
    int i;
    mt_state[0] = s;
    for (i = 1; i < 624; ++i) mt_state[i] = 1812433253u * (mt_state[i - 1] ^ (mt_state[i - 1] >> 30)) + (uint32_t)i;
    mt_pos = 624;
}

static uint32_t mt_draw(void) {
    uint32_t y;
    if (mt_pos == 624) {
        int k;
        for (k = 0; k < 624; ++k) {
            uint32_t u = (mt_state[k] & 0x80000000u) | (mt_state[(k + 1) % 624] & 0x7fffffffu);
            uint32_t v = mt_state[(k + 397) % 624] ^ (u >> 1);
            if (u & 1u) v ^= 0x9908b0dfu;
            mt_state[k] = v;
        }
        mt_pos = 0;
    }
    y = mt_state[mt_pos++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

void hbao_ref_noise(float* out64, uint32_t* first3, float* theta0) {
    int i;
    mt_seed(0u);
    for (i = 0; i < 3; ++i) first3[i] = mt_draw();
    mt_seed(0u);
    for (i = 0; i < 16; ++i) {
        float theta = ((float)mt_draw() / 4294967296.0f) * (2.0f * 3.141f);
        float r1 = (float)mt_draw() / 4294967296.0f;
        float r2 = (float)mt_draw() / 4294967296.0f;
        if (i == 0) *theta0 = theta;
        out64[4 * i + 0] = (float)sin((double)theta);
        out64[4 * i + 1] = (float)cos((double)theta);
        out64[4 * i + 2] = r1;
        out64[4 * i + 3] = r2;
    }
}
