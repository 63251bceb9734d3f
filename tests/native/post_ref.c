/* post_ref.c -- the scalar checker of the post-AO image passes (tests/post_checker.py).
 *
 * A restatement of the reference's shader text, one texel at a time, written from that text: it includes no header
 * of csrc/ or oracle/ and takes no line from them (loop headers and one-operation statements that the shader
 * dictates inevitably read alike).  The motion vectors have no shader: they follow librsd's definition in
 * include/rsd_graph.h, whose operation order the bit-for-bit comparison fixes.  The passes: CrossBilateralBlur, TAA, Deinterleave / Interleave, RayMinMaxLength,
 * AOFlickerMask, BinaryDilation, TemporalAO and the two motion-vector entries.  (ImageEquation, the ninth
 * operation, is evaluated from the formula text in post_checker.py.)
 *
 * Built with gcc -O2 -ffp-contract=off -msse2 -mfpmath=sse: binary32, one rounding per operation, in the order
 * the shader writes them.  Transcendentals are evaluated in double and rounded once (librsd's numerics).
 *
 * The texture rules, restated here and used by every pass below:
 *   T1  point sampling, clamp: texel floor(uv * size) clamped into the image.
 *   T2  linear sampling: the sample position in texels is uv * size - 0.5; its fraction is quantised to 8 bits,
 *       round(frac * 256) with halves up, and a fraction that rounds to 256 moves to the next texel with weight
 *       0; rows are blended first (a (1 - wx) + b wx), then the two rows ((1 - wy) r0 + wy r1).  Address modes:
 *       wrap (Falcor's default sampler) or clamp.
 *   T3  Gather: the 2 x 2 footprint of T2 (the four texels linear sampling would blend), whatever the weights.
 *   T4  Load / operator[] outside the image reads 0.
 *   T5  UNORM8 store: NaN -> 0, clamp to [0, 1], floor(x * 255 + 0.5); UNORM8 load: c / 255.
 *   T6  HLSL min / max / clamp return the non-NaN operand.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

/* ------------------------------------------------------------------------------------------------ rules */
static float h_min(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }            /* T6 */
static float h_max(float a, float b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }            /* T6 */
static float h_clamp(float x, float lo, float hi) { return h_min(h_max(x, lo), hi); }
static float h_saturate(float x) { return h_min(h_max(x, 0.0f), 1.0f); }                                /* NaN -> 0 */

static uint8_t st_unorm8(float x)                                                                       /* T5 */
{
    if (x != x) return 0;
    if (x < 0.0f) x = 0.0f;
    if (x > 1.0f) x = 1.0f;
    return (uint8_t)(int)floorf(x * 255.0f + 0.5f);
}
static float ld_unorm8(uint8_t c) { return (float)c / 255.0f; }                                         /* T5 */

static float centre_uv(int i, int n) { return ((float)i + 0.5f) / (float)n; }       /* texC of a pixel centre */
static int clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }
static int wrapi(int i, int n) { int r = i % n; return r < 0 ? r + n : r; }
static int point_index(float uv, int n) { return clampi((int)floorf(uv * (float)n), 0, n - 1); }        /* T1 */

typedef struct { int i0, i1; float w; } lin_axis;

/* T2 along one axis: the two texel indices (before addressing) and the weight of the second */
static lin_axis linear_axis(float uv, int n)
{
    const float p = uv * (float)n - 0.5f;
    const float base = floorf(p);
    float q = floorf((p - base) * 256.0f + 0.5f);
    lin_axis a;
    a.i0 = (int)base;
    if (q >= 256.0f) { a.i0 += 1; q = 0.0f; }
    a.i1 = a.i0 + 1;
    a.w = q / 256.0f;
    return a;
}
static float blend(float t00, float t10, float t01, float t11, float wx, float wy)
{
    const float r0 = t00 * (1.0f - wx) + t10 * wx;
    const float r1 = t01 * (1.0f - wx) + t11 * wx;
    const float keep = 1.0f - wy;
    return r0 * keep + r1 * wy;
}

/* ------------------------------------------------------------------------------- CrossBilateralBlur
 * CrossBilateralBlur.ps.slang:28-88; the sampler is point / clamp (CrossBilateralBlur.cpp:50), the two passes
 * x then y through the ping-pong image (CrossBilateralBlur.cpp:138-148), uvMin / uvMax GuardBand.cpp:62-63. */

/* CrossBilateralBlur.ps.slang:28-43: the weight of tap d (1..R) of one side; depth is the tap's depth */
static float blur_weight(int R, float depth, float centre, float slope, unsigned d)
{
    const float blur_sigma = ((float)R + 1.0f) * 0.5f, two_sigma = 2.0f * blur_sigma;   /* :31 */
    const float falloff = 1.0f / (two_sigma * blur_sigma);                            /* :32, 2.0 * s * s left to right */
    depth -= slope * (float)d;                                                        /* :35 */
    float dz = fabsf(depth - centre) * 16.0f;                                         /* :36 */
    dz = dz * 12.0f / centre;                                                         /* :38 */
    return (float)exp2((double)(-(float)(d * d) * falloff - dz * dz));                /* :40 */
}

/* The weights of the 2R+1 taps of one texel from its depth cache (index R is the centre, weight 1).
 * CrossBilateralBlur.ps.slang:45-57 and :80-85. */
void post_blur_weights(const float* cache, int R, int better, float* w)
{
    const float left = cache[R] - cache[R - 1];                                       /* :80 */
    const float right = cache[R + 1] - cache[R];                                      /* :81 */
    const float min_slope = fabsf(left) < fabsf(right) ? left : right;                /* :82 */
    w[R] = 1.0f;
    for (int dir = 1; dir >= -1; dir -= 2) {                                          /* :84-85 */
        float slope = dir > 0 ? min_slope : -min_slope;
        for (unsigned d = 1; d <= (unsigned)R; ++d) {
            const float depth = cache[R + dir * (int)d];
            if (d == 1 && !better) slope = depth - cache[R];                          /* :53 */
            w[R + dir * (int)d] = blur_weight(R, depth, cache[R], slope, d);
        }
    }
}

static void blur_pass(const uint8_t* src, int texel, const float* z, int zw, int zh, uint8_t* dst, int W, int H,
                      int g, int R, int better, float dirx, float diry)
{
    const float lox = ((float)g + 0.5f) / (float)W, loy = ((float)g + 0.5f) / (float)H;            /* GuardBand.cpp:62 */
    const float hix = ((float)W - ((float)g + 0.5f)) / (float)W, hiy = ((float)H - ((float)g + 0.5f)) / (float)H;
    const float dux = 1.0f / (float)W * dirx, duy = 1.0f / (float)H * diry;                        /* :64 */
    float zc[41], ac[41], w[41];
    for (int y = g; y < H - g; ++y)                                                                /* scissor */
        for (int x = g; x < W - g; ++x) {
            const float tx = centre_uv(x, W), ty = centre_uv(y, H);
            for (int d = -R; d <= R; ++d) {                                                        /* :68-73 */
                const float u = h_clamp(tx + (float)d * dux, lox, hix);
                const float v = h_clamp(ty + (float)d * duy, loy, hiy);
                zc[R + d] = z[(size_t)point_index(v, zh) * zw + point_index(u, zw)];
                ac[R + d] = ld_unorm8(src[((size_t)point_index(v, H) * W + point_index(u, W)) * texel]);
            }
            post_blur_weights(zc, R, better, w);
            float ao = ac[R], sum = 1.0f;                                                          /* :76-77 */
            for (int dir = 1; dir >= -1; dir -= 2)
                for (int d = 1; d <= R; ++d) {
                    ao += w[R + dir * d] * ac[R + dir * d];                                        /* :41 */
                    sum += w[R + dir * d];                                                         /* :42 */
                }
            dst[(size_t)y * W + x] = st_unorm8(ao / sum);                                          /* :87 */
        }
}

/* src: W x H texels of `texel` bytes (byte 0 is read, `.x`); pingpong / dst: W x H bytes, written in the scissor */
void post_blur(const uint8_t* src, int texel, const float* z, int zw, int zh, uint8_t* pingpong, uint8_t* dst,
               int W, int H, int g, int R, int better)
{
    blur_pass(src, texel, z, zw, zh, pingpong, W, H, g, R, better, 1.0f, 0.0f);
    blur_pass(pingpong, 1, z, zw, zh, dst, W, H, g, R, better, 0.0f, 1.0f);
}

/* ------------------------------------------------------------------------------------------------ TAA
 * TAA.ps.slang:45-148; RGBToYCgCo / YCgCoToRGB ColorHelpers.slang:79-98; gSampler linear / wrap (T2). */
typedef struct { float x, y, z; } v3;

static float dot3(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static v3 to_ycgco(const float* c)
{
    const v3 rgb = {c[0], c[1], c[2]};
    const v3 ky = {0.25f, 0.50f, 0.25f}, kg = {-0.25f, 0.50f, -0.25f}, ko = {0.50f, 0.00f, -0.50f};
    const v3 r = {dot3(rgb, ky), dot3(rgb, kg), dot3(rgb, ko)};                       /* ColorHelpers.slang:81-83 */
    return r;
}
static const float kZero4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
static const float* load4(const float* t, int W, int H, int x, int y)                 /* T4 */
{
    return (x < 0 || y < 0 || x >= W || y >= H) ? kZero4 : t + 4 * ((size_t)y * W + x);
}
static v3 sample_rgb_wrap(const float* t, int W, int H, float u, float v)             /* T2, wrap */
{
    const lin_axis ax = linear_axis(u, W), ay = linear_axis(v, H);
    const float* t00 = t + 4 * ((size_t)wrapi(ay.i0, H) * W + wrapi(ax.i0, W));
    const float* t10 = t + 4 * ((size_t)wrapi(ay.i0, H) * W + wrapi(ax.i1, W));
    const float* t01 = t + 4 * ((size_t)wrapi(ay.i1, H) * W + wrapi(ax.i0, W));
    const float* t11 = t + 4 * ((size_t)wrapi(ay.i1, H) * W + wrapi(ax.i1, W));
    v3 r;
    r.x = blend(t00[0], t10[0], t01[0], t11[0], ax.w, ay.w);
    r.y = blend(t00[1], t10[1], t01[1], t11[1], ax.w, ay.w);
    r.z = blend(t00[2], t10[2], t01[2], t11[2], ax.w, ay.w);
    return r;
}

/* TAA.ps.slang:48-62 along one axis: the weights w0, w12, w3 and the coordinates tc0, tc12, tc3 (in uv) */
void post_catmull_rom_axis(float sample_pos, float size, float* w /*[4]: w0 w1 w2 w3*/, float* tc /*[3]*/)
{
    const float inv = 1.0f / size;                                                    /* :47 */
    const float c = floorf(sample_pos - 0.5f) + 0.5f;                                 /* :48 */
    const float f = sample_pos - c, f2 = f * f, f3 = f2 * f;                          /* :49-51 */
    w[0] = f2 - 0.5f * (f3 + f);                                                      /* :53 */
    w[1] = 1.5f * f3 - 2.5f * f2 + 1.0f;                                              /* :54 */
    w[3] = 0.5f * (f3 - f2);                                                          /* :55 */
    w[2] = 1.0f - w[0] - w[1] - w[3];                                                 /* :56 */
    const float w12 = w[1] + w[2];                                                    /* :58 */
    tc[0] = (c - 1.0f) * inv;                                                         /* :60 */
    tc[1] = (c + w[2] / w12) * inv;                                                   /* :61 */
    tc[2] = (c + 2.0f) * inv;                                                         /* :62 */
}

void post_taa(const float* color, const float* mvec, const float* prev, int W, int H, float alpha0, float box,
              int anti_flicker, float* out)
{
    static const int off[8][2] = {{-1, -1}, {-1, 1}, {1, -1}, {1, 1}, {1, 0}, {0, -1}, {0, 1}, {-1, 0}};  /* :81-87 */
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float tcx = ((float)x + 0.5f) / (float)W, tcy = ((float)y + 0.5f) / (float)H;
            const v3 col = to_ycgco(load4(color, W, H, x, y));                        /* :99-100 */
            v3 avg = col, var = {col.x * col.x, col.y * col.y, col.z * col.z};        /* :101-102 */
            for (int k = 0; k < 8; ++k) {                                             /* :104-110 */
                const v3 c = to_ycgco(load4(color, W, H, x + off[k][0], y + off[k][1]));
                avg.x += c.x; avg.y += c.y; avg.z += c.z;
                var.x += c.x * c.x; var.y += c.y * c.y; var.z += c.z * c.z;
            }
            const float ninth = 1.0f / 9.0f;                                          /* :112 */
            avg.x *= ninth; avg.y *= ninth; avg.z *= ninth;
            var.x *= ninth; var.y *= ninth; var.z *= ninth;
            const v3 sg = {sqrtf(h_max(0.0f, var.x - avg.x * avg.x)), sqrtf(h_max(0.0f, var.y - avg.y * avg.y)),
                           sqrtf(h_max(0.0f, var.z - avg.z * avg.z))};                /* :116 */
            const v3 lo = {avg.x - box * sg.x, avg.y - box * sg.y, avg.z - box * sg.z};   /* :117 */
            const v3 hi = {avg.x + box * sg.x, avg.y + box * sg.y, avg.z + box * sg.z};   /* :118 */
            const float* own = mvec + 2 * ((size_t)y * W + x);
            float mx = own[0], my = own[1];   /* :121 */
            for (int k = 0; k < 8; ++k) {                                             /* :123-127 */
                const int xx = x + off[k][0], yy = y + off[k][1];
                float nx = 0.0f, ny = 0.0f;                                           /* T4 */
                if (xx >= 0 && yy >= 0 && xx < W && yy < H) {
                    nx = mvec[2 * ((size_t)yy * W + xx)];
                    ny = mvec[2 * ((size_t)yy * W + xx) + 1];
                }
                if (nx * nx + ny * ny > mx * mx + my * my) { mx = nx; my = ny; }
            }
            float wx[4], wy[4], cx[3], cy[3];                                         /* :130 */
            post_catmull_rom_axis((tcx + mx) * (float)W, (float)W, wx, cx);
            post_catmull_rom_axis((tcy + my) * (float)H, (float)H, wy, cy);
            const float ax[3] = {wx[0], wx[1] + wx[2], wx[3]}, ay[3] = {wy[0], wy[1] + wy[2], wy[3]};
            v3 h = {0.0f, 0.0f, 0.0f};
            for (int i = 0; i < 3; ++i)                                               /* :64-73, x outer, y inner */
                for (int j = 0; j < 3; ++j) {
                    const v3 t = sample_rgb_wrap(prev, W, H, cx[i], cy[j]);
                    const float w = ax[i] * ay[j];
                    if (i == 0 && j == 0) { h.x = t.x * w; h.y = t.y * w; h.z = t.z * w; }
                    else { h.x = h.x + t.x * w; h.y = h.y + t.y * w; h.z = h.z + t.z * w; }
                }
            const float hrgb[3] = {h.x, h.y, h.z};
            v3 hist = to_ycgco(hrgb);                                                 /* :132 */
            float alpha = alpha0;                                                     /* :134 */
            if (anti_flicker) {                                                       /* :139-143 */
                const float dist = h_min(fabsf(lo.x - hist.x), fabsf(hi.x - hist.x));
                alpha = h_clamp((alpha0 * dist) / (dist + hi.x - lo.x), 0.0f, 1.0f);
            }
            hist.x = h_clamp(hist.x, lo.x, hi.x);                                     /* :145 */
            hist.y = h_clamp(hist.y, lo.y, hi.y);
            hist.z = h_clamp(hist.z, lo.z, hi.z);
            const v3 l = {hist.x + alpha * (col.x - hist.x), hist.y + alpha * (col.y - hist.y),
                          hist.z + alpha * (col.z - hist.z)};                         /* :146 lerp */
            const float tmp = l.x - l.y;                                              /* ColorHelpers.slang:93-96 */
            float* o = out + 4 * ((size_t)y * W + x);
            o[0] = tmp + l.z;
            o[1] = l.x + l.y;
            o[2] = tmp - l.z;
            o[3] = 1.0f;                                                              /* :147 */
        }
}

/* ------------------------------------------------------------------------- Deinterleave / Interleave
 * Deinterleave.slang:24-43: layer s of a quarter-size array takes src[4 xyQuarter + (s % 4, s / 4)] (T4 outside);
 * Interleave.slang:9-14: out[xy] = src[xy / 4, slice (y % 4) * 4 + x % 4].  Texels are `texel` opaque bytes. */
void post_deinterleave(const uint8_t* src, int W, int H, int texel, uint8_t* dst)
{
    const int qw = (W + 3) / 4, qh = (H + 3) / 4;
    for (int s = 0; s < 16; ++s)
        for (int y = 0; y < qh; ++y)
            for (int x = 0; x < qw; ++x) {
                const int sx = 4 * x + s % 4, sy = 4 * y + s / 4;
                uint8_t* o = dst + (((size_t)s * qh + y) * qw + x) * texel;
                if (sx < W && sy < H) memcpy(o, src + ((size_t)sy * W + sx) * texel, (size_t)texel);
                else memset(o, 0, (size_t)texel);
            }
}

void post_interleave(const uint8_t* src, int W, int H, int texel, uint8_t* dst)
{
    const int qw = (W + 3) / 4, qh = (H + 3) / 4;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int slice = (y % 4) * 4 + x % 4;
            memcpy(dst + ((size_t)y * W + x) * texel, src + (((size_t)slice * qh + y / 4) * qw + x / 4) * texel,
                   (size_t)texel);
        }
}

/* ------------------------------------------------------------------------------------ RayMinMaxLength
 * RayMinMaxLength.ps.slang:6-14 */
void post_ray_min_max_length(const uint32_t* rmin, const uint32_t* rmax, int n, float* out)
{
    for (int i = 0; i < n; ++i) {
        float a, b;
        memcpy(&a, rmin + i, 4);
        memcpy(&b, rmax + i, 4);
        out[i] = rmax[i] == 0u ? 0.0f : h_max(0.0f, b - a) / 32.0f;
    }
}

/* -------------------------------------------------------------------------------------- AOFlickerMask
 * AOFlickerMask.ps.slang:14-81.  flags (optional): bit 0 a neighbour outside the image, bit 1 a zero offset
 * (normalize gives NaN) among the four, bits 2 / 3 dx / dy above the threshold. */
static v3 uv_to_view(float u, float v, float depth, float sx, float sy)               /* :14-19 */
{
    const float nx = u * 2.0f - 1.0f, ny = (1.0f - v) * 2.0f - 1.0f;
    const v3 r = {nx * depth * sx, ny * depth * sy, -depth};
    return r;
}
static float plane_diff(v3 p, v3 n, v3 q, int* zero)                                  /* :39-43 */
{
    const v3 d = {p.x - q.x, p.y - q.y, p.z - q.z};
    const float len2 = dot3(d, d);
    const float inv = 1.0f / sqrtf(len2);                                             /* normalize = v * rsqrt(dot) */
    const v3 u = {d.x * inv, d.y * inv, d.z * inv};
    if (len2 == 0.0f) *zero = 1;
    return fabsf(dot3(u, n));
}

void post_flicker_mask(const float* z, const float* normal_w, int W, int H, const float* view_mat, float frame_w,
                       float frame_h, float focal, uint8_t* mask, uint8_t* flags, float* dxy)
{
    const float sx = 0.5f * (frame_w / focal), sy = 0.5f * (frame_h / focal);         /* :17 */
    static const int nb[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};                   /* right, left, down, up */
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float* n = normal_w + 4 * ((size_t)y * W + x);
            const v3 nv = {view_mat[0] * n[0] + view_mat[1] * n[1] + view_mat[2] * n[2],
                           view_mat[4] * n[0] + view_mat[5] * n[1] + view_mat[6] * n[2],
                           view_mat[8] * n[0] + view_mat[9] * n[1] + view_mat[10] * n[2]};   /* :49 */
            const v3 P = uv_to_view(h_saturate(((float)x + 0.5f) / (float)W), h_saturate(((float)y + 0.5f) / (float)H),
                                    z[(size_t)y * W + x], sx, sy);                    /* :70 */
            float pd[4];
            int outside = 0, zero = 0;
            for (int k = 0; k < 4; ++k) {
                const int i = x + nb[k][0], j = y + nb[k][1];
                const int out = i < 0 || j < 0 || i >= W || j >= H;
                const float d = out ? 0.0f : z[(size_t)j * W + i];                    /* T4, :50-53 */
                outside |= out;
                const v3 Q = uv_to_view(h_saturate(((float)i + 0.5f) / (float)W),
                                        h_saturate(((float)j + 0.5f) / (float)H), d, sx, sy);   /* :71-74 */
                pd[k] = plane_diff(P, nv, Q, &zero);
            }
            const float dx = h_min(pd[0], pd[1]), dy = h_min(pd[2], pd[3]);           /* :75-76 */
            mask[(size_t)y * W + x] = (dx <= 0.1f && dy <= 0.1f) ? 1 : 0;             /* :78-81 */
            if (flags)
                flags[(size_t)y * W + x] = (uint8_t)(outside | (zero << 1) | (!(dx <= 0.1f) << 2) | (!(dy <= 0.1f) << 3));
            if (dxy) { dxy[2 * ((size_t)y * W + x)] = dx; dxy[2 * ((size_t)y * W + x) + 1] = dy; }
        }
}

/* ------------------------------------------------------------------------------------- BinaryDilation
 * BinaryDilation.ps.slang:8-41: five Gathers (T3, wrap: the unbound sampler S is Falcor's default) */
static unsigned gather_reduce(const uint8_t* t, int W, int H, float u, float v, int op_max)
{
    const lin_axis ax = linear_axis(u, W), ay = linear_axis(v, H);
    const int xs[2] = {wrapi(ax.i0, W), wrapi(ax.i1, W)}, ys[2] = {wrapi(ay.i0, H), wrapi(ay.i1, H)};
    unsigned r = t[(size_t)ys[0] * W + xs[0]];
    for (int k = 1; k < 4; ++k) {
        const unsigned c = t[(size_t)ys[k >> 1] * W + xs[k & 1]];
        r = op_max ? (c > r ? c : r) : (c < r ? c : r);                               /* :8-11 */
    }
    return r;
}

void post_binary_dilation(const uint8_t* in, int W, int H, int op_max, uint8_t* out)
{
    const float hx = 0.5f / (float)W, hy = 0.5f / (float)H;                           /* :18 */
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float u = centre_uv(x, W), v = centre_uv(y, H);
            const float pts[5][2] = {{u + hx, v + 3.0f * hy},                         /* :30 */
                                     {u + 3.0f * hx, v + -hy},                        /* :31 */
                                     {u + -hx, v + -3.0f * hy},                       /* :32 */
                                     {u + -3.0f * hx, v + hy},                        /* :33 */
                                     {u, v}};                                         /* :35 */
            unsigned r = gather_reduce(in, W, H, pts[0][0], pts[0][1], op_max);
            for (int k = 1; k < 5; ++k) {
                const unsigned c = gather_reduce(in, W, H, pts[k][0], pts[k][1], op_max);
                r = op_max ? (c > r ? c : r) : (c < r ? c : r);
            }
            out[(size_t)y * W + x] = (uint8_t)r;
        }
}

/* ----------------------------------------------------------------------------------------- TemporalAO
 * TemporalAO.ps.slang:23-100; gAOSampler linear / clamp (T2), gDepthSampler at texC is the texel itself.
 * flags (optional), one byte per texel of the scissor: 1 outside the valid area, 2 depth test failed,
 * 4 stable pixel, 8 accumulated. */
static float sample_unorm8_clamp(const uint8_t* t, int W, int H, float u, float v)
{
    const lin_axis ax = linear_axis(u, W), ay = linear_axis(v, H);
    const int x0 = clampi(ax.i0, 0, W - 1), x1 = clampi(ax.i1, 0, W - 1);
    const int y0 = clampi(ay.i0, 0, H - 1), y1 = clampi(ay.i1, 0, H - 1);
    return blend(ld_unorm8(t[(size_t)y0 * W + x0]), ld_unorm8(t[(size_t)y0 * W + x1]), ld_unorm8(t[(size_t)y1 * W + x0]),
                 ld_unorm8(t[(size_t)y1 * W + x1]), ax.w, ay.w);
}

void post_temporal_ao(const uint8_t* ao_in, const float* z, const float* mvec, const float* prev_z,
                      const uint8_t* prev_ao, const uint8_t* prev_n, const uint8_t* stable, int W, int H, int g,
                      float frame_w, float frame_h, float focal, const float* m /* prevViewToCurView, row-major */,
                      uint8_t* ao_out, uint8_t* n_out, uint8_t* flags, float* prev_depth_out)
{
    const float lox = ((float)g + 0.5f) / (float)W, loy = ((float)g + 0.5f) / (float)H;            /* GuardBand.cpp:62 */
    const float hix = ((float)W - ((float)g + 0.5f)) / (float)W, hiy = ((float)H - ((float)g + 0.5f)) / (float)H;
    const float sx = 0.5f * (frame_w / focal), sy = 0.5f * (frame_h / focal);                      /* :41 */
    for (int y = g; y < H - g; ++y)
        for (int x = g; x < W - g; ++x) {
            const size_t o = (size_t)y * W + x;
            const float tx = centre_uv(x, W), ty = centre_uv(y, H);
            const float depth = z[o];                                                 /* :67 */
            float ao = ld_unorm8(ao_in[o]);                                           /* :69 */
            unsigned n = 1;                                                           /* :70 */
            unsigned fl = 0;
            const float u = tx + mvec[2 * o], v = ty + mvec[2 * o + 1];               /* :73-75 */
            if (prev_depth_out) prev_depth_out[o] = NAN;
            if (!(u >= lox && u <= hix && v >= loy && v <= hiy)) {                    /* :25, :75 */
                fl = 1;
            } else {
                const int px = (int)floorf(u * (float)W), py = (int)floorf(v * (float)H);   /* :28-33 */
                const size_t po = (size_t)clampi(py, 0, H - 1) * W + clampi(px, 0, W - 1);
                const float raw = prev_z[po];                                         /* :82 */
                const v3 pv = uv_to_view(u, v, raw, sx, sy);                          /* :83, :38-43 */
                const float cur_z = m[8] * pv.x + m[9] * pv.y + m[10] * pv.z + m[11];  /* row 2 of mul(M, float4(p, 1)) */
                const float prev_depth = -cur_z;                                      /* :84 */
                const int is_stable = stable && stable[o] != 0;                       /* :86; unbound reads 0 */
                const float rel = fabsf(1.0f - prev_depth / depth);                   /* :54-57 */
                if (prev_depth_out) prev_depth_out[o] = prev_depth;
                if (rel < 0.1f && !is_stable) {                                       /* :87 */
                    const float pa = sample_unorm8_clamp(prev_ao, W, H, u, v);        /* :89 */
                    const unsigned pn = prev_n[po];                                   /* :92 */
                    const unsigned grown = pn + 1u;                                   /* uint: 255 + 1 = 256 */
                    ao = ((float)pn * pa + ao) / (float)grown;                        /* :93 */
                    n = grown > 30u ? 30u : grown;                                    /* :94 */
                    fl = 8;
                } else {
                    fl = (rel < 0.1f ? 0u : 2u) | (is_stable ? 4u : 0u);
                }
            }
            ao_out[o] = st_unorm8(ao);
            n_out[o] = (uint8_t)n;
            if (flags) flags[o] = (uint8_t)fl;
        }
}

/* -------------------------------------------------------------------------------------- motion vectors
 * librsd's definition (include/rsd_graph.h) of GBufferRaster.mvec for a static scene: the pixel-centre primary
 * hit P = posW + (z / cos) d projected by the previous camera, mvec = prevUV(P) - uv; behind the previous camera
 * (2, 2); background (0, 0) (GBufferRaster.cpp:176 clears mvec, GBufferRaster.3d.slang:117 writes geometry only).
 * cam / prev: posW[3] U[3] V[3] W[3] nearZ farZ, 14 floats.  raw != 0: z holds the raster depth, background is
 * raw >= 1 and the linear depth is near far / (far + d (near - far)).  pw_ratio (optional): pw |prev W| / |rel|, the cosine of the point's angle to the previous view axis. */
void post_motion_vectors(const float* cam, const float* prev, const float* z, int raw, int W, int H, float* mvec,
                         float* pw_ratio)
{
    const float *pos = cam, *U = cam + 3, *V = cam + 6, *Wv = cam + 9;
    const float near_z = cam[12], far_z = cam[13];
    const float *ppos = prev, *axes[3] = {prev + 3, prev + 6, prev + 9};
    float inv_axes[3][3];
    for (int a = 0; a < 3; ++a) {                                                     /* axis / |axis|^2, once, in double */
        const double l2 = (double)axes[a][0] * axes[a][0] + (double)axes[a][1] * axes[a][1] + (double)axes[a][2] * axes[a][2];
        for (int k = 0; k < 3; ++k) inv_axes[a][k] = (float)(axes[a][k] / l2);
    }
    const v3 w = {Wv[0], Wv[1], Wv[2]}, pwv = {prev[9], prev[10], prev[11]};
    const float prev_w_len = sqrtf(dot3(pwv, pwv));
    const float winv = 1.0f / sqrtf(dot3(w, w));
    const v3 wn = {w.x * winv, w.y * winv, w.z * winv};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t o = (size_t)y * W + x;
            float depth = z[o];
            int background;
            if (raw) {
                background = !(depth < 1.0f);
                depth = near_z * far_z / (far_z + depth * (near_z - far_z));
            } else {
                background = !(depth < far_z);
            }
            if (pw_ratio) pw_ratio[o] = NAN;
            if (background) { mvec[2 * o] = 0.0f; mvec[2 * o + 1] = 0.0f; continue; }
            const float u = centre_uv(x, W), v = centre_uv(y, H);
            const float a = 2.0f * u + -1.0f, b = -2.0f * v + 1.0f;
            const v3 dir = {a * U[0] + b * V[0] + Wv[0], a * U[1] + b * V[1] + Wv[1], a * U[2] + b * V[2] + Wv[2]};
            const float dinv = 1.0f / sqrtf(dot3(dir, dir));
            const v3 d = {dir.x * dinv, dir.y * dinv, dir.z * dinv};
            const float t = depth / dot3(wn, d);
            const v3 rel = {pos[0] + t * d.x - ppos[0], pos[1] + t * d.y - ppos[1], pos[2] + t * d.z - ppos[2]};
            const v3 iu = {inv_axes[0][0], inv_axes[0][1], inv_axes[0][2]}, iv = {inv_axes[1][0], inv_axes[1][1], inv_axes[1][2]},
                     iw = {inv_axes[2][0], inv_axes[2][1], inv_axes[2][2]};
            const float pa = dot3(rel, iu), pb = dot3(rel, iv), pw = dot3(rel, iw);
            if (pw_ratio) pw_ratio[o] = pw * prev_w_len / sqrtf(dot3(rel, rel));
            float* out = mvec + 2 * o;
            out[0] = out[1] = 2.0f;                                                   /* behind the previous camera */
            if (pw > 0.0f) {
                const float ndc_x = pa / pw, ndc_y = pb / pw;                         /* previous NDC, y up */
                out[0] = (ndc_x + 1.0f) * 0.5f - u;                                   /* previous uv - uv */
                out[1] = (1.0f - ndc_y) * 0.5f - v;
            }
        }
}

/* the pieces the known-answer tests ask for one at a time */
uint8_t post_store_unorm8(float x) { return st_unorm8(x); }
float post_hlsl_min(float a, float b) { return h_min(a, b); }
float post_hlsl_max(float a, float b) { return h_max(a, b); }
void post_linear_axis(float uv, int n, int* i0, float* w) { const lin_axis a = linear_axis(uv, n); *i0 = a.i0; *w = a.w; }
float post_sample_unorm8_clamp(const uint8_t* t, int W, int H, float u, float v) { return sample_unorm8_clamp(t, W, H, u, v); }
