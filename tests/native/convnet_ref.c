/* convnet_ref.c -- the scalar CPU checker of the ConvolutionalNet tests: a restatement of the pass's semantics written
 * from its specification (the issue text restating ConvolutionNet.h:115-231 and ConvolutionalNet.cpp:131-235); it shares
 * no code with csrc/convnet.hip.  Built by tests/convnet_checker.py with -ffp-contract=off and SSE arithmetic: every
 * multiply and every add rounds on its own, in the order the reference's generated shader performs them.
 *
 *   out(x, y)   = act_L( bias + sum over terms of in(x + a - K/2, y + b - K/2, c) * w[a][b][c][co] )
 *   term order  : input channel (the first layer) or group of 4 input channels (the others), then b (y), then a (x),
 *                 then the channel inside the group; channels beyond Cin are skipped
 *   in          : the first layer reads the four inputs (0 outside the image), the others the previous layer's stored
 *                 activations (0 outside the scissor, which lies inside the image)
 *   act         : ReLU, except the last layer: clamp into [dark, bright] or nothing; only its channel 0 is output
 *
 * Besides the output it returns every intermediate (as the float values a reader of the stored format sees), counters
 * that tell whether the inputs reach every case, and a forward error bound per output texel for an implementation that
 * sums the same terms in any order with or without fused multiply-adds:
 *   bound_out = sum |w| * bound_in + gamma(n + 1) * (|bias| + sum |w * x|),  gamma(n) = n u / (1 - n u),  u = 2^-24,
 * n the number of terms; ReLU and the clamp (both 1-Lipschitz) leave it unchanged. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { C_WRITTEN, C_RELU_CLIPPED, C_RELU_PASSED, C_CLAMP_LOW, C_CLAMP_HIGH, C_CLAMP_INSIDE, C_TAP_OUTSIDE_IMAGE,
       C_TAP_OUTSIDE_SCISSOR, C_COUNT };

static float half_round(float f) { /* float -> binary16 (round to nearest even) -> float */
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = x & 0x80000000u;
    uint32_t m = x & 0x7fffffffu;
    float r;
    if (m >= 0x7f800000u) return f;                 /* inf, NaN */
    if (m >= 0x477ff000u) {                         /* >= 65520: rounds to infinity */
        m = 0x7f800000u;
    } else if (m < 0x38800000u) {                   /* below 2^-14: a multiple of 2^-24 */
        float a;
        memcpy(&a, &m, 4);
        a = nearbyintf(a * 16777216.0f) / 16777216.0f; /* both exact: power-of-two scalings, ties to even */
        memcpy(&m, &a, 4);
    } else {                                        /* keep 10 mantissa bits */
        const uint32_t rem = m & 0x1fffu, keep = m & ~0x1fffu;
        m = keep;
        if (rem > 0x1000u || (rem == 0x1000u && (keep & 0x2000u))) m += 0x2000u;
    }
    m |= sign;
    memcpy(&r, &m, 4);
    return r;
}

static float unorm_round(float x) { /* an R8Unorm store read back: NaN -> 0, saturate, round half up */
    if (x != x) return 0.0f;
    x = !(x > 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x);
    return (float)(uint8_t)floorf(x * 255.0f + 0.5f) / 255.0f;
}

static float read_input(const void* p, int bytes, size_t i) {
    return bytes == 1 ? (float)((const uint8_t*)p)[i] / 255.0f : ((const float*)p)[i];
}

/* K, Cin, Cout: [L]; w[l]: [S][K][K][Cin][Cout] (axis 0 = x offset); bias[l]: [S][Cout] or NULL; in[c]: [S][qh][qw] of
 * in_bytes[c]-byte texels (NULL beyond Cin[0]); out: [S][qh][qw], prefilled by the caller; inter[l], l < L - 1:
 * [S][Cout[l]][qh][qw], zero-filled by the caller; bound: [S][qh][qw] doubles, zero-filled; g: the scissor. */
void convnet_ref(int L, int S, const int* K, const int* Cin, const int* Cout, const float* const* w,
                 const float* const* bias, int qw, int qh, int g, const void* const* in, const int* in_bytes,
                 int precision, int clamp_output, float* out, float* const* inter, double* bound, uint64_t* counters) {
    const size_t plane = (size_t)qw * qh;
    const double u = ldexp(1.0, -24);
    double* bprev = NULL; /* error bounds of the previous layer's activations, [S][C][qh][qw] */
    memset(counters, 0, C_COUNT * sizeof(uint64_t));
    if (2 * g >= qw || 2 * g >= qh) return;
    for (int l = 0; l < L; ++l) {
        const int k = K[l], ci = Cin[l], co_n = Cout[l], last = l == L - 1;
        const int group = l == 0 ? 1 : 4;
        const int n_terms = ci * k * k;
        const double gamma = (n_terms + 1) * u / (1.0 - (n_terms + 1) * u);
        double* bcur = last ? NULL : (double*)calloc((size_t)S * co_n * plane, sizeof(double));
        for (int s = 0; s < S; ++s)
            for (int y = g; y < qh - g; ++y)
                for (int x = g; x < qw - g; ++x)
                    for (int co = 0; co < (last ? 1 : co_n); ++co) {
                        const float bi = bias[l] ? bias[l][(size_t)s * co_n + co] : 0.0f;
                        float o = bi;
                        double eb = 0.0, mag = fabs((double)bi);
                        for (int c0 = 0; c0 < ci; c0 += group)
                            for (int b = 0; b < k; ++b)
                                for (int a = 0; a < k; ++a)
                                    for (int sub = 0; sub < group; ++sub) {
                                        const int c = c0 + sub;
                                        const int xx = x + a - k / 2, yy = y + b - k / 2;
                                        float v = 0.0f;
                                        double vb = 0.0;
                                        if (c >= ci) continue;
                                        const float wt = w[l][((((size_t)s * k + a) * k + b) * ci + c) * co_n + co];
                                        if (l == 0) {
                                            if (xx < 0 || xx >= qw || yy < 0 || yy >= qh) {
                                                if (co == 0) counters[C_TAP_OUTSIDE_IMAGE]++;
                                            } else {
                                                v = read_input(in[c], in_bytes[c], (size_t)s * plane + (size_t)yy * qw + xx);
                                            }
                                        } else if (xx < g || xx >= qw - g || yy < g || yy >= qh - g) {
                                            if (co == 0) counters[C_TAP_OUTSIDE_SCISSOR]++;
                                        } else {
                                            const size_t i = ((size_t)s * ci + c) * plane + (size_t)yy * qw + xx;
                                            v = inter[l - 1][i];
                                            vb = bprev[i];
                                        }
                                        {
                                            const float p = v * wt;
                                            o = o + p;
                                        }
                                        eb += fabs((double)wt) * vb;
                                        mag += fabs((double)wt * (double)v);
                                    }
                        eb += gamma * mag;
                        const size_t centre = (size_t)s * plane + (size_t)y * qw + x;
                        if (last) {
                            if (clamp_output) {
                                const float dark = read_input(in[1], in_bytes[1], centre);
                                const float bright = read_input(in[0], in_bytes[0], centre);
                                float r = o;
                                if (!(r >= dark)) r = dark;    /* max(v, dark): a NaN gives dark */
                                if (!(r <= bright)) r = bright; /* min(., bright): dark > bright gives bright */
                                if (o < dark) counters[C_CLAMP_LOW]++;
                                else if (o > bright) counters[C_CLAMP_HIGH]++;
                                else counters[C_CLAMP_INSIDE]++;
                                o = r;
                            }
                            out[centre] = o;
                            bound[centre] = eb;
                            counters[C_WRITTEN]++;
                        } else {
                            float r = o > 0.0f ? o : 0.0f; /* max(0, v): a NaN gives 0 */
                            if (o < 0.0f) counters[C_RELU_CLIPPED]++;
                            else if (o > 0.0f) counters[C_RELU_PASSED]++;
                            if (precision == 1) r = half_round(r);
                            else if (precision == 2) r = unorm_round(r);
                            inter[l][((size_t)s * co_n + co) * plane + (size_t)y * qw + x] = r;
                            bcur[((size_t)s * co_n + co) * plane + (size_t)y * qw + x] = eb;
                        }
                    }
        free(bprev);
        bprev = bcur;
    }
    free(bprev);
}
