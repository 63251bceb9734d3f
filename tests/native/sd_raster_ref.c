/*
 * sd_raster_ref.c -- CPU statement of the raster StochasticDepthMap semantics (include/rsd.h rsd_sd_raster),
 * the checker of tests/test_sd_raster.py, tests/test_gpu_sd_raster.py and tests/test_gpu_graph_sd_raster.py.
 *
 * TEST INFRASTRUCTURE ONLY; it shares no code with librsd.  A brute-force loop over ALL triangles per SD
 * texel (no BVH, no bounds), threaded over rows:
 *   ray      pixel-centre pinhole ray of the sdW x sdH image, d = normalize(dir((x+.5)/sdW - jitterX,
 *            (y+.5)/sdH + jitterY)), cosT = dot(normalize(W), d), interval [nearZ / cosT, farZ / cosT];
 *   fragment every triangle the oracle's watertight test (ocpu_intersect) accepts in the interval and the
 *            culling keeps;
 *   stencil  (use_stencil) a texel whose mask value -- stencil (bytes) if given, else rayMax -- is 0 gets no
 *            fragment;
 *   discard  1. alpha test at LOD 0 (ocpu_alpha_fails) for triangles whose flags carry bit 2;
 *            2. zlin = t cosT, z = farZ (zlin - nearZ) / (zlin (farZ - nearZ)); z <= firstDepth, the depth
 *               map sampled at ((x+.5)/sdW, (y+.5)/sdH): point for an odd (int)(zW / (float)sdW + .5f),
 *               bilinear (D3D, 8 sub-texel bits) for an even one, wrap addressing;
 *            3. (ray_interval, both maps) posW = o + d t, dist = |posW - o|; rayMin != 0 && dist <=
 *               asfloat(rayMin); rayMax != 0 && dist >= asfloat(rayMax);
 *            4. rng = hash(hash(hash(posW.x, posW.y), posW.z), 1.438943289), R = (int)floor(alpha N + rng);
 *               R == 0; R >= N covers every sample, else the mask is lut[(int)(a + rng2 (b - a))],
 *               rng2 = hash(hash(posW.z, posW.y), posW.x), a = idx[R], b = idx[R + 1];
 *   value    (zlin - nearZ) / (farZ - nearZ) with linearize, else z; a covered sample keeps the minimum.
 * Output [layer][y][x][min(N,4)], cleared to 1.  counters (summed over the frame):
 *   [0] fragments, [1] discarded by the alpha test, [2] by the first layer, [3] by rayMin, [4] by rayMax,
 *   [5] with R == 0, [6] texels stencilled out, [7] texels holding >= 2 distinct values below 1.
 * tests/test_sd_raster.py pins it to the oracle's G-buffers (N = 1, alpha = 1, a zero depth map).
 *
 * Built by the tests with gcc -O2 -ffp-contract=off -pthread against the oracle's shared library.
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "rsd_oracle.h"

typedef struct {
    uint32_t sample_count;
    float alpha;
    uint32_t cull_mode, linearize, alpha_test, implementation, ray_interval, use_stencil;
} sdr_params;

typedef struct {
    const oscene* s;
    int has_alpha;
    const float* pos;
    const uint32_t* idx;
    const uint32_t* flags;
    uint32_t nt;
    const ocam* c;
    const sdr_params* p;
    const float* z;
    uint32_t zW, zH;
    const uint32_t* rmin;
    const uint32_t* rmax;
    const uint8_t* stencil;
    float* out;
    uint32_t W, H;
    const int32_t* lutIdx;
    const uint32_t* lut;
    uint64_t cnt[8];
    uint32_t y0, y1;
} job_t;

static float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static void normalize3(const float v[3], float r[3])
{
    float inv = 1.0f / sqrtf(dot3(v, v));
    r[0] = v[0] * inv; r[1] = v[1] * inv; r[2] = v[2] * inv;
}

/* Camera.slang:73-90 computeNonNormalizedRayDirPinhole */
static void ray_dir(const ocam* c, float px, float py, float out[3])
{
    float ndcx = 2.0f * px + -1.0f;
    float ndcy = -2.0f * py + 1.0f;
    for (int i = 0; i < 3; ++i) out[i] = ndcx * c->U[i] + ndcy * c->V[i] + c->W[i];
}

static int is_culled(float det, uint32_t flags, uint32_t cull)
{
    if (cull == 0 || (flags & 1u)) return 0;
    int front = (det > 0.0f) != ((flags & 2u) != 0);
    return cull == 1 ? !front : front;
}

static int wrap(int i, int n)
{
    i %= n;
    return i < 0 ? i + n : i;
}

static float texel(const float* t, int W, int H, int x, int y) { return t[(size_t)wrap(y, H) * W + wrap(x, W)]; }

/* D3D linear filtering with 8 sub-texel bits, wrap addressing */
static float sample_linear(const float* t, int W, int H, float u, float v)
{
    float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    float fx = floorf(x), fy = floorf(y);
    float qx = floorf((x - fx) * 256.0f + 0.5f), qy = floorf((y - fy) * 256.0f + 0.5f);
    int ix = (int)fx, iy = (int)fy;
    if (qx >= 256.0f) { ix += 1; qx = 0.0f; }
    if (qy >= 256.0f) { iy += 1; qy = 0.0f; }
    float wx = qx * (1.0f / 256.0f), wy = qy * (1.0f / 256.0f);
    float t00 = texel(t, W, H, ix, iy), t10 = texel(t, W, H, ix + 1, iy);
    float t01 = texel(t, W, H, ix, iy + 1), t11 = texel(t, W, H, ix + 1, iy + 1);
    /* a tap of weight 0 drops out exactly (finite texels), as in the oracle's filter */
    if (qx == 0.0f && qy == 0.0f) return t00;
    if (qy == 0.0f) return t00 * (1.0f - wx) + t10 * wx;
    if (qx == 0.0f) return t00 * (1.0f - wy) + t01 * wy;
    float r0 = t00 * (1.0f - wx) + t10 * wx;
    float r1 = t01 * (1.0f - wx) + t11 * wx;
    return r0 * (1.0f - wy) + r1 * wy;
}

static float as_float(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static void* rows(void* arg)
{
    job_t* j = (job_t*)arg;
    const ocam* c = j->c;
    const sdr_params* p = j->p;
    const uint32_t N = p->sample_count, ch = N < 4 ? N : 4;
    const size_t plane = (size_t)j->W * j->H;
    const int div = (int)((float)j->zW / (float)j->W + 0.5f);
    const int interval = p->ray_interval && j->rmin && j->rmax;
    float wn[3];
    normalize3(c->W, wn);
    for (uint32_t y = j->y0; y < j->y1; ++y)
        for (uint32_t x = 0; x < j->W; ++x) {
            const size_t o = (size_t)y * j->W + x;
            float s[16];
            for (uint32_t i = 0; i < N; ++i) s[i] = 1.0f;
            int live = 1;
            if (p->use_stencil) {
                if (j->stencil) live = j->stencil[o] != 0;
                else if (j->rmax) live = j->rmax[o] != 0u;
            }
            if (!live) j->cnt[6]++;
            float u = ((float)x + 0.5f) / (float)j->W, v = ((float)y + 0.5f) / (float)j->H;
            float dn[3], d[3];
            ray_dir(c, u + -c->jitterX, v + c->jitterY, dn);
            normalize3(dn, d);
            const float cosT = dot3(wn, d);
            const float invCos = 1.0f / cosT;
            const float tmin = c->nearZ * invCos, tmax = c->farZ * invCos;
            float fd;
            if (div % 2 == 0) fd = sample_linear(j->z, (int)j->zW, (int)j->zH, u, v);
            else fd = texel(j->z, (int)j->zW, (int)j->zH, (int)floorf(u * (float)j->zW), (int)floorf(v * (float)j->zH));
            const uint32_t iMin = interval ? j->rmin[o] : 0u, iMax = interval ? j->rmax[o] : 0u;
            for (uint32_t prim = 0; live && prim < j->nt; ++prim) {
                const float* v0 = j->pos + 3 * (size_t)j->idx[3 * prim];
                const float* v1 = j->pos + 3 * (size_t)j->idx[3 * prim + 1];
                const float* v2 = j->pos + 3 * (size_t)j->idx[3 * prim + 2];
                float t, bu, bv, det;
                if (!ocpu_intersect(c->posW, d, v0, v1, v2, &t, &bu, &bv, &det)) continue;
                if (!(t >= tmin && t <= tmax)) continue;
                if (is_culled(det, j->flags[prim], p->cull_mode)) continue;
                j->cnt[0]++;
                if (p->alpha_test && j->has_alpha && (j->flags[prim] & 4u) &&
                    ocpu_alpha_fails(j->s, prim, bu, bv, 0, t, d, 0.0f)) { j->cnt[1]++; continue; }
                const float zlin = t * cosT;
                const float z = c->farZ * (zlin - c->nearZ) / (zlin * (c->farZ - c->nearZ));
                if (z <= fd) { j->cnt[2]++; continue; }
                float pw[3], q[3];
                for (int i = 0; i < 3; ++i) { pw[i] = c->posW[i] + d[i] * t; q[i] = pw[i] - c->posW[i]; }
                if (interval) {
                    const float dist = sqrtf(dot3(q, q));
                    if (iMin != 0u && dist <= as_float(iMin)) { j->cnt[3]++; continue; }
                    if (iMax != 0u && dist >= as_float(iMax)) { j->cnt[4]++; continue; }
                }
                const float rng = ocpu_hash(ocpu_hash(ocpu_hash(pw[0], pw[1]), pw[2]), 1.438943289f);
                const int R = (int)floorf(p->alpha * (float)N + rng);
                uint32_t mask = 0xffffu;
                if (R < (int)N) {
                    if (R == 0) { j->cnt[5]++; continue; }
                    const float rng2 = ocpu_hash(ocpu_hash(pw[2], pw[1]), pw[0]);
                    const float a = (float)j->lutIdx[R], b = (float)j->lutIdx[R + 1];
                    mask = j->lut[(int)(a + rng2 * (b - a))];
                }
                const float val = p->linearize ? (zlin - c->nearZ) / (c->farZ - c->nearZ) : z;
                for (uint32_t i = 0; i < N; ++i)
                    if ((mask & (1u << i)) && val < s[i]) s[i] = val;
            }
            int distinct = 0;
            for (uint32_t i = 0; i < N; ++i) {
                if (!(s[i] < 1.0f)) continue;
                int seen = 0;
                for (uint32_t k = 0; k < i; ++k) seen |= s[k] == s[i];
                distinct += !seen;
            }
            if (distinct >= 2) j->cnt[7]++;
            for (uint32_t i = 0; i < N; ++i) j->out[(i / 4) * plane * ch + o * ch + i % 4] = s[i];
        }
    return NULL;
}

/* s: the oracle scene of the same geometry (read by ocpu_alpha_fails only); has_alpha: it holds alpha
 * materials.  positions float3[], indices uint32[3 nt], flags uint32[nt].  rmin / rmax / stencil may be NULL. */
void sd_raster_ref(const oscene* s, int has_alpha, const float* positions, const uint32_t* indices,
                   const uint32_t* flags, uint32_t nt, const ocam* cam, const sdr_params* p, const float* depth,
                   uint32_t zW, uint32_t zH, const uint32_t* rmin, const uint32_t* rmax, const uint8_t* stencil,
                   float* out, uint32_t sdW, uint32_t sdH, uint64_t counters[8], int nthreads)
{
    const uint32_t N = p->sample_count;
    int32_t lutIdx[17];
    uint32_t* lut = (uint32_t*)malloc(sizeof(uint32_t) << N);
    ocpu_stratified_lut((int)N, lutIdx, lut);
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    if ((uint32_t)nthreads > sdH) nthreads = (int)sdH;
    job_t jobs[64];
    pthread_t th[64];
    for (int i = 0; i < nthreads; ++i) {
        job_t j = {s, has_alpha, positions, indices, flags, nt, cam, p, depth, zW, zH, rmin, rmax, stencil, out, sdW,
                   sdH, lutIdx, lut, {0}, (uint32_t)((uint64_t)sdH * i / nthreads),
                   (uint32_t)((uint64_t)sdH * (i + 1) / nthreads)};
        jobs[i] = j;
        pthread_create(&th[i], NULL, rows, &jobs[i]);
    }
    for (int k = 0; k < 8; ++k) counters[k] = 0;
    for (int i = 0; i < nthreads; ++i) {
        pthread_join(th[i], NULL);
        for (int k = 0; k < 8; ++k) counters[k] += jobs[i].cnt[k];
    }
    free(lut);
}
