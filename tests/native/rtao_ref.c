/*
 * rtao_ref.c -- CPU statement of the RTAO semantics (include/rsd.h rsd_rtao, rsd_gbuffer_world), the checker
 * of tests/test_rtao.py and tests/test_gpu_rtao.py.
 *
 * TEST INFRASTRUCTURE ONLY; it shares no code with librsd.  Brute force over ALL triangles per ray (no BVH)
 * with the oracle's watertight test (ocpu_intersect) and alpha test (ocpu_alpha_fails), threaded over rays:
 *   rtao_mt_ref      raw draws of MT19937 (Matsumoto & Nishimura 1998, the 2002 initialisation), written out here
 *   rtao_table_ref   the pass's 5312 RGBA8Snorm samples: two draws of mt19937(89) per entry, each
 *                    u = (float)raw * 2^-32 with u >= 1 replaced by nextafterf(1, 0); phi = u.y * 2 * pi,
 *                    t = sqrt(1 - u.x), s = sqrt(1 - t^2), (s cos phi, s sin phi, t, 0) packed as
 *                    round(clamp(v, -1, 1) * 127)
 *   rtao_hash_ref    jenkins(x * 449 + y * 2857 + jenkins(frame))
 *   rtao_origins_ref origin = posW.xyz + n * normalScale with n = normalize(faceNormal.xyz); w = 1, or all 0
 *                    where posW.w == 0
 *   rtao_dirs_ref    the spp = 1 directions: entry hash % 5312 of the table, decoded max(c / 127, -1), in the
 *                    frame bitangent = |n.x| > |n.y| ? (-n.z, 0, n.x) : (0, n.z, -n.y), tangent =
 *                    cross(bitangent, n): normalize(tangent s.x + bitangent s.y + n s.z)
 *   rtao_trace_ref   per ray the hit with the smallest (t, prim) in [0.001, tmax], no culling, alpha test at
 *                    LOD 0 for triangles whose flags carry bit 2: its t, or 0 on a miss
 *   rtao_posw_ref    the world position (o + d t, 1) of the pixel-centre primary ray's closest hit in
 *                    [nearZ / cos, farZ / cos] with culling and alpha test (rsd_gbuffer_raster's hit), 0 on a miss
 * normalize(v) = v * (1 / sqrt(dot(v, v))), dot summed left to right; every operation rounds on its own.
 *
 * Built by the tests with gcc -O2 -ffp-contract=off -pthread against the oracle's shared library.
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>

#include "rsd_oracle.h"

#define RTAO_SAMPLES 5312u

/* ---- MT19937 */
typedef struct {
    uint32_t mt[624];
    int i;
} mt_t;

static void mt_seed(mt_t* m, uint32_t seed)
{
    m->mt[0] = seed;
    for (int k = 1; k < 624; ++k) m->mt[k] = 1812433253u * (m->mt[k - 1] ^ (m->mt[k - 1] >> 30)) + (uint32_t)k;
    m->i = 624;
}

static uint32_t mt_next(mt_t* m)
{
    if (m->i >= 624) {
        for (int k = 0; k < 624; ++k) {
            uint32_t y = (m->mt[k] & 0x80000000u) | (m->mt[(k + 1) % 624] & 0x7fffffffu);
            m->mt[k] = m->mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        m->i = 0;
    }
    uint32_t y = m->mt[m->i++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

void rtao_mt_ref(uint32_t seed, uint32_t n, uint32_t* out)
{
    mt_t m;
    mt_seed(&m, seed);
    for (uint32_t i = 0; i < n; ++i) out[i] = mt_next(&m);
}

static float draw01(mt_t* m)
{
    float u = (float)mt_next(m) * 0x1p-32f;
    return u >= 1.0f ? nextafterf(1.0f, 0.0f) : u;
}

static uint32_t snorm8(float v)
{
    float c = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
    return (uint32_t)(uint8_t)(int8_t)(int)roundf(c * 127.0f);
}

void rtao_table_ref(uint32_t* out)
{
    mt_t m;
    mt_seed(&m, 89u);
    for (uint32_t i = 0; i < RTAO_SAMPLES; ++i) {
        float ux = draw01(&m);
        float uy = draw01(&m);
        float phi = uy * 2.0f * (float)M_PI;
        float t = sqrtf(1.0f - ux);
        float s = sqrtf(1.0f - t * t);
        out[i] = snorm8(s * cosf(phi)) | (snorm8(s * sinf(phi)) << 8) | (snorm8(t) << 16);
    }
}

static uint32_t jenkins_ref(uint32_t a)
{
    a -= (a << 6);
    a ^= (a >> 17);
    a -= (a << 9);
    a ^= (a << 4);
    a -= (a << 3);
    a ^= (a << 10);
    a ^= (a >> 15);
    return a;
}

uint32_t rtao_jenkins_ref(uint32_t a) { return jenkins_ref(a); }

uint32_t rtao_hash_ref(uint32_t x, uint32_t y, uint32_t frame)
{
    return jenkins_ref(x * 449u + y * 2857u + jenkins_ref(frame));
}

/* ---- vectors */
static float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static void normalize3(const float v[3], float r[3])
{
    float inv = 1.0f / sqrtf(dot3(v, v));
    r[0] = v[0] * inv; r[1] = v[1] * inv; r[2] = v[2] * inv;
}

/* origins: float4 per pixel */
void rtao_origins_ref(const float* posW, const float* faceN, uint32_t count, float normalScale, float* origins)
{
    for (uint32_t i = 0; i < count; ++i) {
        float* o = origins + 4 * (size_t)i;
        if (posW[4 * (size_t)i + 3] == 0.0f) {
            o[0] = o[1] = o[2] = o[3] = 0.0f;
            continue;
        }
        float n[3];
        normalize3(faceN + 4 * (size_t)i, n);
        for (int k = 0; k < 3; ++k) o[k] = posW[4 * (size_t)i + k] + n[k] * normalScale;
        o[3] = 1.0f;
    }
}

static float unpack_snorm(uint32_t packed, int k)
{
    float v = (float)(int)(int8_t)(uint8_t)(packed >> (8 * k)) / 127.0f;
    return v > -1.0f ? v : -1.0f;
}

/* dirs: float4 per pixel (w unused, 0); index_shift is added to the table index before the modulo
 * (0 = the pass; the tests use 1 to show that a neighbouring entry gives another frame) */
void rtao_dirs_ref(const float* posW, const float* faceN, uint32_t W, uint32_t H, uint32_t frame,
                   uint32_t index_shift, float* dirs)
{
    uint32_t* table = (uint32_t*)malloc(RTAO_SAMPLES * sizeof(uint32_t));
    rtao_table_ref(table);
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            float* d = dirs + 4 * i;
            d[0] = d[1] = d[2] = d[3] = 0.0f;
            if (posW[4 * i + 3] == 0.0f) continue;
            float n[3], b[3], t[3], v[3];
            normalize3(faceN + 4 * i, n);
            if (fabsf(n[0]) > fabsf(n[1])) { b[0] = -n[2]; b[1] = 0.0f; b[2] = n[0]; }
            else { b[0] = 0.0f; b[1] = n[2]; b[2] = -n[1]; }
            t[0] = b[1] * n[2] - b[2] * n[1];
            t[1] = b[2] * n[0] - b[0] * n[2];
            t[2] = b[0] * n[1] - b[1] * n[0];
            const uint32_t packed = table[(rtao_hash_ref(x, y, frame) + index_shift) % RTAO_SAMPLES];
            const float sx = unpack_snorm(packed, 0), sy = unpack_snorm(packed, 1), sz = unpack_snorm(packed, 2);
            for (int k = 0; k < 3; ++k) v[k] = t[k] * sx + b[k] * sy + n[k] * sz;
            normalize3(v, d);
        }
    free(table);
}

/* ---- tracing */
typedef struct {
    const oscene* s;
    int has_alpha;
    const float* pos;
    const uint32_t* idx;
    const uint32_t* flags;
    uint32_t nt;
    const float* origins;
    const float* dirs;
    uint32_t spp;
    float tmin, tmax;
    float* out;
    uint32_t r0, r1;
} trace_job;

static void* trace_rays(void* arg)
{
    const trace_job* j = (const trace_job*)arg;
    for (uint32_t r = j->r0; r < j->r1; ++r) {
        const float* o = j->origins + 4 * (size_t)(r / j->spp);
        const float* d = j->dirs + 4 * (size_t)r;
        j->out[r] = 0.0f;
        if (o[3] == 0.0f) continue;
        int found = 0;
        float bestT = INFINITY;
        uint32_t bestP = 0xffffffffu;
        for (uint32_t prim = 0; prim < j->nt; ++prim) {
            const float* v0 = j->pos + 3 * (size_t)j->idx[3 * prim];
            const float* v1 = j->pos + 3 * (size_t)j->idx[3 * prim + 1];
            const float* v2 = j->pos + 3 * (size_t)j->idx[3 * prim + 2];
            float t, bu, bv, det;
            if (!ocpu_intersect(o, d, v0, v1, v2, &t, &bu, &bv, &det)) continue;
            if (!(t >= j->tmin && t <= j->tmax)) continue;
            if (found && !(t < bestT || (t == bestT && prim < bestP))) continue;
            if (j->has_alpha && (j->flags[prim] & 4u) && ocpu_alpha_fails(j->s, prim, bu, bv, 0, t, d, 0.0f)) continue;
            found = 1;
            bestT = t;
            bestP = prim;
        }
        if (found) j->out[r] = bestT;
    }
    return NULL;
}

/* origins float4[count] (w == 0: no ray), dirs float4[count * spp]; out float[count * spp].  tmin: the pass's
 * 0.001 (the tests pass 0 to show that TMin matters on their frames). */
void rtao_trace_ref(const oscene* s, int has_alpha, const float* positions, const uint32_t* indices,
                    const uint32_t* flags, uint32_t nt, const float* origins, const float* dirs, uint32_t count,
                    uint32_t spp, float tmin, float tmax, float* out, int nthreads)
{
    const uint32_t rays = count * spp;
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    if ((uint32_t)nthreads > rays) nthreads = (int)(rays ? rays : 1);
    trace_job jobs[64];
    pthread_t th[64];
    for (int i = 0; i < nthreads; ++i) {
        trace_job j = {s, has_alpha, positions, indices, flags, nt, origins, dirs, spp, tmin, tmax, out,
                       (uint32_t)((uint64_t)rays * i / nthreads), (uint32_t)((uint64_t)rays * (i + 1) / nthreads)};
        jobs[i] = j;
        pthread_create(&th[i], NULL, trace_rays, &jobs[i]);
    }
    for (int i = 0; i < nthreads; ++i) pthread_join(th[i], NULL);
}

/* ---- the world-position G-buffer */
static int is_culled(float det, uint32_t flags, uint32_t cull)
{
    if (cull == 0 || (flags & 1u)) return 0;
    int front = (det > 0.0f) != ((flags & 2u) != 0);
    return cull == 1 ? !front : front;
}

void rtao_posw_ref(const oscene* s, int has_alpha, const float* positions, const uint32_t* indices,
                   const uint32_t* flags, uint32_t nt, const ocam* c, uint32_t W, uint32_t H, uint32_t cull,
                   float* posW)
{
    float wn[3];
    normalize3(c->W, wn);
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            float px = ((float)x + 0.5f) / (float)W + -c->jitterX;
            float py = ((float)y + 0.5f) / (float)H + c->jitterY;
            float ndcx = 2.0f * px + -1.0f, ndcy = -2.0f * py + 1.0f;
            float dn[3], d[3];
            for (int k = 0; k < 3; ++k) dn[k] = ndcx * c->U[k] + ndcy * c->V[k] + c->W[k];
            normalize3(dn, d);
            const float invCos = 1.0f / dot3(wn, d);
            const float tmin = c->nearZ * invCos, tmax = c->farZ * invCos;
            int found = 0;
            float bestT = INFINITY;
            uint32_t bestP = 0xffffffffu;
            for (uint32_t prim = 0; prim < nt; ++prim) {
                const float* v0 = positions + 3 * (size_t)indices[3 * prim];
                const float* v1 = positions + 3 * (size_t)indices[3 * prim + 1];
                const float* v2 = positions + 3 * (size_t)indices[3 * prim + 2];
                float t, bu, bv, det;
                if (!ocpu_intersect(c->posW, d, v0, v1, v2, &t, &bu, &bv, &det)) continue;
                if (!(t >= tmin && t <= tmax)) continue;
                if (is_culled(det, flags[prim], cull)) continue;
                if (found && !(t < bestT || (t == bestT && prim < bestP))) continue;
                if (has_alpha && (flags[prim] & 4u) && ocpu_alpha_fails(s, prim, bu, bv, 0, t, d, 0.0f)) continue;
                found = 1;
                bestT = t;
                bestP = prim;
            }
            float* o = posW + 4 * ((size_t)y * W + x);
            if (!found) {
                o[0] = o[1] = o[2] = o[3] = 0.0f;
                continue;
            }
            for (int k = 0; k < 3; ++k) o[k] = c->posW[k] + d[k] * bestT;
            o[3] = 1.0f;
        }
}
